"""What --exclude costs: BDX_TIMING=1 bin/breakdancer-max on a write_genome_bam file (default 1/64 of hg38's lengths: 14.5 M records,
~2 GB, the size of bench.py --full's BAM -> table leg) three ways, in alternating rounds -- a built copy of the parent commit
(--parent-exe, its libbdx.so beside it as the Makefile's rpath expects), this tree without the option, this tree with a 1,000-interval
BED that masks under 1 % of the records.  Decode-stage and whole-run seconds of the timing line, median / min / max of seven rounds
(an eighth, the first, warms up and is not counted) -> <out>/exclude_measurement.json, the last round's stderr beside it.
    python tools/exclude_ab.py --parent-exe ../parent/bin/breakdancer-max --out profiles/exclude_ab"""
import argparse, json, os, re, shutil, statistics, struct, subprocess, sys, tempfile, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from breakdancer_amd.bamwrite import write_genome_bam

ap = argparse.ArgumentParser()
ap.add_argument("--parent-exe", required=True)
ap.add_argument("--out", required=True)
ap.add_argument("--fraction", type=float, default=1.0 / 64)
a = ap.parse_args()
out_dir = os.path.abspath(a.out)
os.makedirs(out_dir, exist_ok=True)
td = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    t0 = time.time()
    bam, cfg, n = write_genome_bam(td, a.fraction)
    print("wrote %s: %d records, %.2f GB in %.1f s" % (bam, n, os.path.getsize(bam) / 1e9, time.time() - t0), flush=True)
    head = zlib.decompressobj(31).decompress(open(bam, "rb").read(1 << 20))
    l_text, = struct.unpack_from("<i", head, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", head, o)
    o += 4
    names, lens = [], []
    for _ in range(n_ref):
        l, = struct.unpack_from("<i", head, o)
        names.append(head[o + 4:o + 4 + l - 1].decode())
        lens.append(struct.unpack_from("<i", head, o + 4 + l)[0])
        o += 8 + l
    # the header's lengths are nominal: place the intervals within what the generator used
    from breakdancer_amd.bamwrite import HG38_MBP
    real = [int(m * 1e6 * a.fraction) for m in HG38_MBP]
    rng = np.random.default_rng(5)
    w = np.array(real, float) / sum(real)
    with open(os.path.join(td, "mask.bed"), "w") as f:
        for _ in range(1000):
            t = int(rng.choice(len(real), p=w))
            b = int(rng.integers(0, real[t] - 200))
            f.write("%s\t%d\t%d\n" % (names[t], b, b + 200))
    variants = [("parent", os.path.abspath(a.parent_exe), []),
                ("head", os.path.join(ROOT, "bin", "breakdancer-max"), []),
                ("head+exclude", os.path.join(ROOT, "bin", "breakdancer-max"), ["--exclude", "mask.bed"])]
    res = {v[0]: dict(decode=[], total=[], wall=[]) for v in variants}
    tables = {}
    excluded = None
    for rep in range(8):   # (the first round warms the page cache and the driver: not counted)
        for name, exe, extra in variants:
            t0 = time.time()
            p = subprocess.run(["timeout", "-k", "10", "120", exe] + extra + [os.path.basename(cfg)], cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               env=dict(os.environ, BDX_TIMING="1", BDX_FOREGROUND="1"))
            wall = time.time() - t0
            err = p.stderr.decode()
            if p.returncode != 0:
                print(name, "FAILED", p.returncode, err[-2000:], flush=True)
                sys.exit(1)
            m = re.search(r"decode\+merge\+stream=([0-9.]+)s.*total=([0-9.]+)s", err)
            x = re.search(r"excluded (\d+) records in (\d+) intervals", err)
            if x:
                excluded = (int(x.group(1)), int(x.group(2)))
            tables.setdefault(name, set()).add("\n".join(l for l in p.stdout.decode().splitlines() if not l.startswith(("#Command", "#Software"))))
            if rep:
                res[name]["decode"].append(float(m.group(1))); res[name]["total"].append(float(m.group(2))); res[name]["wall"].append(wall)
            if rep == 7:
                open(os.path.join(out_dir, "timing_%s.txt" % name.replace("+", "_")), "w").write(err)
    summary = {"records": n, "bam_bytes": os.path.getsize(bam), "excluded_records_intervals": excluded, "runs_each": 7,
               "parent_table_equals_head_table": tables["parent"] == tables["head"], "tables_per_variant": {k: len(v) for k, v in tables.items()}}
    for name in res:
        summary[name] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), all=v) for k, v in res[name].items()}
    json.dump(summary, open(os.path.join(out_dir, "exclude_measurement.json"), "w"), indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) or "decode" not in v else {q: (v[q]["median"], v[q]["min"], v[q]["max"]) for q in v}) for k, v in summary.items()}, indent=1))
finally:
    shutil.rmtree(td, ignore_errors=True)
