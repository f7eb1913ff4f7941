"""Is the CLI as fast as its parent commit's?  BDX_TIMING=1 BDX_FOREGROUND=1 bin/breakdancer-max on write_genome_bam files (as
tools/exclude_ab.py: 1/64 of hg38's lengths is the size of bench.py --full's BAM -> table leg; 1/32 prints a table above 8,192 rows, so
that the several-thread writer is what formats it), from a built copy of the parent commit (--parent-exe, its libbdx.so beside it as
the Makefile's rpath expects) and from this tree in alternating rounds, parent first.  Decode-stage, format and whole-run seconds of
the timing line, median / min / max of seven rounds (an eighth, the first, warms up and is not counted) -> --out, a JSON file.
    python tools/cli_parent_ab.py --parent-exe ../parent/bin/breakdancer-max --out profiles/cli_ab.json"""
import argparse, json, os, re, shutil, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from breakdancer_amd.bamwrite import write_genome_bam

ap = argparse.ArgumentParser()
ap.add_argument("--parent-exe", required=True)
ap.add_argument("--out", required=True)
ap.add_argument("--fractions", default="0.015625,0.03125")
ap.add_argument("--rounds", type=int, default=8)
a = ap.parse_args()
variants = [("parent", os.path.abspath(a.parent_exe)), ("head", os.path.join(ROOT, "bin", "breakdancer-max"))]
summary = {"runs_each": a.rounds - 1, "legs": {}}
for fraction in [float(f) for f in a.fractions.split(",")]:
    td = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        t0 = time.time()
        bam, cfg, n = write_genome_bam(td, fraction)
        print("wrote %s: %d records, %.2f GB in %.1f s" % (bam, n, os.path.getsize(bam) / 1e9, time.time() - t0), flush=True)
        res = {v[0]: dict(decode=[], format=[], total=[], wall=[]) for v in variants}
        tables = {v[0]: set() for v in variants}
        for rep in range(a.rounds):   # (the first round warms the page cache and the driver: not counted)
            for name, exe in variants:
                t0 = time.time()
                p = subprocess.run(["timeout", "-k", "10", "120", exe, os.path.basename(cfg)], cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                   env=dict(os.environ, BDX_TIMING="1", BDX_FOREGROUND="1"))
                wall = time.time() - t0
                err = p.stderr.decode()
                if p.returncode != 0:
                    print(name, "FAILED", p.returncode, err[-2000:], flush=True)
                    sys.exit(1)
                m = re.search(r"decode\+merge\+stream=([0-9.]+)s.*format=([0-9.]+)s total=([0-9.]+)s", err)
                tables[name].add("\n".join(l for l in p.stdout.decode().splitlines() if not l.startswith(("#Command", "#Software"))))
                if rep:
                    for k, v in zip(("decode", "format", "total"), m.groups()):
                        res[name][k].append(float(v))
                    res[name]["wall"].append(wall)
        rows = sum(1 for l in next(iter(tables["head"])).splitlines() if not l.startswith("#"))
        leg = {"records": n, "bam_bytes": os.path.getsize(bam), "table_rows": rows, "several_thread_writer": rows >= 8192,
               "tables_equal_byte_for_byte": len(tables["parent"] | tables["head"]) == 1}
        for name in res:
            leg[name] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), all=v) for k, v in res[name].items()}
        leg["head_median_inside_parent_min_max"] = {k: leg["parent"][k]["min"] <= leg["head"][k]["median"] <= leg["parent"][k]["max"] for k in ("decode", "format", "total")}
        summary["legs"]["%g" % fraction] = leg
        print(json.dumps({k: ({q: (v[q]["median"], v[q]["min"], v[q]["max"]) for q in v} if k in res else v) for k, v in leg.items()}), flush=True)
        json.dump(summary, open(a.out, "w"), indent=1)
    finally:
        shutil.rmtree(td, ignore_errors=True)
