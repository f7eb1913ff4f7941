#!/usr/bin/env python3
"""What --sites' pair count (bdx_count_site_pairs, KS) costs at a GPU's share of a genome, next to K8 and to --ci's breakpoint bounds
(bdx_site_breakpoint_bounds, KI) at the same queries, and how far its record-only rule stands from the walk's own count.

(a) One context over a synthetic genome share (synth.make_genome: hg38 lengths x fraction, 4 libraries, 30x, as tools/junction_probe.py):
    --sites N sites (default 10,000) made from that run's printed calls -- each call's two ends and type, cycled with its ends moved by up
    to a window when there are fewer calls than sites -- counted with the window the CLI would choose (the largest library uppercutoff),
    timed by HIP events on the context's stream around the whole call (site upload, kernel, count download) and by the host's clock; a
    first call (code object load included) and `--repeat` more.  bdx_count_junction_pairs (K8) is timed the same way on the same sites:
    one query per site, over both junctions of a same-chromosome site and over the first of a CTX site.  bdx_site_breakpoint_bounds (KI)
    likewise, on the same sites with the same window, beside each of the two (it has no key choice: it reads the library column whenever the
    context has more than one library); its n must equal KS's row sums.
(b) With --recall: the CLI on the chr21 golden fixture, its own table fed back as --sites; per printed call, the site's DV summed over
    the samples against the call's num_Reads.
Usage: site_probe.py [--fraction 0.125] [--sites 10000] [--repeat 5] [--recall] [--out FILE]  (--out: the whole record as JSON; the summary
goes to stdout either way)"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HG38_MBP = [248.96, 242.19, 198.30, 190.21, 181.54, 170.81, 159.35, 145.14, 138.39, 133.80, 135.09, 133.28, 114.36, 107.04,
            101.99, 90.34, 83.26, 80.37, 58.62, 64.44, 46.71, 50.82, 156.04, 57.23]
LIBS4 = ((400.0, 30.0), (350.0, 40.0), (500.0, 50.0), (300.0, 25.0))
TYPE_MASK = {1: (1 << 1) | (1 << 5), 2: 1 << 2, 3: 1 << 3, 4: 1 << 4, 5: (1 << 1) | (1 << 5), 8: 1 << 8}   # a call's flag -> its type's mask (no -l)


def make_sites(svs, n_sites, window, rng):
    from breakdancer_amd import _lib
    p = svs[(svs["printed"] == 1) & (svs["pos"].min(axis=1) >= 1) & np.isin(svs["flag"], list(TYPE_MASK))]
    idx = np.arange(n_sites) % len(p)
    jitter = np.where(np.arange(n_sites) < len(p), 0, 1)[:, None] * rng.integers(-window, window + 1, (n_sites, 2))
    chr_, pos = p["chr"][idx].astype(np.int64), np.maximum(p["pos"][idx].astype(np.int64) + jitter, 1)
    swap = (chr_[:, 0] > chr_[:, 1]) | ((chr_[:, 0] == chr_[:, 1]) & (pos[:, 0] > pos[:, 1]))
    a, b = np.where(swap, 1, 0), np.where(swap, 0, 1)
    r = np.arange(n_sites)
    s = np.zeros(n_sites, dtype=_lib.SITE_DTYPE)
    s["tid1"], s["pos1"], s["tid2"], s["pos2"] = chr_[r, a], pos[r, a], chr_[r, b], pos[r, b]
    s["flag_mask"] = [TYPE_MASK[int(f)] for f in p["flag"][idx]]
    return len(p), s


def timed(bd, stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    h0 = time.perf_counter()
    c = fn()
    h1 = time.perf_counter()
    e1.record(stream)
    e1.synchronize()
    return c, round(e0.elapsed_time(e1), 4), round(1e3 * (h1 - h0), 4)


def kernel_probe(fraction, n_sites, repeat):
    import torch
    import breakdancer_amd as bda
    from breakdancer_amd.api import LibraryConfig, Options
    from breakdancer_amd.synth import make_genome
    lengths = [int(m * 1e6 * fraction) for m in HG38_MBP]
    libs = [LibraryConfig(mean_insertsize=m, std_insertsize=sd, uppercutoff=m + 3 * sd, lowercutoff=m - 3 * sd, readlens=100.0, name="lib%d" % i)
            for i, (m, sd) in enumerate(LIBS4)]
    window = int(max(math.ceil(m + 3 * sd) for m, sd in LIBS4))
    t0 = time.perf_counter()
    d = make_genome(lengths, coverage=30.0, seed=11, libs=LIBS4, lib_bam=(0, 0, 0, 0), n_translocations=int(5000 * fraction * 8))
    n = len(d["tid"])
    print("synthesised %d records in %.1f s" % (n, time.perf_counter() - t0), flush=True)
    bd = bda.BreakDancer(Options(), libs, 1, ntids=len(lengths), max_read_window_size=200, device=0)
    bd.lib.bdx_reserve(bd.h, n)
    bd.push_reads(d)
    bd.run()
    svs, _, _ = bd.svs()
    rows, sites = make_sites(svs, n_sites, window, np.random.default_rng(3))
    same = sites["tid1"] == sites["tid2"]
    j_tid, j_a, j_b = sites["tid1"], sites["pos1"], np.where(same, sites["pos2"], sites["pos1"])
    stream = torch.cuda.ExternalStream(bd.lib.bdx_stream(bd.h))
    calls = []
    ref = None
    for i in range(1 + repeat):
        for by_library in (False, True):
            c, ev, host = timed(bd, stream, lambda: bd.count_site_pairs(sites, window, by_library=by_library))
            _, ev8, host8 = timed(bd, stream, lambda: bd.count_junction_pairs(j_tid, j_a, j_b, by_library=by_library))
            b, evi, hosti = timed(bd, stream, lambda: bd.site_breakpoint_bounds(sites, window))
            calls.append(dict(call=i, by_library=by_library, sites_event_ms=ev, sites_host_ms=host, k8_event_ms=ev8, k8_host_ms=host8,
                              bounds_event_ms=evi, bounds_host_ms=hosti))
            assert (b["n"] == c.sum(axis=1)).all()
            if not by_library:
                ref = c if ref is None else ref
                assert (c == ref).all()
            else:
                assert (c.sum(axis=1) == ref[:, 0]).all()
            print(calls[-1], flush=True)
    later = [x for x in calls if x["call"] > 0]
    med = lambda key: {k: float(np.median([x[key] for x in later if x["by_library"] == b])) for k, b in (("by_file", False), ("by_library", True))}
    out = dict(fraction=fraction, reads=n, printed_rows=rows, sites=int(n_sites), window=window, same_chromosome_sites=int(same.sum()),
               keys_by_file=1, keys_by_library=len(libs), pairs_counted_mean=float(ref.sum(axis=1).mean()), sites_with_pairs=float((ref.sum(axis=1) > 0).mean()),
               calls=calls, median_sites_event_ms=med("sites_event_ms"), median_sites_host_ms=med("sites_host_ms"),
               median_k8_event_ms=med("k8_event_ms"), median_k8_host_ms=med("k8_host_ms"),
               median_bounds_event_ms=med("bounds_event_ms"), median_bounds_host_ms=med("bounds_host_ms"))
    # (KI's call is the same whichever KS call it stands next to: both medians are over the same kind of call)
    out["bounds_over_sites_event"] = {k: round(out["median_bounds_event_ms"][k] / out["median_sites_event_ms"][k], 3) for k in ("by_file", "by_library")}
    out["sites_contradictory"] = float(((b["n"] > 0) & ((b["lo1"] > b["hi1"]) | (b["lo2"] > b["hi2"]))).mean())
    bd.close()
    return out


def recall_probe():
    cwd = os.path.join(ROOT, "tests", "golden", "chr21")
    exe = os.path.join(ROOT, "bin", "breakdancer-max")
    td = tempfile.mkdtemp(prefix="bdx_site_probe")
    res = {}
    for label, args in (("default", []), ("every_call", ["-y", "-1", "-r", "1"])):
        table = subprocess.run([exe] + args + ["inv_del_bam_config"], cwd=cwd, stdout=subprocess.PIPE, check=True).stdout.decode()
        rows = [l.split("\t") for l in table.split("\n") if l and not l.startswith("#")]
        keep = [r for r in rows if (r[6] == "CTX") == (r[0] != r[3])]
        tf, out = os.path.join(td, label + ".txt"), os.path.join(td, label + ".vcf")
        open(tf, "w").write("".join("\t".join(r) + "\n" for r in keep))
        subprocess.run([exe, "--sites", tf, "--sites-vcf", out] + args + ["inv_del_bam_config"], cwd=cwd, stdout=subprocess.PIPE, check=True)
        recs = {l.split("\t")[2]: l.split("\t") for l in open(out).read().split("\n") if l and not l.startswith("#")}
        diff, by_type = [], {}
        for k, r in enumerate(keep):
            dv = sum(int(f.split(":")[4]) for f in recs["SITE%d" % (k + 1)][9:])
            diff.append(dv - int(r[9]))
            t = by_type.setdefault(r[6], [0, 0])
            t[0] += 1
            t[1] += dv >= int(r[9])
        d = np.array(diff)
        res[label] = dict(args=args, calls=len(rows), sites=len(keep), window=[l for l in open(out).read().split("\n") if l.startswith("##sites_window=")][0].split("=")[1],
                          dv_reaches_num_reads=float((d >= 0).mean()) if len(d) else None, dv_equals_num_reads=float((d == 0).mean()) if len(d) else None,
                          by_type={t: dict(sites=v[0], dv_reaches_num_reads=v[1]) for t, v in by_type.items()},
                          difference_quantiles=dict(zip(("min", "p10", "p25", "median", "p75", "p90", "max"),
                                                        [float(x) for x in np.quantile(d, [0, 0.1, 0.25, 0.5, 0.75, 0.9, 1])])) if len(d) else None,
                          differences=[int(x) for x in d])
        print(label, {k: v for k, v in res[label].items() if k != "differences"}, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fraction", type=float, default=0.125)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--recall", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {}
    if a.recall:
        out["recall"] = recall_probe()
    if a.fraction > 0:
        out["kernel"] = kernel_probe(a.fraction, a.sites, a.repeat)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("calls",)} for k, v in out.items()}, indent=1))


if __name__ == "__main__":
    main()
