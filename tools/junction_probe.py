#!/usr/bin/env python3
"""What --vcf's junction count (bdx_count_junction_pairs, K8) costs at a GPU's share of a genome.

(a) One context over a synthetic genome share (synth.make_genome: hg38 lengths x fraction, 4 libraries, 30x, as the full-size tests use
    it): the junctions of that run's printed calls, queried the way the CLI does (one query per same-chromosome call over both junctions,
    two per CTX call), timed by HIP events on the context's stream around the whole call (query upload, kernel, count download) and by the
    host's clock; a first call (code object load included) and `--repeat` more.
(b) With --bam-fraction F: the CLI's wall time on an indexed genome BAM of that share (bamwrite.write_genome_bam), with and without --vcf,
    BDX_TIMING=1 (its "--vcf: junction counts" line is the host's view of the count inside the process).
Usage: junction_probe.py [--fraction 0.125] [--repeat 5] [--bam-fraction 0.015625] [--out FILE]  (--out: the whole record as JSON; the
summary goes to stdout either way)"""
import argparse
import json
import os
import re
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


def queries(svs):
    p = svs[svs["printed"] == 1]
    same = p["chr"][:, 0] == p["chr"][:, 1]
    s, c = p[same], p[~same]
    tid = np.concatenate([s["chr"][:, 0], c["chr"][:, 0], c["chr"][:, 1]])
    pa = np.concatenate([s["pos"].min(axis=1), c["pos"][:, 0], c["pos"][:, 1]])
    pb = np.concatenate([s["pos"].max(axis=1), c["pos"][:, 0], c["pos"][:, 1]])
    return len(p), tid.astype(np.int32), pa.astype(np.int32), pb.astype(np.int32)


def kernel_probe(fraction, repeat):
    import torch
    import breakdancer_amd as bda
    from breakdancer_amd.api import LibraryConfig, Options
    from breakdancer_amd.synth import make_genome
    lengths = [int(m * 1e6 * fraction) for m in HG38_MBP]
    libs = [LibraryConfig(mean_insertsize=m, std_insertsize=sd, uppercutoff=m + 3 * sd, lowercutoff=m - 3 * sd, readlens=100.0, name="lib%d" % i)
            for i, (m, sd) in enumerate(LIBS4)]
    t0 = time.perf_counter()
    d = make_genome(lengths, coverage=30.0, seed=11, libs=LIBS4, lib_bam=(0, 0, 0, 0), n_translocations=int(5000 * fraction * 8))
    n = len(d["tid"])
    print("synthesised %d records in %.1f s" % (n, time.perf_counter() - t0), flush=True)
    bd = bda.BreakDancer(Options(), libs, 1, ntids=len(lengths), max_read_window_size=200, device=0)
    bd.lib.bdx_reserve(bd.h, n)
    bd.push_reads(d)
    bd.run()
    svs, _, _ = bd.svs()
    rows, tid, pa, pb = queries(svs)
    stream = torch.cuda.ExternalStream(bd.lib.bdx_stream(bd.h))
    calls = []
    ref = None
    for i in range(1 + repeat):
        for by_library in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            h0 = time.perf_counter()
            c = bd.count_junction_pairs(tid, pa, pb, by_library=by_library)
            h1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            calls.append(dict(call=i, by_library=by_library, event_ms=round(e0.elapsed_time(e1), 4), host_ms=round(1e3 * (h1 - h0), 4)))
            if not by_library:
                ref = c if ref is None else ref
                assert (c == ref).all()
            print(calls[-1], flush=True)
    later = [x for x in calls if x["call"] > 0]
    out = dict(fraction=fraction, reads=n, printed_rows=rows, queries=len(tid), keys_by_file=1, keys_by_library=len(libs),
               pairs_counted_mean=float(ref.sum(axis=1).mean()), calls=calls,
               median_event_ms={k: float(np.median([x["event_ms"] for x in later if x["by_library"] == b])) for k, b in (("by_file", False), ("by_library", True))},
               median_host_ms={k: float(np.median([x["host_ms"] for x in later if x["by_library"] == b])) for k, b in (("by_file", False), ("by_library", True))})
    bd.close()
    return out


def cli_probe(fraction, runs=2):
    from breakdancer_amd.bamwrite import write_genome_bam
    td = os.environ.get("BDX_PROBE_DIR", os.path.join(tempfile.gettempdir(), "bdx_junction_probe"))
    bam, cfg, n = write_genome_bam(td, fraction, tag="genome")
    res = dict(fraction=fraction, records=n, runs=[])
    for r in range(runs):
        for vcf in (False, True):
            args = [os.path.join(ROOT, "bin", "breakdancer-max")] + (["--vcf", os.path.join(td, "out.vcf")] if vcf else []) + [cfg]
            time.sleep(2.0)   # (untimed: the driver is still taking back the previous process's memory)
            t0 = time.perf_counter()
            p = subprocess.run(args, cwd=td, env=dict(os.environ, BDX_TIMING="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            dt = time.perf_counter() - t0
            err = p.stderr.decode()
            m = re.search(r"--vcf: junction counts of (\d+) rows ([0-9.]+) s", err)
            tot = re.search(r"total=([0-9.]+)s", err)
            res["runs"].append(dict(run=r, vcf=vcf, rc=p.returncode, wall_s=round(dt, 4), in_process_total_s=float(tot.group(1)) if tot else None,
                                    vcf_count_s=float(m.group(2)) if m else None, rows=int(m.group(1)) if m else None,
                                    table_lines=sum(1 for l in p.stdout.splitlines() if l and not l.startswith(b"#"))))
            print(res["runs"][-1], flush=True)
            if p.returncode:
                print(err[-3000:])
                return res
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fraction", type=float, default=0.125)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--bam-fraction", type=float, default=0.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"kernel": kernel_probe(a.fraction, a.repeat)}
    if a.bam_fraction > 0:
        out["cli"] = cli_probe(a.bam_fraction)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("calls", "runs")} for k, v in out.items()}, indent=1))


if __name__ == "__main__":
    main()
