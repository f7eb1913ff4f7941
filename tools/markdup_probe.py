#!/usr/bin/env python3
"""What --mark-dup costs: the marking kernel (KD, csrc/kd_markdup.hip) on a GPU's share of a genome next to K1 on the same store, and the
whole command with and without the option on one BAM.

(a) One store over a synthetic genome share (synth.make_genome: hg38 lengths x --fraction, 4 libraries, 30x, as tools/site_probe.py) in
    which --dup-share of the pairs are written twice (both mates, a new name; the copies stand next to their originals, so the store stays
    sorted).  The columns live in HBM and are adopted (bdx_set_device_reads), so that with and without the option pass 1 starts from tile 0
    and no PCIe copy is in the timing; every repetition adopts them again -- a new load, KD runs again.  bdx_run is timed by HIP events on
    the context's stream and by the host's clock, enqueue-ahead mode 1 (every run a first run), a first run (code object load included) and
    --repeat more; K1's own time is bdx_get_timings' [0] of the same runs.  on - off = KD's launches, its two host read-backs, and the
    private copy of the flag column that adopted reads get (4 B per read of traffic that a pushed store does not pay).
    With --pileup N the same again on a store that also holds one position with N records (N / 50 groups), which sends that run through
    KD's table, and once more with all N sharing one K (a collapsed repeat: every record meets in one slot).
(b) With --cli-fraction F: one library, hg38 lengths x F as ONE BAM (tmpfs when there is one), `breakdancer-max cfg` against
    `breakdancer-max --mark-dup cfg`, one process from start to exit (BDX_FOREGROUND=1), best of 3, page cache warm: what pass 1 not running
    behind the decode costs end to end, together with KD itself.
Usage: markdup_probe.py [--fraction 0.125] [--dup-share 0.1] [--repeat 5] [--pileup 100000] [--cli-fraction 0.015625] [--out FILE]"""
import argparse
import json
import os
import shutil
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
CFG_LINE = "readgroup:rg1\tplatform:illumina\tmap:%s\treadlen:100.00\tlib:lib1\tlower:310.00\tupper:490.00\tmean:400.00\tstd:30.00\n"


def plant_copies(d, share):
    """`share` of the pairs written twice: both mates (they share the name key the choice is made by), the copy right behind its original
    under a new name key"""
    n = len(d["tid"])
    h = (d["name_key"] * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    reps = np.where(h < np.uint64(int(share * (1 << 24))), 2, 1)
    idx = np.repeat(np.arange(n), reps)
    out = {k: v[idx] for k, v in d.items()}
    copy = np.zeros(len(idx), bool)
    copy[1:] = idx[1:] == idx[:-1]
    out["name_key"] = np.where(copy, out["name_key"] ^ np.uint64(0x5555555555555555), out["name_key"])
    return out, int(copy.sum())


def with_pileup(d, n_pile, rng, groups=None):
    """one position (the store's middle record's) with n_pile more records: candidates with `groups` different mate positions
    (default n_pile / 50; 1: a collapsed repeat whose records all share one K and meet in one slot of KD's table)"""
    at = len(d["tid"]) // 2
    while at + 1 < len(d["tid"]) and d["pos"][at + 1] == d["pos"][at] and d["tid"][at + 1] == d["tid"][at]:
        at += 1
    pile = {k: np.repeat(v[at:at + 1], n_pile) for k, v in d.items()}
    pile["flag"] = np.full(n_pile, 0x1 | 0x20 | 0x40, np.uint16)
    pile["mtid"] = pile["tid"].copy()
    pile["mpos"] = (pile["pos"] + 200 + rng.integers(0, groups or max(1, n_pile // 50), n_pile)).astype(np.int32)
    pile["isize"] = (pile["mpos"] - pile["pos"] + 100).astype(np.int32)
    pile["name_key"] = rng.integers(1, 1 << 62, n_pile).astype(np.uint64)
    return {k: np.concatenate([v[:at + 1], pile[k], v[at + 1:]]) for k, v in d.items()}


def to_device(d):
    import torch
    from breakdancer_amd.api import BATCH_FIELDS
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint64): np.int64}
    keep, ptrs = [], {}
    for k, dt in BATCH_FIELDS:
        a = np.ascontiguousarray(d[k], dtype=dt)
        t = torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()
        keep.append(t)
        ptrs[k] = t.data_ptr()
    torch.cuda.synchronize()
    return keep, ptrs


def time_runs(d, libs, ntids, mark, repeat):
    import torch
    import breakdancer_amd as bda
    from breakdancer_amd.api import Options
    n = len(d["tid"])
    keep, ptrs = to_device(d)
    bd = bda.BreakDancer(Options(), libs, 1, ntids=ntids, max_read_window_size=200, device=0)
    if mark:
        bd.mark_duplicates()
    bd.set_enqueue_ahead(1)
    stream = torch.cuda.ExternalStream(bd.lib.bdx_stream(bd.h))
    runs = []
    for i in range(1 + repeat):
        bd.set_device_reads(ptrs, n)   # a new load
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        h0 = time.perf_counter()
        bd.run()
        h1 = time.perf_counter()
        e1.record(stream)
        e1.synchronize()
        runs.append(dict(run=i, event_ms=round(e0.elapsed_time(e1), 4), host_ms=round(1e3 * (h1 - h0), 4), k1_ms=round(bd.timings()["classify"], 4)))
        print("mark_dup=%d" % mark, runs[-1], flush=True)
    marked, groups = bd.duplicates()
    s = bd.summary()
    later = runs[1:] or runs
    out = dict(mark_dup=bool(mark), reads=n, runs=runs, median_event_ms=float(np.median([r["event_ms"] for r in later])),
               median_host_ms=float(np.median([r["host_ms"] for r in later])), median_k1_ms=float(np.median([r["k1_ms"] for r in later])),
               marked=marked, groups=groups, n_anomalous=int(s["n_anomalous"]), n_svs_printed=int(s["n_svs_printed"]))
    bd.close()
    del keep
    torch.cuda.empty_cache()
    return out


def kernel_probe(fraction, dup_share, repeat, pileup):
    from breakdancer_amd.api import LibraryConfig
    from breakdancer_amd.synth import make_genome
    lengths = [int(m * 1e6 * fraction) for m in HG38_MBP]
    libs = [LibraryConfig(mean_insertsize=m, std_insertsize=sd, uppercutoff=m + 3 * sd, lowercutoff=m - 3 * sd, readlens=100.0, name="lib%d" % i)
            for i, (m, sd) in enumerate(LIBS4)]
    t0 = time.perf_counter()
    d = make_genome(lengths, coverage=30.0, seed=11, libs=LIBS4, lib_bam=(0, 0, 0, 0), n_translocations=int(5000 * fraction * 8))
    d, copies = plant_copies(d, dup_share)
    print("synthesised %d records (%d of them planted copies) in %.1f s" % (len(d["tid"]), copies, time.perf_counter() - t0), flush=True)
    out = dict(fraction=fraction, dup_share=dup_share, planted_copies=copies, off=time_runs(d, libs, len(lengths), False, repeat),
               on=time_runs(d, libs, len(lengths), True, repeat))
    out["on_minus_off_event_ms"] = out["on"]["median_event_ms"] - out["off"]["median_event_ms"]
    if pileup:
        p = with_pileup(d, pileup, np.random.default_rng(5))
        out["pileup"] = dict(records_at_one_position=pileup, on=time_runs(p, libs, len(lengths), True, repeat))
        out["pileup"]["on_minus_plain_on_event_ms"] = out["pileup"]["on"]["median_event_ms"] - out["on"]["median_event_ms"]
        p = with_pileup(d, pileup, np.random.default_rng(5), groups=1)
        out["pileup_one_k"] = dict(records_at_one_position=pileup, on=time_runs(p, libs, len(lengths), True, repeat))
        out["pileup_one_k"]["on_minus_plain_on_event_ms"] = out["pileup_one_k"]["on"]["median_event_ms"] - out["on"]["median_event_ms"]
    return out


def cli_probe(fraction, dup_share):
    from breakdancer_amd.bamwrite import write_bam
    from breakdancer_amd.synth import make_genome
    lengths = [int(m * 1e6 * fraction) for m in HG38_MBP]
    d, copies = plant_copies(make_genome(lengths, coverage=30.0, seed=12, n_translocations=int(5000 * fraction * 8)), dup_share)
    td = tempfile.mkdtemp(prefix="bdx_markdup_probe", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        bam = os.path.join(td, "genome.bam")
        t0 = time.perf_counter()
        write_bam(bam, d, ["chr%d" % (i + 1) for i in range(len(lengths))])
        print("wrote %d records, %.2f GB of BAM in %.1f s" % (len(d["tid"]), os.path.getsize(bam) / 1e9, time.perf_counter() - t0), flush=True)
        open(os.path.join(td, "cfg"), "w").write(CFG_LINE % "genome.bam")
        res = dict(fraction=fraction, records=len(d["tid"]), planted_copies=copies, bam_bytes=os.path.getsize(bam))
        for label, args in (("without", []), ("with_mark_dup", ["--mark-dup"]), ("without_again", [])):
            best = None
            for _ in range(3):
                time.sleep(0.5)
                t0 = time.perf_counter()
                p = subprocess.run([os.path.join(ROOT, "bin", "breakdancer-max")] + args + ["cfg"], cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                   env=dict(os.environ, BDX_TIMING="1", BDX_FOREGROUND="1"))
                dt = time.perf_counter() - t0
                if p.returncode != 0:
                    raise RuntimeError(p.stderr.decode()[-400:])
                rows = sum(1 for l in p.stdout.splitlines() if l and not l.startswith(b"#"))
                tl = [x for x in p.stderr.decode().splitlines() if x.startswith("[bdx timing]") and ("reads=" in x or "inside bdx_run" in x or "--mark-dup" in x)]
                if best is None or dt < best[0]:
                    best = (dt, rows, tl)
            res[label] = dict(seconds=round(best[0], 4), sv_rows=best[1], cli_breakdown=best[2])
            print(label, res[label], flush=True)
        res["mark_dup_costs_seconds"] = round(res["with_mark_dup"]["seconds"] - min(res["without"]["seconds"], res["without_again"]["seconds"]), 4)
        return res
    finally:
        shutil.rmtree(td, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fraction", type=float, default=0.125)
    ap.add_argument("--dup-share", type=float, default=0.1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--pileup", type=int, default=100000)
    ap.add_argument("--cli-fraction", type=float, default=1.0 / 64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    if a.fraction > 0:
        out["kernel"] = kernel_probe(a.fraction, a.dup_share, a.repeat, a.pileup)
        save()
    if a.cli_fraction > 0:
        out["cli"] = cli_probe(a.cli_fraction, a.dup_share)
        save()
    strip = lambda v: {k: (strip(x) if isinstance(x, dict) else x) for k, x in v.items() if k != "runs"}
    print(json.dumps(strip(out), indent=1))


if __name__ == "__main__":
    main()
