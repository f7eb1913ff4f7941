#!/usr/bin/env python3
"""What --estimate's histogram (bdx_insert_size_histogram, KH) costs against the classifier launch (K1) of the same process, on the
benchmark's configs[1] store (synth.make_chromosome: one chromosome of 50 Mbp, 30x, one library) and, with --share N, on a store of
N records as one GPU of eight holds of a genome (the configs[1] chromosome repeated on further sequences).

Each store twice: as it is (one library: the lib column is not resident, 15 B/read) and with its reads dealt out at random to four
libraries of the same cutoffs (16 B/read, 2048 LDS bins per library).  Per store:
  k1_ms        the classifier's own begin-to-end time by HIP events (bdx_get_timings[0], stage timing on), median of --repeat runs
  call_ms      one bdx_insert_size_histogram call by HIP events on the context's stream: zeroing the table, KH, the table's download;
               a first call (code object load included) and the median of --repeat more
  floor_ms     the same call on a context that holds ONE record: what zeroing and downloading nlibs x 256 KiB cost without the store
  kh_ms        call_ms - floor_ms: KH's own share
KH's bytes per read are its column list's (tid, mtid, isize 4 B each, flag 2 B, mapq 1 B, lib 1 B with several libraries) against the
28 B/read K1 is quoted with (25 read, the class byte and its share of the tables written).
Usage: estimate_probe.py [--length 50000000] [--share 0] [--repeat 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return r, e0.elapsed_time(e1)


def median(v):
    return round(float(np.median(v)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--share", type=int, default=0, help="records of a second store, a GPU's share of a genome (0: none)")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import breakdancer_amd as bda
    from breakdancer_amd.api import LibraryConfig, Options
    from breakdancer_amd.synth import LIB_C2, make_chromosome
    t0 = time.perf_counter()
    base = make_chromosome(length=a.length, seed=1)
    print("synthesised %d records in %.1f s" % (len(base["tid"]), time.perf_counter() - t0), flush=True)
    rng = np.random.default_rng(5)
    stores = [("configs1", base)]
    if a.share:
        reps = -(-a.share // len(base["tid"]))
        d = {k: np.tile(v, reps)[:a.share] for k, v in base.items()}
        d["tid"] = d["mtid"] = (np.arange(a.share) // len(base["tid"])).astype(np.int32)
        stores.append(("genome_share", d))
    out = dict(repeat=a.repeat, k1_bytes_per_read=28, stores={})
    for label, d in stores:
        n = len(d["tid"])
        for nlibs in (1, 4):
            if nlibs > 1:
                d = dict(d, lib=rng.integers(0, nlibs, n).astype(np.uint8))
            libs = [LibraryConfig(**LIB_C2) for _ in range(nlibs)]
            one = bda.BreakDancer(Options(), libs, 1, ntids=1, max_read_window_size=200, device=0)
            one.push_reads({k: v[:1] for k, v in d.items()})
            s1 = torch.cuda.ExternalStream(one.lib.bdx_stream(one.h))
            floor = [timed(s1, one.insert_size_histogram)[1] for _ in range(a.repeat + 1)][1:]
            one.close()
            bd = bda.BreakDancer(Options(), libs, 1, ntids=1, max_read_window_size=200, device=0)
            bd.set_stage_timing(True)
            bd.lib.bdx_reserve(bd.h, n)
            bd.push_reads(d)
            stream = torch.cuda.ExternalStream(bd.lib.bdx_stream(bd.h))
            (hist, over), first = timed(stream, bd.insert_size_histogram)
            calls = [timed(stream, bd.insert_size_histogram)[1] for _ in range(a.repeat)]
            bd.run()   # (the classifier followed the batch as it arrived: this run's K1 covers the tail only and is not timed)
            k1 = []
            for _ in range(a.repeat):
                bd.run()
                k1.append(bd.timings()["classify"])
            again, _ = timed(stream, bd.insert_size_histogram)
            assert np.array_equal(again[0], hist) and np.array_equal(again[1], over)
            bd.close()
            bpr = 15 if nlibs == 1 else 16
            call, fl = median(calls), median(floor)
            kh = round(call - fl, 4)
            rec = dict(reads=n, libraries=nlibs, observations=int(hist.sum()), n_over=int(over.sum()), touched_bins=int((hist > 0).sum()),
                       kh_bytes_per_read=bpr, k1_ms=median(k1), first_call_ms=round(first, 4), call_ms=call, call_min_ms=round(min(calls), 4),
                       call_max_ms=round(max(calls), 4), floor_ms=fl, kh_ms=kh, kh_over_k1=round(kh / median(k1), 3) if median(k1) else None,
                       kh_tb_per_s=round(n * bpr / (kh * 1e-3) / 1e12, 3) if kh > 0 else None,
                       k1_tb_per_s=round(n * 28 / (median(k1) * 1e-3) / 1e12, 3) if median(k1) else None)
            out["stores"]["%s_%d_lib" % (label, nlibs)] = rec
            print(json.dumps(rec), flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
