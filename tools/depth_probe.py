#!/usr/bin/env python3
"""What --depth's count (bdx_count_interval_reads, KR) costs on the benchmark's configs[1] store (synth.make_chromosome: one chromosome of
50 Mbp, 30x, one library), on both of its routes: with the per-call chunk table, and with every interval walked ("depth_plain").

Three sets of intervals, each timed by HIP events on the context's stream around the whole call (interval upload, table build, queries,
count download) and by the host's clock; a first call (code object load included) and `--repeat` more, medians over the latter:
  own    the three intervals (inside, two flanks of 1,000) of every printed same-chromosome call of the run itself, as the CLI submits them
  worst  1,000 intervals that each span the whole chromosome
  none   one empty interval: on the table route the build and prefix steps with next to no query, on the walked route the call's fixed cost;
         their difference is what the table costs per call
Both routes must give the same counts.  Everything twice: on the store as it is (one library: one key, the class bytes alone are read) and
with its reads dealt out at random to four libraries of the same cutoffs, counted per library (four keys: the key column and LDS atomics).
Usage: depth_probe.py [--length 50000000] [--repeat 7] [--out FILE]"""
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
    h0 = time.perf_counter()
    c = fn()
    h1 = time.perf_counter()
    e1.record(stream)
    e1.synchronize()
    return c, round(e0.elapsed_time(e1), 4), round(1e3 * (h1 - h0), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--flank", type=int, default=1000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import breakdancer_amd as bda
    from breakdancer_amd import _lib
    from breakdancer_amd.api import LibraryConfig, Options
    from breakdancer_amd.synth import LIB_C2, make_chromosome
    t0 = time.perf_counter()
    d = make_chromosome(length=a.length, seed=1)
    n = len(d["tid"])
    print("synthesised %d records in %.1f s" % (n, time.perf_counter() - t0), flush=True)
    rng = np.random.default_rng(5)
    out = dict(reads=n, chunk=_lib.DEPTH_CHUNK, chunks=-(-n // _lib.DEPTH_CHUNK), stores={})
    for nkeys in (1, 4):                # the store as it is (one library: one key), and its reads dealt out to four libraries of the same cutoffs
        if nkeys > 1:
            d["lib"] = rng.integers(0, nkeys, n).astype(np.uint8)
        bd = bda.BreakDancer(Options(), [LibraryConfig(**LIB_C2) for _ in range(nkeys)], 1, ntids=1, max_read_window_size=200, device=0)
        bd.lib.bdx_reserve(bd.h, n)
        bd.push_reads(d)
        bd.run()
        svs, _, _ = bd.svs()
        p = svs[(svs["printed"] == 1) & (svs["chr"][:, 0] == svs["chr"][:, 1]) & (svs["pos"][:, 0] != svs["pos"][:, 1])]
        lo, hi = p["pos"].min(axis=1).astype(np.int64), p["pos"].max(axis=1).astype(np.int64)
        clamp = lambda x: np.minimum(np.maximum(x, 1), a.length + 1)
        own = np.zeros(3 * len(p), dtype=_lib.INTERVAL_DTYPE)
        own["tid"] = np.repeat(p["chr"][:, 0], 3)
        own["beg"] = np.stack([clamp(lo), clamp(lo - a.flank), clamp(hi)], axis=1).ravel() - 1
        own["end"] = np.stack([clamp(hi), clamp(lo), clamp(hi + a.flank)], axis=1).ravel() - 1
        worst = np.zeros(1000, dtype=_lib.INTERVAL_DTYPE)
        worst["beg"], worst["end"] = np.arange(1000), a.length - np.arange(1000)
        none = np.zeros(1, dtype=_lib.INTERVAL_DTYPE)
        stream = torch.cuda.ExternalStream(bd.lib.bdx_stream(bd.h))
        rec = dict(keys=nkeys, passing=int((bd.read_class() & 0x10 != 0).sum()), printed_same_chromosome_calls=len(p), sets={})
        for name, iv, repeat in (("none", none, a.repeat), ("own", own, a.repeat), ("worst", worst, min(a.repeat, 3))):
            res = {}
            counts = {}
            for route, plain in (("table", 0), ("walked", 1)):
                bd.set_debug("depth_plain", plain)
                calls = []
                for i in range(1 + repeat):
                    c, ev, host = timed(stream, lambda: bd.count_interval_reads(iv, by_library=True))
                    calls.append((ev, host))
                counts[route] = c
                res[route] = dict(first_event_ms=calls[0][0], median_event_ms=float(np.median([x[0] for x in calls[1:]])),
                                  median_host_ms=float(np.median([x[1] for x in calls[1:]])), min_event_ms=min(x[0] for x in calls[1:]),
                                  max_event_ms=max(x[0] for x in calls[1:]))
            assert counts["table"].shape == (len(iv), nkeys) and (counts["table"] == counts["walked"]).all()
            res.update(intervals=len(iv), reads_counted_mean=float(counts["table"].sum(axis=1).mean()),
                       walked_over_table=round(res["walked"]["median_event_ms"] / res["table"]["median_event_ms"], 2))
            rec["sets"][name] = res
            print(nkeys, name, json.dumps(res), flush=True)
        rec["table_build_ms"] = round(rec["sets"]["none"]["table"]["median_event_ms"] - rec["sets"]["none"]["walked"]["median_event_ms"], 4)
        out["stores"]["%d_key%s" % (nkeys, "s" if nkeys > 1 else "")] = rec
        bd.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "sets"} for k, v in out["stores"].items()}, indent=1))


if __name__ == "__main__":
    main()
