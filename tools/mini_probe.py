#!/usr/bin/env python3
"""What --mini's kernel (bdx_window_insert_shift, KW) costs on the benchmark's configs[1] store (synth.make_chromosome: one chromosome of
50 Mbp, 30x, one library), over the CLI's own grid (window = the mean insert size, step = half of it), on both of its routes: the
production routing, and every window through the staged all-pairs route ("mini_staged").

Each call is timed by HIP events on the context's stream around the whole call (window upload, KW, row download) and by the host's clock;
a first call (code object load included) and `--repeat` more, medians over the latter:
  grid   the windows of the CLI's grid over the chromosome
  floor  as many windows of width 0 at the same starts: the upload, the search, one empty step and the download of as many rows -- what
         is left of `grid` is the walk over the records, the ranks and the reads of the null's table
  hist   bdx_insert_size_histogram after the run (KH), which gives the null
Both routes must give the same rows.  Everything twice: on the store as it is (one library) and with its reads dealt out at random to
four libraries of the same cutoffs (the library column is read, four rows per window).
Usage: mini_probe.py [--length 50000000] [--repeat 7] [--out FILE]"""
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
    window = int(np.ceil(LIB_C2["mean_insertsize"]))
    step = max(window // 2, 1)
    starts = np.arange(0, a.length, step, dtype=np.int64)
    grid = np.zeros(len(starts), dtype=_lib.INTERVAL_DTYPE)
    grid["beg"], grid["end"] = starts, np.minimum(starts + window, a.length)
    floor = grid.copy()
    floor["end"] = floor["beg"]
    out = dict(reads=n, window=window, step=step, windows=len(grid), stores={})
    for nlibs in (1, 4):
        if nlibs > 1:
            d["lib"] = rng.integers(0, nlibs, n).astype(np.uint8)
        bd = bda.BreakDancer(Options(), [LibraryConfig(**LIB_C2) for _ in range(nlibs)], 1, ntids=1, max_read_window_size=200, device=0)
        bd.lib.bdx_reserve(bd.h, n)
        bd.push_reads(d)
        bd.run()
        stream = torch.cuda.ExternalStream(bd.lib.bdx_stream(bd.h))
        hist_calls = [timed(stream, bd.insert_size_histogram) for _ in range(1 + a.repeat)]
        hist = hist_calls[-1][0][0]
        bd.set_insert_null(hist)
        rec = dict(libraries=nlibs, null_pairs=[int(v) for v in hist.sum(axis=1)], hist_ms=float(np.median([x[1] for x in hist_calls[1:]])), sets={})
        rows = {}
        for name, iv in (("floor", floor), ("grid", grid)):
            res = {}
            for route, staged in (("production", 0), ("staged", 1)):
                bd.set_debug("mini_staged", staged)
                calls = []
                for _ in range(1 + a.repeat):
                    r, ev, host = timed(stream, lambda: bd.window_insert_shift(iv))
                    calls.append((ev, host))
                rows[(name, route)] = r
                res[route] = dict(first_event_ms=calls[0][0], median_event_ms=float(np.median([x[0] for x in calls[1:]])),
                                  median_host_ms=float(np.median([x[1] for x in calls[1:]])), min_event_ms=min(x[0] for x in calls[1:]),
                                  max_event_ms=max(x[0] for x in calls[1:]))
            assert rows[(name, "production")].tobytes() == rows[(name, "staged")].tobytes()
            rec["sets"][name] = res
            print(nlibs, name, json.dumps(res), flush=True)
        g = rows[("grid", "production")]
        per = g["n"].sum(axis=1)
        rec.update(observations=int(per.sum()), per_window_mean=float(per.mean()), per_window_max=int(per.max()), over_64=int((per > 64).sum()),
                   saturated=int(g["saturated"].max(axis=1).sum()), row_bytes=int(g.nbytes),
                   kw_ms={r: round(rec["sets"]["grid"][r]["median_event_ms"] - rec["sets"]["floor"][r]["median_event_ms"], 4) for r in ("production", "staged")})
        out["stores"]["%d_librar%s" % (nlibs, "ies" if nlibs > 1 else "y")] = rec
        bd.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "sets"} for k, v in out["stores"].items()}, indent=1))


if __name__ == "__main__":
    main()
