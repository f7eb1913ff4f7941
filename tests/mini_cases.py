"""--mini restated in numpy and Python, for tests/test_mini.py (CPU) and tests/test_gpu_mini.py: the rule of bdx_window_insert_shift
(include/bdx.h), the score of a row (csrc/bdx_mini.h) and the CLI's window call, threshold, merge and table (host/mini.h).

The restatement is brute force and shares nothing with the kernel: per window one mask over all records, np.sort, a count per distinct
value by comparison, Python integers for the products.  No search, no routes.

  OBSERVATION  record i is an observation x = |isize| of its library for (tid, [beg, end)) when tid[i] == tid, beg <= pos[i] < end,
               cls & 0x10, cls & 15 in {NORMAL_FR 6, NORMAL_RF 7, ARP_LARGE_INSERT 2, ARP_SMALL_INSERT 3}, mtid == tid, and pos < mpos or
               (pos == mpos and flag & 0x40).  A library index out of range is library 0.  x >= ISIZE_BINS counts only in n_over.
  ROW          n, n_over, saturated, pad = 0, sum, t_plus = max(0, max_i(#{x_j <= x_i} N - C(x_i) n)),
               t_minus = max(0, max_i(C(x_i - 1) n - #{x_j < x_i} N)), C the null's cumulative counts, N its total, C(-1) = 0.
  CAP          more than MINI_CAP observations in a window, all libraries together: saturated = 1 and both t's 0 in every row."""
import math

import numpy as np

ISIZE_BINS = 32768
MINI_CAP = 4096
MINI_CLASSES = (6, 7, 2, 3)
USABLE = 1000


def qualifies(soa, cls, nlibs):
    """(the records that are observations of the windows they start in, their x, their library)"""
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    mt, ms = soa["mtid"].astype(np.int64), soa["mpos"].astype(np.int64)
    first = (soa["flag"].astype(np.int64) & 0x40) != 0
    ok = ((cls & 0x10) != 0) & np.isin(cls & 15, MINI_CLASSES) & (mt == t) & ((s < ms) | ((s == ms) & first))
    x = np.abs(soa["isize"].astype(np.int64))
    lib = soa["lib"].astype(np.int64) if nlibs > 1 else np.zeros(len(t), np.int64)
    lib = np.where((lib >= 0) & (lib < nlibs), lib, 0)
    return ok, x, lib


def row_of(xs, n_over, crow, saturated=False):
    """one library's row from its observations below ISIZE_BINS (any order) and the null's cumulative row"""
    xs = np.sort(np.asarray(xs, dtype=np.int64))
    n, N = len(xs), int(crow[-1])
    tp = tm = 0
    if not saturated:
        for v in sorted(set(xs.tolist())):
            le, lt = int((xs <= v).sum()), int((xs < v).sum())
            tp = max(tp, le * N - int(crow[v]) * n)
            tm = max(tm, (int(crow[v - 1]) if v else 0) * n - lt * N)
    return (n, int(n_over), int(bool(saturated)), 0, int(xs.sum()), tp, tm)


def expected_rows(soa, cls, nlibs, intervals, hist):
    """[len(intervals)][nlibs] rows as tuples (n, n_over, saturated, pad, sum, t_plus, t_minus)"""
    ok, x, lib = qualifies(soa, cls, nlibs)
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    cum = np.cumsum(np.asarray(hist, dtype=np.uint64).reshape(nlibs, ISIZE_BINS), axis=1)
    out = []
    for tid, beg, end in intervals:
        m = ok & (t == tid) & (s >= beg) & (s < end)
        inside = m & (x < ISIZE_BINS)
        sat = int(inside.sum()) > MINI_CAP
        out.append([row_of(x[inside & (lib == L)], int((m & ~inside & (lib == L)).sum()), cum[L], sat) for L in range(nlibs)])
    return out


def rows_array(rows, dtype):
    a = np.zeros((len(rows), len(rows[0]) if rows else 0), dtype=dtype)
    for i, r in enumerate(rows):
        for j, v in enumerate(r):
            a[i, j] = v
    return a


# ---------------------------------------------------------------------------------------------------------------------------------
# SCORE
# ---------------------------------------------------------------------------------------------------------------------------------
def lam_of(n, D):
    return (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * D


def score(row, N):
    """(score, D) of a row (n, n_over, saturated, pad, sum, t_plus, t_minus) against a null of N"""
    n, sat, tp, tm = row[0], row[2], row[5], row[6]
    if n == 0 or N == 0 or sat:
        return 0.0, 0.0
    D = float(max(tp, tm)) / (float(n) * float(N))
    lam = lam_of(n, D)
    if lam < 0.4:
        return 0.0, D
    S, j = 0.0, 1
    while True:
        term = math.exp(-2.0 * (j * j - 1.0) * lam * lam)
        S += term if j % 2 else -term
        if term < 1e-17:
            break
        j += 1
    lnp = math.log(2.0) - 2.0 * lam * lam + math.log(S)
    return -10.0 * lnp / math.log(10.0), D


# ---------------------------------------------------------------------------------------------------------------------------------
# the CLI's call: window, threshold, merge, table
# ---------------------------------------------------------------------------------------------------------------------------------
def null_figures(hist):
    """(N, mu, usable) per library of hist[nlibs][ISIZE_BINS]; mu in double, bins ascending, count * x"""
    N, mu = [], []
    for h in np.asarray(hist, dtype=np.uint64):
        tot, cnt = 0.0, 0
        for xv in np.nonzero(h)[0]:
            tot += float(int(h[xv])) * float(int(xv))
            cnt += int(h[xv])
        N.append(cnt)
        mu.append(tot / float(cnt) if cnt else 0.0)
    return N, mu, [n >= USABLE for n in N]


def window_call(rows, N, mu, min_pairs):
    """None for a window without a scoring row, else dict(score, shift, D, pairs, type)"""
    total, moved, pairs, best, bestD = 0.0, 0.0, 0, -1.0, 0.0
    hit = False
    for L, r in enumerate(rows):
        if N[L] < USABLE or r[2] or r[0] < min_pairs:
            continue
        sc, D = score(r, N[L])
        hit = True
        total += sc
        pairs += r[0]
        moved += float(r[4]) - float(r[0]) * mu[L]
        if sc > best:
            best, bestD = sc, D
    if not hit:
        return None
    shift = moved / float(pairs)
    return dict(score=total, shift=shift, D=bestD, pairs=pairs, type="DEL" if shift > 0 else "INS")


def default_threshold(W):
    """20 + ceil(10 log10 W), in integers: the smallest k with 10^k >= W^10"""
    k = 0
    while 10 ** k < max(W, 1) ** 10:
        k += 1
    return 20 + k


def grid(length, step):
    return (length - 1) // step + 1 if length else 0


def merge(calls, threshold, window, step, lengths):
    """calls: {(seq, j): window_call}; returns rows (seq, beg, end, type, shift, score, pairs, D, windows)"""
    out, prev = [], None
    for (seq, j) in sorted(calls):
        c = calls[(seq, j)]
        if c is None or not c["score"] >= threshold:
            continue
        end = min(j * step + window, lengths[seq])
        if prev is not None and prev[0] == seq and prev[1] + 1 == j and prev[2] == c["type"]:
            r = out[-1]
            r[2] = end
            r[8] += 1
            if c["score"] > r[5]:
                r[4], r[5], r[6], r[7] = c["shift"], c["score"], c["pairs"], c["D"]
        else:
            out.append([seq, j * step + 1, end, c["type"], c["shift"], c["score"], c["pairs"], c["D"], 1])
        prev = (seq, j, c["type"])
    return out


def table_text(rows, names):
    lines = ["#Chr\tBeg\tEnd\tType\tShift\tScore\tPairs\tD\tWindows"]
    for seq, beg, end, typ, shift, sc, pairs, D, nw in rows:
        lines.append("%s\t%d\t%d\t%s\t%.1f\t%d\t%d\t%.3f\t%d" % (names[seq], beg, end, typ, shift, min(int(math.floor(sc + 0.5)), 99999), pairs, D, nw))
    return "".join(l + "\n" for l in lines)


def rows_text(rows_by_window):
    """the ROWS file of bdx-mini-check: {window index: [row per library]}, all-zero rows left out"""
    out = []
    for w in sorted(rows_by_window):
        for L, r in enumerate(rows_by_window[w]):
            if any(r):
                out.append("%d %d %d %d %d %d %d %d" % (w, L, r[0], r[1], r[2], r[4], r[5], r[6]))
    return "".join(l + "\n" for l in out)
