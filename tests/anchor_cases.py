"""--anchor restated in numpy and plain Python: the rule of bdx_window_anchor_split (include/bdx.h) by brute force over positions --
A(S) and B(S) are counted afresh for every S that is tried, nothing is accumulated along the store --, and the host half (anchor.h):
the default window and step, a window's call, the merge and the table.  Shared by tests/test_anchor.py and tests/test_gpu_anchor.py."""
import math

import numpy as np

MATE_UNMAPPED = 9
FIELDS = ("n_fwd", "n_rev", "n_low", "n_left", "n_right", "u_left", "u_right", "split", "last_left", "first_right")
SCAN_ALL_BELOW = 3000       # windows this narrow are also scanned at EVERY S of [beg, end]
HEADER = "#Chr\tPos1\tPos2\tType\tLeft\tRight\tDistinctLeft\tDistinctRight\tLowQual\tWindows\n"


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def record_kinds(soa, cls, minima, min_qual=-1, long_insert=False):
    """(points right, points left, low) per record of the store: cls the whole class byte, minima the libraries' resolved minima"""
    cls = np.asarray(cls).astype(np.int64)
    flag, qual, lib = soa["flag"].astype(np.int64), soa["bdqual"].astype(np.int64), soa["lib"].astype(np.int64)
    minima = np.asarray(minima, np.int64)
    cand = cls == MATE_UNMAPPED
    if min_qual < 0:
        ok = qual > minima[np.where((lib >= 0) & (lib < len(minima)), lib, 0)]
    else:
        ok = qual >= min_qual
    rev = ((flag & 0x10) != 0) != bool(long_insert)
    return cand & ok & ~rev, cand & ok & rev, cand & ~ok


def split_row(R, L, n_low, beg, end):
    """one row from the positions of the window's right-pointing (R) and left-pointing (L) anchors"""
    R, L = np.sort(np.asarray(R, np.int64)), np.sort(np.asarray(L, np.int64))
    row = dict(n_fwd=len(R), n_rev=len(L), n_low=int(n_low), n_left=0, n_right=0, u_left=0, u_right=0, split=int(beg), last_left=-1, first_right=-1)
    if end <= beg:
        return dict(row, n_fwd=0, n_rev=0, n_low=0)
    score = lambda S: (R[None, :] < S[:, None]).sum(axis=1) + (L[None, :] >= S[:, None]).sum(axis=1)      # A(S) + B(S), counted afresh for every S
    # A + B changes only between p and p + 1 for a position p that holds an anchor: these S, with beg and end, are all that can matter ...
    both = np.concatenate([R, L])
    tries = np.unique(np.concatenate([np.array([beg, end], np.int64), both, both + 1]))
    tries = tries[(tries >= beg) & (tries <= end)]
    at = score(tries)
    best = int(at.max())
    split = int(tries[at == best].min())
    if end - beg <= SCAN_ALL_BELOW:      # ... which a narrow window shows by trying every S there is
        S = np.arange(int(beg), int(end) + 1, dtype=np.int64)
        every = score(S)
        assert int(every.max()) == best and int(S[int(np.argmax(every))]) == split
    left, right = R[R < split], L[L >= split]
    row.update(split=split, n_left=len(left), n_right=len(right), u_left=len(set(left.tolist())), u_right=len(set(right.tolist())),
               last_left=int(left.max()) if len(left) else -1, first_right=int(right.min()) if len(right) else -1)
    return row


def expected_rows(soa, cls, minima, intervals, min_qual=-1, long_insert=False):
    """[row dict] per (tid, beg, end)"""
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    right, left, low = record_kinds(soa, cls, minima, min_qual, long_insert)
    out = []
    for tid, beg, end in intervals:
        m = (t == tid) & (s >= beg) & (s < end)
        out.append(split_row(s[m & right], s[m & left], (m & low).sum(), beg, end))
    return out


def rows_array(rows, dtype):
    a = np.zeros(len(rows), dtype=dtype)
    for i, r in enumerate(rows):
        for k in FIELDS:
            a[i][k] = r[k]
    return a


# ---------------------------------------------------------------------------------------------------------------------------------
# the host half
# ---------------------------------------------------------------------------------------------------------------------------------
def default_window(uppercutoffs):
    """2 x the ceiling of the largest finite cutoff, at most 2^30; None when that gives no window of at least 1"""
    best = 0
    for u in uppercutoffs:
        u = float(np.float32(u))
        if math.isfinite(u):
            best = max(best, 2 * math.ceil(u))
    return min(best, 1 << 30) if best >= 1 else None


def default_step(window):
    return max(window // 2, 1)


def grid(length, step):
    return (length - 1) // step + 1 if length else 0


def calls(row, minimum):
    return row["u_left"] >= minimum and row["u_right"] >= minimum


def merge(called):
    """called: [(seq, row)] in grid order; [(seq, row kept, windows)] in sequence and position order.  Groups are the connected sets of
    the relation "the closed intervals [last_left, first_right] intersect", found pair by pair"""
    n = len(called)
    group = list(range(n))

    def find(i):
        while group[i] != i:
            i = group[i]
        return i

    for i in range(n):
        for j in range(i):
            (sa, a), (sb, b) = called[i], called[j]
            if sa == sb and a["last_left"] <= b["first_right"] and b["last_left"] <= a["first_right"]:
                group[find(i)] = find(j)
    out = []
    for g in sorted({find(i) for i in range(n)}):
        members = sorted((i for i in range(n) if find(i) == g), key=lambda i: (called[i][1]["split"], i))
        rank = lambda i: (called[i][1]["u_left"] + called[i][1]["u_right"], called[i][1]["n_left"] + called[i][1]["n_right"], -called[i][1]["split"])
        top = max(rank(i) for i in members)
        keep = [i for i in members if rank(i) == top][0]
        out.append((called[keep][0], called[keep][1], len(members)))
    return sorted(out, key=lambda c: (c[0], c[1]["split"]))


def table(merged, names):
    return HEADER + "".join("%s\t%d\t%d\tINS\t%d\t%d\t%d\t%d\t%d\t%d\n" % (names[seq], r["last_left"] + 1, r["first_right"] + 1, r["n_left"], r["n_right"], r["u_left"],
                                                                       r["u_right"], r["n_low"], w) for seq, r, w in merged)


def table_of_rows(seq_rows, minimum, names):
    """the file's table from [(seq, row)] in grid order"""
    return table(merge([(s, r) for s, r in seq_rows if calls(r, minimum)]), names)


def rows_text(seq_rows):
    """the rows file of bdx-anchor-check"""
    return "".join("%d %s\n" % (s, " ".join(str(int(r[k])) for k in FIELDS)) for s, r in seq_rows)
