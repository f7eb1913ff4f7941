"""Sizes, values and CPU references of tests/test_gpu_prims.py, which holds csrc/bdx_scan.h, csrc/bdx_wave_search.h and
csrc/bdx_window.h to them through tests/prims/prims.hip.  Nothing here needs a GPU: tests/test_prims_cases.py checks the
references against plain loops and the tables against the edges they are there for.

Scans: elements are uint32 words, one or four columns; the reference is numpy's cumulative sum in uint32 per column, so a sum
that wraps 2^32 is part of what is expected.  Search: a store sorted by (tid, pos); the reference is bisect_left over the
(tid, pos) tuples.  Window walk: queries (t, wlo, whi) over such a store; the reference is numpy's searchsorted on the combined
key: the records [L, R) and (R - L) // 64 + 1 steps.  Key counters: numpy's bincount over [L, R)."""
import bisect

import numpy as np

# ---- scans -----------------------------------------------------------------------------------------------------------------

SCAN_BLOCK = 256                 # kScanBlock
CHUNK3 = 512                     # kScanBlock * kScanIters: elements per workgroup of the three-launch scan as K9 calls it
SELF_SUM_MAX = 1024              # kScanSelfSumMax: workgroups up to which phase 3 adds up the block sums itself
LB_MAX_N = (1 << 20) + 1         # no look-back launch of a test is larger (4,097 workgroups)
FILL = 0xA5A5A5A5                # what the harness fills every output with before a launch
FAMILIES = ("flags", "small", "full")


def grid3(n_upper):
    return (n_upper + CHUNK3 - 1) // CHUNK3 if n_upper else 1


def scan_reference(a):
    """inclusive prefix sums down axis 0, modulo 2^32"""
    return np.cumsum(np.asarray(a, np.uint32), axis=0, dtype=np.uint32)


def exclusive_reference(a):
    a = np.asarray(a, np.uint32)
    return scan_reference(a) - a


def values(family, n, cols, seed=0):
    """[n] (cols == 1) or [n, cols] uint32: 0/1 flags, values up to 65,535, or the full range (about half of those with bit 31
    set: a workgroup's total of 256 of them has wrapped 2^32 some hundred times)"""
    rng = np.random.default_rng([FAMILIES.index(family), cols, seed])
    hi = {"flags": 2, "small": 1 << 16, "full": 1 << 32}[family]
    v = rng.integers(0, hi, size=(n, cols), dtype=np.uint64).astype(np.uint32)
    if family == "full" and n:
        v[0] = 0xFFFFFFFF          # (the first prefix is the largest word: every further one wraps)
    return v[:, 0].copy() if cols == 1 else v


# the three-launch scan: n (= n_upper) and what each value is there for
SCAN3_SIZES = [
    1, 511, 512, 513,                                          # one chunk and its edges
    512 * 255 - 1, 512 * 255 + 1, 512 * 256 - 1, 512 * 256 + 1, 512 * 257, 512 * 257 + 1,  # the self-sum loop's second trip (workgroup 257 is the first to make it)
    512 * 1024,                                                # last self-summing grid
    512 * 1024 + 1,                                            # first phase-2 grid: 1,025 block sums, two trips of its loop
    512 * 2048 + 1,                                            # three trips
]
# (n, n_upper): the launch is chosen by n_upper and the work by *n_ptr
SCAN3_NPTR = [(0, 300), (0, 512 * 1024 + 1), (700, 512 * 1024 + 1)]


def scan3_has_total(n_upper):
    """scan_launch writes *total on the phase-2 route only"""
    return grid3(n_upper) > SELF_SUM_MAX


# the look-back scan: variant -> (columns, kIters); a launch looks at 64 / columns predecessors per window, four windows a step
LB_VARIANTS = {"u32_1": (1, 1), "u4_1": (4, 1), "u4_2": (4, 2)}
LB_TAILS = [0, 1, 63, 64, 65, 255]
LB_BLOCKS = {1: [0, 1, 63, 64, 65, 255, 256, 257, 513], 4: [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300]}


def lb_window_edges(cols):
    win = 64 // cols
    return {win - 1, win, win + 1, 4 * win - 1, 4 * win, 4 * win + 1}


def lb_sizes(variant):
    """(B, r, n): B full workgroups and a tail of r elements; every B with every r"""
    cols, iters = LB_VARIANTS[variant]
    return [(B, r, SCAN_BLOCK * iters * B + r) for B in LB_BLOCKS[cols] for r in LB_TAILS]


LB_NPTR = (1000, 100_000)                    # (n, n_upper): *n_ptr well below the bound the launch was sized for
LB_STALE_SEQUENCE = [LB_MAX_N, 300, 70_000]  # one state array, never cleared in between, consecutive stamps
LB_LAST_STAMP = 0x3FFFFFFF                   # the largest stamp; next_lb_stamp clears the words and starts again at 1

# k6_place_kernel's head: (B, r) -> n = 256 * B + r elements, B + 1 workgroups (B when r == 0), arbitrary totals
HEAD_CASES = [(B, r) for B in LB_BLOCKS[4] for r in (0, 1, 255)]


def head_workgroups(n):
    return (n + SCAN_BLOCK - 1) // SCAN_BLOCK


# ---- wave search -----------------------------------------------------------------------------------------------------------

SEARCH_SIZES = [0, 1, 2, 63, 64, 65, 66, 4159, 4160, 4161, 4224, 4225, 4226, 274_624, 274_625, 274_626, (1 << 20) + 3]
SEARCH_LARGE = (1 << 26) + (1 << 20) + 1     # the smallest size class at which a 32-bit len * (lane + 1) goes wrong
SEARCH_FAMILIES = ("distinct", "runs", "equal", "tids")
RUN_LENGTHS = (1, 64, 65, 5000)
RUN_LANES = (5, 20, 40, 60)                  # the first-round probe point each run is laid across
QUERY_COUNTS = (1, 4, 5)                     # a block with idle waves, a full one, one wave into the next block
SAMPLE = 2000
TIDS = (1, 2, 5, 6, 9)                       # 0, 3, 4, 7, 8 and 10 are absent


def probe_point(n, lane):
    """the record lane `lane` looks at in the first round of a search over n > 64 records"""
    return n * (lane + 1) // 65


def runs_layout(n):
    """[(length, start)] of the runs of equal keys in the `runs` store of n records: a run of each length of RUN_LENGTHS across
    a probe point of the first round, as far as n has room for it"""
    out, used_to = [], 0
    if n <= 64:
        return out
    for length, lane in zip(RUN_LENGTHS, RUN_LANES):
        start = probe_point(n, lane) - length // 2
        if start < used_to or start + length > n:
            continue
        out.append((length, start))
        used_to = start + length + 1
    return out


def store(family, n):
    """(tid, pos) int32 columns of n records sorted by (tid, pos)"""
    i = np.arange(n, dtype=np.int64)
    if family == "distinct":
        tid, pos = np.full(n, 7, np.int64), 3 * i - 1000
    elif family == "runs":
        tid, pos = np.full(n, 7, np.int64), 3 * i + 10
        for length, start in runs_layout(n):
            pos[start:start + length] = pos[start]
    elif family == "equal":
        tid, pos = np.full(n, 3, np.int64), np.full(n, 77, np.int64)
    elif family == "tids":
        per = max(1, -(-n // len(TIDS)))
        tid = np.asarray(TIDS, np.int64)[np.minimum(i // per, len(TIDS) - 1)]
        pos = ((i % per) // 2) * 3 - 1       # (every tid starts with two records at -1)
    else:
        raise ValueError(family)
    return tid.astype(np.int32), pos.astype(np.int32)


def large_store(n=SEARCH_LARGE):
    """a formula over the index: odd tids 1, 3, 5 ..., 2^24 records each, pairs of equal keys, every tid starting at pos -1"""
    i = np.arange(n, dtype=np.int64)
    tid = ((i >> 24) * 2 + 1).astype(np.int32)
    i &= (1 << 24) - 1
    i >>= 1
    i *= 3
    i -= 1
    return tid, i.astype(np.int32)


class KeyView:
    """the (tid, pos) tuples of a store as a sequence, for a store whose list of tuples would not fit in memory"""

    def __init__(self, tid, pos):
        self.tid, self.pos = tid, pos

    def __len__(self):
        return len(self.tid)

    def __getitem__(self, i):
        return (int(self.tid[i]), int(self.pos[i]))


def keys_of(tid, pos, as_view=False):
    return KeyView(tid, pos) if as_view else list(zip(tid.tolist(), pos.tolist()))


def search_reference(keys, qt, qp, n=None):
    """first index in [0, n) whose (tid, pos) is not below (t, p)"""
    n = len(keys) if n is None else n
    return np.array([bisect.bisect_left(keys, (int(t), int(p)), 0, n) for t, p in zip(qt, qp)], np.uint64)


def queries(tid, pos, n=None, seed=0, extra=()):
    """(qt int32, qp int64): every distinct key of a small store or a sample of SAMPLE records of a large one (first, last and
    the records `extra` among them: the ends of the runs), each with p - 1 and p + 1; below the first and above the last record; a tid below all,
    above all and absent in the middle; p = +-2^40"""
    n = len(tid) if n is None else n
    far = 1 << 40
    q = []
    if n:
        if n <= 5000:
            idx = np.arange(n)
        else:
            rng = np.random.default_rng([seed, n])
            idx = np.unique(np.concatenate([rng.integers(0, n, SAMPLE), [0, 1, n - 2, n - 1], [e for e in extra if 0 <= e < n]]).astype(np.int64))
        seen = set()
        for i in idx:
            k = (int(tid[i]), int(pos[i]))
            if k in seen:
                continue
            seen.add(k)
            q += [(k[0], k[1] - 1), k, (k[0], k[1] + 1)]
        t0, p0, t1, p1 = int(tid[0]), int(pos[0]), int(tid[n - 1]), int(pos[n - 1])
        mid = sorted(set(range(t0, t1)) - set(int(t) for t in np.unique(tid[:n][:: max(1, n // 65536)])) - {t0, t1})
        q += [(t0, p0 - 2), (t1, p1 + 2), (t0 - 1, p1 + 5), (t0 - 1, -far), (t0 - 1, far), (t1 + 1, p0 - 5), (t1 + 1, -far), (t1 + 1, far),
              (t0, -far), (t0, far), (t1, -far), (t1, far)]
        if mid:
            m = mid[len(mid) // 2]
            q += [(m, 0), (m, -far), (m, far), (m, p0), (m, p1)]
    q += [(0, 0), (0, -far), (0, far), (-1, -1), (2**31 - 1, far), (-2**31, -far)]
    return np.array([t for t, _ in q], np.int32), np.array([p for _, p in q], np.int64)


def run_ends(n):
    """records at and next to both ends of every run of runs_layout(n)"""
    return [i for length, start in runs_layout(n) for i in (start - 1, start, start + 1, start + length - 2, start + length - 1, start + length)]


# ---- window walk and key counters ------------------------------------------------------------------------------------------

WALK_STORES = [0, 1, 63, 64, 65, 128, 129, 64 * 65]
WALK_COUNTS = [0, 1, 63, 64, 65, 128]        # records in a window: none, one, and either side of one and two whole steps
WHI_WIDE = 2**31 - 2 + 2**30                 # the largest whi a kernel makes (pos 2^31 - 1, window 2^30): not a 32-bit number
WALK_RUN_STORE = 64 * 65                     # holds the runs of 1, 64 and 65 equal positions of runs_layout
WALK_TID_STORES = [5 * 64, 5 * 65, 5 * 128]  # `tids` stores whose chromosomes hold 64, 65 and 128 records
COUNT_NKEYS = [1, 2, 64, 65, 255]
COUNT_STORE = 700


def walk_reference(tid, pos, qt, qlo, qhi, n=None):
    """(L, R, steps) per query (t, wlo, whi) over the first n records: L the first record not below (t, wlo), R the first index
    >= L whose record is off t or behind whi (n if none is), and the (R - L) // 64 + 1 steps the walk takes"""
    n = len(tid) if n is None else n
    key = tid[:n].astype(np.int64) * (1 << 32) + pos[:n]
    t = np.asarray(qt, np.int64) * (1 << 32)
    # (a bound outside the int32 range stands for the nearest value outside it: no pos lies in between)
    lo = t + np.clip(np.asarray(qlo, np.int64), -(1 << 31), 1 << 31)
    hi = t + np.clip(np.asarray(qhi, np.int64), -(1 << 31) - 1, (1 << 31) - 1)
    L = np.searchsorted(key, lo, "left").astype(np.int64)
    R = np.maximum(L, np.searchsorted(key, hi, "right").astype(np.int64))
    return L, R, (R - L) // 64 + 1


def _windows_at(pos, n, t):
    """windows of every count of WALK_COUNTS at the first record, ending at the last, and in the middle of a store of distinct positions
    three apart"""
    q = []
    for k in WALK_COUNTS:
        if k > n:
            continue
        for a in sorted({0, n - k, (n - k) // 2}):
            if k:
                q.append((t, int(pos[a]), int(pos[a + k - 1])))
            elif a < n:
                q.append((t, int(pos[a]) + 1, int(pos[a]) + 2))       # between two records (behind the last one for a == n - 1)
        if k == 0 and n:
            q.append((t, int(pos[0]) - 2, int(pos[0]) - 1))           # in front of the first record
    return q


def walk_cases():
    """[(label, family, n_upper, n, [(t, wlo, whi)])]: the stores and windows at which the walk can go wrong"""
    far = 1 << 40
    out = []
    for n in WALK_STORES:
        tid, pos = store("distinct", n)   # tid 7, pos = 3 i - 1000: negative up to record 333
        q = _windows_at(pos, n, 7)
        q += [(7, -far, WHI_WIDE), (7, -(1 << 31) - 5, -1), (7, -2000, WHI_WIDE), (7, 5, 4), (7, WHI_WIDE, -far), (7, -1000, -1001),
              (6, -far, WHI_WIDE), (8, -far, WHI_WIDE), (0, 0, 0), (2**31 - 1, -far, far), (-1, -far, far)]
        out.append(("distinct-%d" % n, "distinct", n, n, q))
    # the store ends inside the window although the memory behind it holds records that would lie inside
    _, pos = store("distinct", 129 + 64)
    out.append(("prefix-128", "distinct", 129 + 64, 128, [(7, -far, WHI_WIDE), (7, int(pos[64]), int(pos[191])), (7, int(pos[127]), int(pos[128])), (7, int(pos[128]), WHI_WIDE)]))
    out.append(("prefix-0", "distinct", 64, 0, [(7, -far, WHI_WIDE), (7, -1000, -1000)]))
    # a window that ends with its chromosome while the next one starts at positions <= whi; absent chromosomes; one behind the last
    for n in WALK_TID_STORES:
        tid, pos = store("tids", n)
        per = n // len(TIDS)
        q = []
        for c, t in enumerate(TIDS):
            end = (c + 1) * per
            for k in (1, 2, 63, 64, 65, 66, 128):
                if k <= per:
                    q.append((t, int(pos[end - k]), WHI_WIDE))
            q += [(t, -far, WHI_WIDE), (t, -1, -1), (t, int(pos[end - 1]) + 1, WHI_WIDE)]
        q += [(t, -far, WHI_WIDE) for t in (0, 3, 4, 7, 8, 10, 11)]
        out.append(("tids-%d" % n, "tids", n, n, q))
    # runs of equal positions across wlo and across whi
    n = WALK_RUN_STORE
    tid, pos = store("runs", n)
    q = []
    for length, start in runs_layout(n):
        v, before, after = int(pos[start]), int(pos[start - 1]), int(pos[start + length])
        q += [(7, v, v), (7, v + 1, after), (7, v + 1, WHI_WIDE), (7, before, v), (7, before, v - 1), (7, -far, v), (7, -far, v - 1), (7, v, after)]
    out.append(("runs-%d" % n, "runs", n, n, q))
    return out


def walk_arrays(queries):
    return (np.array([t for t, _, _ in queries], np.int32), np.array([lo for _, lo, _ in queries], np.int64), np.array([hi for _, _, hi in queries], np.int64))


def count_store(n=COUNT_STORE):
    """a `tids` store with a hit byte (0, or 1 / 2 / 255: three records in four are hits) and a key byte per record: half of them
    0 ... 3, the others over the whole range; the first chromosome's first records are hits with the last key of every COUNT_NKEYS,
    with key 0 and with key 255 (out of range for every nkeys) whatever the draw"""
    tid, pos = store("tids", n)
    rng = np.random.default_rng([77, n])
    hit = rng.choice(np.array([0, 1, 2, 255], np.uint8), n)
    key = np.where(rng.random(n) < 0.5, rng.integers(0, 4, n), rng.integers(0, 256, n)).astype(np.uint8)
    fixed = [255, 0] + [k - 1 for k in COUNT_NKEYS if k > 1]
    key[:len(fixed)], hit[:len(fixed)] = fixed, 1
    return tid, pos, hit, key


def count_queries(tid, pos):
    """five windows: a whole chromosome, an absent one (a row of zeros), 64 records, everything of the first chromosome from its start,
    the last chromosome up to the store's end"""
    n = len(tid)
    per = n // len(TIDS)
    far = 1 << 40
    return [(TIDS[0], -far, WHI_WIDE), (3, -far, WHI_WIDE), (TIDS[2], int(pos[2 * per + 10]), int(pos[2 * per + 73])), (TIDS[0], -1, int(pos[per - 1])),
            (TIDS[-1], int(pos[n - 65]), WHI_WIDE)]


def count_reference(tid, pos, hit, key, qt, qlo, qhi, nkeys):
    """[nq][nkeys] uint32: the hits of [L, R) per key, a key >= nkeys counted as key 0"""
    L, R, _ = walk_reference(tid, pos, qt, qlo, qhi)
    out = np.zeros((len(qt), nkeys), np.uint32)
    for q, (a, b) in enumerate(zip(L, R)):
        k = key[a:b][hit[a:b] != 0].astype(np.int64)
        out[q] = np.bincount(np.where(k < nkeys, k, 0), minlength=nkeys)
    return out
