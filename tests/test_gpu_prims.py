"""The shared primitives of pass 1 and of the query kernels on their own, through tests/prims/prims.hip: the three-launch scan
(scan_launch, as K9 calls it), the look-back scan (scan_launch_lb, the three instantiations of K3), the walk itself as
k6_place_kernel calls it (lookback_exclusive), the 64-ary search of K8 / KS / KI (wave_lower_bound), the window walk they build
on it (wave_window_walk) and the per-wave key counters of K8 / KS (WaveKeyCounts), each against the CPU references of
tests/prims_cases.py at the sizes where their routes, windows, rounds and steps change.  Every comparison is exact.

The look-back launches keep to the scan's preconditions (state sized for n_upper and zero once, a fresh stamp per launch); the
harness refuses a call that would not, and no such launch is ever made."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import prims_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "tests/prims/libbdx_prims.so"
HIP_INVALID_VALUE = 1

_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        env = dict(os.environ)
        env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call(["make", "-C", ROOT, TARGET], env=env)
    so = ctypes.CDLL(path)
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    for name in ("prims_scan3_u32", "prims_scan3_u4"):
        getattr(so, name).argtypes = [_u32p, _u32p, u32, u32, _u32p, _u32p]
    for name in ("prims_scan_lb_u32_1", "prims_scan_lb_u4_1", "prims_scan_lb_u4_2"):
        getattr(so, name).argtypes = [_u32p, _u32p, u32, u32, vp, u32, _u32p]
    so.prims_lb_state_new.argtypes = [u32, ctypes.c_int, ctypes.POINTER(vp)]
    so.prims_lb_state_clear.argtypes = [vp]
    so.prims_lb_state_free.argtypes = [vp]
    so.prims_lb_state_free.restype = None
    so.prims_lb_head.argtypes = [_u32p, _u32p, u32, u32, vp, u32]
    so.prims_search.argtypes = [_i32p, _i32p, u64, u64, _i32p, _i64p, u32, _u64p]
    so.prims_walk.argtypes = [_i32p, _i32p, u64, u64, _i32p, _i64p, _i64p, u32, _u32p, _u32p, _u32p]
    so.prims_key_counts.argtypes = [_i32p, _i32p, u64, _u8p, _u8p, _i32p, _i64p, _i64p, u32, ctypes.c_int, _u32p]
    return so


class State:
    """look-back words sized for n_upper, zero once; hands out the stamps: never the same one twice"""

    def __init__(self, so, n_upper, cols):
        self.so, self.cols, self.stamp = so, cols, 0
        self.h = ctypes.c_void_p()
        assert so.prims_lb_state_new(n_upper, cols, ctypes.byref(self.h)) == 0

    def next_stamp(self):
        self.stamp += 1
        return self.stamp

    def clear(self):
        assert self.so.prims_lb_state_clear(self.h) == 0
        self.stamp = 0

    def free(self):
        self.so.prims_lb_state_free(self.h)
        self.h = None


@pytest.fixture(scope="module")
def states(lib):
    """one state array per column count for the whole module: like a context's, it goes from launch to launch uncleared"""
    st = {cols: State(lib, pc.LB_MAX_N, cols) for cols in (1, 4)}
    yield st
    for s in st.values():
        s.free()


@pytest.fixture(scope="module")
def pools():
    """per (family, columns): LB_MAX_N values and their running sums, computed once; a case takes the first n of both"""
    out = {}
    for cols in (1, 4):
        for family in pc.FAMILIES:
            v = pc.values(family, pc.LB_MAX_N, cols)
            v.setflags(write=False)
            ref = pc.scan_reference(v)
            ref.setflags(write=False)
            out[family, cols] = (v, ref)
    return out


def shaped(n, cols):
    return (n,) if cols == 1 else (n, cols)


def check_scan(got, flags, ref, n, n_upper, what):
    assert flags.tolist() == [0, 0, 0, 0], (what, "n handed over != *n_ptr / e != input / lanes not consecutive", flags.tolist())
    diff = got[:n] != ref[:n]
    bad = np.flatnonzero(diff.any(axis=1) if diff.ndim > 1 else diff)
    assert bad.size == 0, (what, "first wrong element", int(bad[0]), got[bad[0]].tolist(), ref[bad[0]].tolist(), "wrong elements", int(bad.size))
    assert (got[n:] == pc.FILL).all(), (what, "written past n")


def run_scan3(lib, cols, v, n, n_upper):
    fn = lib.prims_scan3_u32 if cols == 1 else lib.prims_scan3_u4
    src = np.ascontiguousarray(v[:n_upper])
    got = np.zeros(shaped(n_upper, cols), np.uint32)
    total, flags = np.zeros(cols, np.uint32), np.zeros(4, np.uint32)
    assert fn(src, got, n, n_upper, total, flags) == 0
    return got, total, flags


# ---- three-launch scan -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [1, 4])
@pytest.mark.parametrize("n", pc.SCAN3_SIZES)
def test_three_launch_scan(lib, pools, cols, n):
    """scan_launch<uint32_t> and scan_launch<U4> at 512 elements a workgroup: one chunk and its edges, the second trip of phase 3's
    own sum over the preceding block sums, the last self-summing grid, and beyond it scan_phase2 with two and three trips of its
    loop and scan_phase3 reading its offsets; *total is the grand sum there and untouched on the self-summing route"""
    for family in pc.FAMILIES if n <= 512 * 257 + 1 else ("full",):
        v, ref = pools[family, cols]
        got, total, flags = run_scan3(lib, cols, v, n, n)
        check_scan(got, flags, ref, n, n, (family, cols, n))
        if pc.scan3_has_total(n):
            assert total.tolist() == ref[n - 1].reshape(-1).tolist(), (family, cols, n)
        else:
            assert total.tolist() == [pc.FILL] * cols, "scan_launch wrote *total on the self-summing route"


@pytest.mark.parametrize("cols", [1, 4])
@pytest.mark.parametrize("n,n_upper", pc.SCAN3_NPTR)
def test_three_launch_scan_works_on_n_ptr_under_a_grid_for_n_upper(lib, pools, cols, n, n_upper):
    """the launch is chosen by n_upper, the work by *n_ptr: nothing at all with *n_ptr == 0 (one workgroup, and more than 1,024),
    700 elements under a phase-2 grid of 1,025"""
    v, ref = pools["full", cols]
    got, total, flags = run_scan3(lib, cols, v, n, n_upper)
    check_scan(got, flags, ref, n, n_upper, (cols, n, n_upper))
    if pc.scan3_has_total(n_upper):
        assert total.tolist() == (ref[n - 1].reshape(-1).tolist() if n else [0] * cols)
    else:
        assert total.tolist() == [pc.FILL] * cols


# ---- look-back scan --------------------------------------------------------------------------------------------------------

def run_lb(lib, variant, state, v, n, n_upper, stamp=None):
    cols, _ = pc.LB_VARIANTS[variant]
    assert state.cols == cols
    src = np.ascontiguousarray(v[:n_upper])
    got = np.zeros(shaped(n_upper, cols), np.uint32)
    flags = np.zeros(4, np.uint32)
    rc = getattr(lib, "prims_scan_lb_" + variant)(src, got, n, n_upper, state.h, state.next_stamp() if stamp is None else stamp, flags)
    assert rc == 0, rc
    return got, flags


@pytest.mark.parametrize("variant", list(pc.LB_VARIANTS))
def test_look_back_scan_at_the_window_edges(lib, pools, states, variant):
    """B full workgroups and a tail of r elements for every B around one window (64 / columns predecessors) and one step (four
    windows) of the walk, with every r, in the three value families -- the full-range one wraps every total and prefix; then
    2^20 + 1 elements, and *n_ptr far below n_upper.  All on one state array that is never cleared"""
    cols, _ = pc.LB_VARIANTS[variant]
    for B, r, n in pc.lb_sizes(variant):
        for family in pc.FAMILIES:
            v, ref = pools[family, cols]
            got, flags = run_lb(lib, variant, states[cols], v, n, n)
            check_scan(got, flags, ref, n, n, (variant, family, B, r))
    v, ref = pools["full", cols]
    got, flags = run_lb(lib, variant, states[cols], v, pc.LB_MAX_N, pc.LB_MAX_N)
    check_scan(got, flags, ref, pc.LB_MAX_N, pc.LB_MAX_N, (variant, "2^20 + 1"))
    n, n_upper = pc.LB_NPTR
    got, flags = run_lb(lib, variant, states[cols], v, n, n_upper)
    check_scan(got, flags, ref, n, n_upper, (variant, "n_ptr below n_upper"))


@pytest.mark.parametrize("variant", list(pc.LB_VARIANTS))
def test_look_back_scan_over_words_of_earlier_launches(lib, pools, variant):
    """a state array of its own, never cleared: 2^20 + 1 elements, then 300, then 70,000 under consecutive stamps -- the later
    launches find the words of a launch with more workgroups and another stamp at their predecessors' places; then the largest
    stamp, and what next_lb_stamp does when its counter comes round: the words cleared, stamp 1 again"""
    cols, _ = pc.LB_VARIANTS[variant]
    st = State(lib, pc.LB_MAX_N, cols)
    try:
        for family in ("full", "flags"):
            v, ref = pools[family, cols]
            for n in pc.LB_STALE_SEQUENCE:
                got, flags = run_lb(lib, variant, st, v, n, n)
                check_scan(got, flags, ref, n, n, (variant, family, n, "stamp", st.stamp))
        assert st.stamp == 2 * len(pc.LB_STALE_SEQUENCE)
        v, ref = pools["small", cols]
        got, flags = run_lb(lib, variant, st, v, 70_000, 70_000, stamp=pc.LB_LAST_STAMP)
        check_scan(got, flags, ref, 70_000, 70_000, (variant, "last stamp"))
        st.clear()
        got, flags = run_lb(lib, variant, st, v, 70_000, 70_000)
        assert st.stamp == 1
        check_scan(got, flags, ref, 70_000, 70_000, (variant, "stamp 1 after the clear"))
    finally:
        st.free()


@pytest.fixture(scope="module")
def head_totals():
    t = pc.values("full", 301, 4, seed=9)
    t.setflags(write=False)
    return t, pc.exclusive_reference(t)


def test_look_back_walk_as_k6_place_calls_it(lib, states, head_totals):
    """lookback_exclusive<U4> called by all 256 threads of every workgroup with an arbitrary total: every thread gets the sum of
    the totals of the workgroups before its own, at every workgroup count around a window and a step; workgroups past n do
    nothing"""
    tots, excl = head_totals
    st = states[4]
    for B, r in pc.HEAD_CASES:
        n = 256 * B + r
        for n_upper in (n, n + 1000) if B in (16, 64) else (n,):
            w, w_upper = pc.head_workgroups(n), max(1, pc.head_workgroups(n_upper))
            src = np.ascontiguousarray(tots[:w_upper])
            got = np.zeros((w_upper, 256, 4), np.uint32)
            assert lib.prims_lb_head(src, got, n, n_upper, st.h, st.next_stamp()) == 0
            same = (got[:w] == got[:w, :1]).all()
            assert same, ("threads of one workgroup disagree on the carry", B, r)
            bad = np.flatnonzero((got[:w, 0] != excl[:w]).any(axis=1))
            assert bad.size == 0, (B, r, "first wrong workgroup", int(bad[0]), got[bad[0], 0].tolist(), excl[bad[0]].tolist())
            assert (got[w:] == pc.FILL).all(), (B, r, "a workgroup past n wrote")


def test_the_harness_refuses_a_launch_that_would_break_the_preconditions(lib, pools):
    """no launch is made for a used stamp, stamp 0, a state array too small or of another column count, or n above n_upper
    (such a launch would wait for words that never come)"""
    v, _ = pools["flags", 1]
    st = State(lib, 1000, 1)
    try:
        src, got, flags = np.ascontiguousarray(v[:1000]), np.zeros(1000, np.uint32), np.zeros(4, np.uint32)
        assert lib.prims_scan_lb_u32_1(src, got, 1000, 1000, st.h, 5, flags) == 0
        assert lib.prims_scan_lb_u32_1(src, got, 1000, 1000, st.h, 5, flags) == HIP_INVALID_VALUE
        assert lib.prims_scan_lb_u32_1(src, got, 1000, 1000, st.h, 0, flags) == HIP_INVALID_VALUE
        assert lib.prims_scan_lb_u32_1(src, got, 1000, 1000, st.h, 0x40000000, flags) == HIP_INVALID_VALUE
        assert lib.prims_scan_lb_u32_1(src, got, 1000, 500, st.h, 6, flags) == HIP_INVALID_VALUE
        big = np.zeros(2000, np.uint32)
        assert lib.prims_scan_lb_u32_1(big, big.copy(), 2000, 2000, st.h, 7, flags) == HIP_INVALID_VALUE
        assert lib.prims_scan_lb_u4_1(np.zeros((10, 4), np.uint32), np.zeros((10, 4), np.uint32), 10, 10, st.h, 8, flags) == HIP_INVALID_VALUE
    finally:
        st.free()


# ---- wave search -----------------------------------------------------------------------------------------------------------

def run_search(lib, tid, pos, n, qt, qp):
    got = np.zeros((len(qt), 64), np.uint64)
    assert lib.prims_search(tid, pos, n, len(tid), np.ascontiguousarray(qt), np.ascontiguousarray(qp), len(qt), got) == 0
    return got


def check_search(got, want, qt, qp, what):
    uniform = (got == got[:, :1]).all(axis=1)
    assert uniform.all(), (what, "lanes of a wave disagree at query", int(np.flatnonzero(~uniform)[0]))
    bad = np.flatnonzero(got[:, 0] != want)
    assert bad.size == 0, (what, "first wrong query", (int(qt[bad[0]]), int(qp[bad[0]])), "got", int(got[bad[0], 0]), "want", int(want[bad[0]]), "wrong", int(bad.size))


@pytest.mark.parametrize("family", pc.SEARCH_FAMILIES)
def test_wave_search(lib, family):
    """wave_lower_bound over stores of 0 ... 2^20 + 3 records, the sizes either side of one, two and three rounds of 65-fold
    narrowing (64, 65, 64 * 65, 65^2, 65^3): every key (a sample of the large stores'), p - 1 and p + 1 of each, keys below
    and above the store, absent chromosomes, p = +-2^40; and the same over a prefix of the store"""
    for n in pc.SEARCH_SIZES:
        tid, pos = pc.store(family, n)
        keys = pc.keys_of(tid, pos)
        qt, qp = pc.queries(tid, pos, extra=pc.run_ends(n) if family == "runs" else ())
        check_search(run_search(lib, tid, pos, n, qt, qp), pc.search_reference(keys, qt, qp), qt, qp, (family, n))
        if n in (66, 4226, 274_626):   # the store cut one and two records short: the size below, without a second upload's worth of cases
            for m in (n - 1, n - 2):
                check_search(run_search(lib, tid, pos, m, qt, qp), pc.search_reference(keys, qt, qp, m), qt, qp, (family, n, "first", m))


@pytest.mark.parametrize("nq", pc.QUERY_COUNTS)
def test_wave_search_with_idle_waves_and_a_second_block(lib, nq):
    """one query (three waves of the block leave at once), four (a full block), five (one wave of a second block)"""
    for family in pc.SEARCH_FAMILIES:
        for n in (65, 4161):
            tid, pos = pc.store(family, n)
            qt, qp = pc.queries(tid, pos)
            for first in (0, 7, len(qt) - nq):
                t, p = qt[first:first + nq], qp[first:first + nq]
                assert len(t) == nq
                check_search(run_search(lib, tid, pos, n, t, p), pc.search_reference(pc.keys_of(tid, pos), t, p), t, p, (family, n, nq, first))


def test_wave_search_beyond_2_26_records(lib):
    """2^26 + 2^20 + 1 records: the first round's len * (lane + 1) no longer fits 32 bits, and the search takes its full five
    rounds.  The store is a formula over the index (prims_cases.large_store); the reference reads it through a sequence view"""
    tid, pos = pc.large_store()
    n = len(tid)
    assert n == pc.SEARCH_LARGE
    qt, qp = pc.queries(tid, pos, seed=3, extra=[(1 << 26) + k for k in (-1, 0, 1, 2)] + [(1 << 24) * k + d for k in (1, 2, 3, 4) for d in (-2, -1, 0, 1)])
    got = run_search(lib, tid, pos, n, qt, qp)
    want = pc.search_reference(pc.keys_of(tid, pos, as_view=True), qt, qp)
    assert (want > 1 << 26).sum() > 10 and (want == n).sum() >= 3 and (want == 0).sum() >= 3
    check_search(got, want, qt, qp, "large")


# ---- window walk and key counters ------------------------------------------------------------------------------------------

WALK_CASES = {case[0]: case for case in pc.walk_cases()}
WALK_FLAGS = "a body call without all 64 lanes (1) / lane l not at lane 0's index + l (2) / s not the record's pos or a record past n (4)"


def run_walk(lib, tid, pos, n, queries):
    qt, qlo, qhi = pc.walk_arrays(queries)
    nq = len(qt)
    visits, steps, flags = np.zeros((nq, len(tid)), np.uint32), np.zeros((nq, 64), np.uint32), np.zeros((nq, 64), np.uint32)
    assert lib.prims_walk(tid, pos, n, len(tid), qt, qlo, qhi, nq, visits, steps, flags) == 0
    return visits, steps, flags


def check_walk(got, tid, pos, n, queries, what):
    visits, steps, flags = got
    L, R, want_steps = pc.walk_reference(tid, pos, *pc.walk_arrays(queries), n)
    bad = np.flatnonzero((flags != 0).any(axis=1))
    assert bad.size == 0, (what, WALK_FLAGS, "first query", queries[bad[0]], flags[bad[0]].tolist())
    bad = np.flatnonzero((steps != want_steps[:, None]).any(axis=1))
    assert bad.size == 0, (what, "steps: first wrong query", queries[bad[0]], "got", steps[bad[0]].tolist(), "want", int(want_steps[bad[0]]))
    idx = np.arange(len(tid))
    want = ((idx >= L[:, None]) & (idx < R[:, None])).astype(np.uint32)
    bad = np.flatnonzero((visits != want).any(axis=1))
    assert bad.size == 0, (what, "visits: first wrong query", queries[bad[0]], "want each of", (int(L[bad[0]]), int(R[bad[0]])), "once; differs at",
                           np.flatnonzero(visits[bad[0]] != want[bad[0]])[:8].tolist())


@pytest.mark.parametrize("label", list(WALK_CASES))
def test_window_walk(lib, label):
    """wave_window_walk over stores of 0 ... 64 * 65 records and windows of 0, 1, 63, 64, 65 and 128 records at the store's first
    record, ending at its last (the extra step of a window of whole steps then runs wholly behind n) and in the middle; windows that
    end with their chromosome while the next one starts at positions <= whi; absent chromosomes; runs of equal positions at wlo - 1,
    wlo, whi and whi + 1; wlo negative, whi = 2^31 - 2 + 2^30, wlo > whi; a store that ends inside the window.  Per query: every
    record of [L, R) handed to the body once with `in` and no other, (R - L) / 64 + 1 steps on every lane, all 64 lanes in every
    body call, consecutive records in consecutive lanes"""
    _, family, n_upper, n, queries = WALK_CASES[label]
    tid, pos = pc.store(family, n_upper)
    check_walk(run_walk(lib, tid, pos, n, queries), tid, pos, n, queries, label)


@pytest.mark.parametrize("nq", pc.QUERY_COUNTS)
def test_window_walk_with_idle_waves_and_a_second_block(lib, nq):
    """one query (three waves of the block leave at once), four (a full block), five (one wave of a second block)"""
    for label in ("distinct-129", "tids-%d" % pc.WALK_TID_STORES[0]):
        _, family, n_upper, n, queries = WALK_CASES[label]
        tid, pos = pc.store(family, n_upper)
        for first in (0, 9, len(queries) - nq):
            q = queries[first:first + nq]
            assert len(q) == nq
            check_walk(run_walk(lib, tid, pos, n, q), tid, pos, n, q, (label, nq, first))


@pytest.fixture(scope="module")
def count_case():
    tid, pos, hit, key = pc.count_store()
    for a in (tid, pos, hit, key):
        a.setflags(write=False)
    return tid, pos, hit, key, pc.count_queries(tid, pos)


@pytest.mark.parametrize("nq", pc.QUERY_COUNTS)
@pytest.mark.parametrize("nkeys", pc.COUNT_NKEYS)
def test_wave_key_counts(lib, count_case, nkeys, nq):
    """WaveKeyCounts under the walk, as K8 and KS use it: one key by ballot + popcount, 2, 64, 65 and 255 keys through the per-wave LDS
    rows, hits with a key >= nkeys counted as key 0, against numpy.bincount over [L, R); with one query and with five the last block
    has three waves without a query, which reach both barriers and leave their rows of the prefilled output untouched"""
    tid, pos, hit, key, queries = count_case
    qt, qlo, qhi = pc.walk_arrays(queries[:nq])
    rows = (nq + 3) // 4 * 4
    got = np.zeros((rows, nkeys), np.uint32)
    assert lib.prims_key_counts(tid, pos, len(tid), hit, key, qt, qlo, qhi, nq, nkeys, got) == 0
    want = pc.count_reference(tid, pos, hit, key, qt, qlo, qhi, nkeys)
    bad = np.flatnonzero((got[:nq] != want).any(axis=1))
    assert bad.size == 0, (nkeys, nq, "first wrong query", queries[bad[0]], "keys", np.flatnonzero(got[bad[0]] != want[bad[0]])[:8].tolist(),
                           "got", got[bad[0]][got[bad[0]] != want[bad[0]]][:8].tolist(), "want", want[bad[0]][got[bad[0]] != want[bad[0]]][:8].tolist())
    assert (got[nq:] == pc.FILL).all(), (nkeys, nq, "a wave without a query wrote its row")
