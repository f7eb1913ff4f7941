"""GPU tests of --mini: bdx_window_insert_shift (KW, csrc/km_mini.hip) against the numpy restatement of tests/mini_cases.py, field by
field and exactly, on the production routing and with "mini_staged" forced; its argument and state errors; two ranks on one GPU; and the
command end to end on planted synthetic BAMs and on the chr21 golden fixture.

The stores come from test_gpu_sites.Store through the oracle.  They are laid out by record index: on every sequence the lower mates sit
ten positions apart, so the observations are counted off by position, and the windows are cut to hold exactly 0, 1, 63, 64, 65,
MINI_CAP - 1, MINI_CAP and MINI_CAP + 1 of them.  Each test asserts from the restatement, before it uses the GPU, that every class of
window and record it means to submit is there."""
import os
import subprocess

import numpy as np
import pytest

import mini_cases as M
import test_gpu_sites as T
from helpers import GOLDEN, ROOT, filter_cmd_lines, load_chr21, make_opts
from runner import oracle_case, product_from_oracle, sharded_from_oracle

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHECK = os.path.join(ROOT, "bin", "bdx-mini-check")
CWD = os.path.join(GOLDEN, "chr21")
IMAX = 2**31 - 1
BINS, CAP = M.ISIZE_BINS, M.MINI_CAP
PAIRS = {0: 6000, 1: 3000, 3: 1000}          # lower mates per sequence, at 1000 + 10 i; c2 stays empty
EQUAL_AT, DISTINCT_AT, SPLIT_AT = 100, 300, 500   # c0: 100 pairs of one insert, 100 of distinct inserts, and (three libraries) 64 + 1 + 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the store
# ---------------------------------------------------------------------------------------------------------------------------------
def index_store(libs, seed):
    rng = np.random.default_rng(seed)
    st = T.Store(libs)

    def last_pair(**change):
        for recs in st.recs:
            for r in recs:
                if r["name"] == st.names:
                    for k, f in change.items():
                        r[k] = f(r)

    for tid, npairs in PAIRS.items():
        for i in range(npairs):
            li = int(rng.integers(0, len(libs)))
            mean, std = libs[li][3], libs[li][4]
            ins = int(round(rng.normal(mean, std)))
            if i % 97 == 5:
                ins = int(mean + 8 * std)                     # ARP_LARGE_INSERT
            if i % 97 == 6:
                ins = int(mean - 6 * std)                     # ARP_SMALL_INSERT
            if tid == 0 and EQUAL_AT <= i < EQUAL_AT + 100:
                li, ins = 0, 400
            if tid == 0 and DISTINCT_AT <= i < DISTINCT_AT + 100:
                li, ins = 0, 350 + (i - DISTINCT_AT)
            if tid == 0 and SPLIT_AT <= i < SPLIT_AT + 65 and len(libs) > 1:
                li = 0 if i < SPLIT_AT + 64 else 1
                ins = int(libs[li][3])
            pa = 1000 + 10 * i
            st.pair(li, tid, pa, tid, pa + max(ins, T.RL + 1) - T.RL, False, True)
            if i % 2 == 0:
                last_pair(flag=lambda r: r["flag"] | 0x2)     # proper pairs: what KH's own histogram counts
    # the special pairs, on c1 between the grid positions (their lower mates at ...5)
    at = lambda k: 1000 + 10 * (200 + 20 * k) + 5
    st.pair(0, 1, at(0), 1, at(0) + 300, False, False)                                   # ARP_FF
    st.pair(0, 1, at(1), 1, at(1) + 300, True, False)                                    # ARP_RF
    st.pair(0, 1, at(2), 3, 5005, False, True)                                           # ARP_CTX: mtid != tid
    st.pair(0, 1, at(3), 1, at(3) + 300, False, True, mapq=0)                            # fails -q
    st.pair(0, 1, at(4), 1, at(4) + 300, False, True)
    last_pair(flag=lambda r: r["flag"] | 0x400)                                          # a duplicate
    st.pair(0, 1, at(5), 1, at(5), False, True)                                          # both mates at one place: the second has the class, and does not count
    st.pair(0, 1, at(10), 1, at(10), True, False)                                        # likewise, but the first in pair has the class: it counts
    st.pair(0, 1, at(6), 1, at(6) + 300, False, True)
    last_pair(isize=lambda r: 0)                                                         # x = 0
    st.pair(len(libs) - 1, 1, at(7), 1, at(7) + BINS - 1 - T.RL, False, True)            # x = BINS - 1
    st.pair(len(libs) - 1, 1, at(8), 1, at(8) + BINS - T.RL, False, True)                # x = BINS: n_over
    st.pair(0, 1, at(9), 1, at(9) + 300, False, True)
    last_pair(isize=lambda r: -r["isize"])                                               # a negative isize on the lower mate
    return st


SPECIAL = [1000 + 10 * (200 + 20 * k) + 5 for k in range(11)]
STORES, NULLS = {}, {}


def case(label):
    """(oracle run, merged stream) of "one" / "three": built and run through the oracle once"""
    if label not in STORES:
        libs = T.ONE_LIB if label == "one" else T.THREE_LIBS
        run = oracle_case(T.config_text(libs), index_store(libs, 3 + len(label)).streams(), T.TARGETS, make_opts())
        STORES[label] = (run, run.merged_soa())
    return STORES[label]


def windows_of(label):
    """the windows of a store, and the assertion that every class of window and record is among them"""
    run, soa = case(label)
    nlibs = run.nlibs
    ok, x, lib = M.qualifies(soa, run.cls, nlibs)
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    obs = ok & (x < BINS)
    iv = [(0, 0, 0), (0, 5000, 5000), (2, 0, IMAX), (2, 100, 5000), (4, 0, IMAX), (1000, 0, IMAX), (IMAX, 0, IMAX), (0, IMAX, IMAX), (0, 0, 1),
          (3, int(s[-1]) + 1, IMAX), (int(t[-1]), int(s[-1]), IMAX)]
    exact = {}
    for tid in (0, 1, 3):
        P = np.unique(s[obs & (t == tid)])
        assert len(P) == int((obs & (t == tid)).sum())                     # (distinct starts: counted off by position)
        idx = np.nonzero(t == tid)[0]
        iv += [(tid, 0, IMAX), (tid, int(s[idx[0]]), int(s[idx[0]]) + 1), (tid, int(s[idx[-1]]), int(s[idx[-1]]) + 1), (tid, int(s[idx[-1]]), IMAX)]
        sizes = (0, 1, 63, 64, 65, CAP - 1, CAP, CAP + 1) if tid == 0 else (1, 63, 64, 65, 130, 700)
        for k in sizes:
            for a in (7, 1500 if tid == 0 else 40):
                if a + k < len(P):
                    w = (tid, int(P[a]) + 1, int(P[a + 1])) if k == 0 else (tid, int(P[a]), int(P[a + k]))
                    iv.append(w)
                    exact[w] = k
    at0 = lambda i: 1000 + 10 * i
    iv += [(0, at0(EQUAL_AT), at0(EQUAL_AT + 64)), (0, at0(EQUAL_AT), at0(EQUAL_AT + 100)), (0, at0(DISTINCT_AT), at0(DISTINCT_AT + 64)),
           (0, at0(DISTINCT_AT), at0(DISTINCT_AT + 100)), (0, at0(SPLIT_AT), at0(SPLIT_AT + 65)), (0, at0(EQUAL_AT - 30), at0(DISTINCT_AT + 130))]
    iv += [(1, p, p + 1) for p in SPECIAL] + [(1, SPECIAL[0] - 40, SPECIAL[-1] + 40)]
    uppers = np.nonzero(((run.cls & 0x10) != 0) & np.isin(run.cls & 15, M.MINI_CLASSES) & (t == soa["mtid"]) & ~ok & ~np.isin(s, s[ok]))[0]
    iv += [(int(t[i]), int(s[i]), int(s[i]) + 1) for i in uppers[:3]]      # an upper mate alone in its window
    order = np.random.default_rng(5).permutation(len(iv))
    iv = [iv[i] for i in order]                                            # unsorted, and overlapping anyway
    # ---- what is there ----
    inside = np.zeros(len(t), bool)
    for tid, beg, end in iv:
        inside |= (t == tid) & (s >= beg) & (s < end)
    passed, f, fl = (run.cls & 0x10) != 0, run.cls & 15, soa["flag"].astype(np.int64)
    mt, ms = soa["mtid"].astype(np.int64), soa["mpos"].astype(np.int64)
    good = passed & np.isin(f, M.MINI_CLASSES)
    has = {
        "an observation of every class": all((inside & ok & (f == c)).any() for c in (6, 2, 3)),
        "an upper mate": (inside & good & (mt == t) & (s > ms)).any(),
        "equal positions, not first in pair": (inside & good & (mt == t) & (s == ms) & ((fl & 0x40) == 0)).any(),
        "equal positions, first in pair": (inside & ok & (s == ms)).any(),
        "ARP_FF, ARP_RF, ARP_CTX": all((inside & passed & (f == c)).any() for c in (1, 4, 8)),
        "a failed -q": (inside & ~passed & (soa["bdqual"] == 0)).any(),
        "0x400": (inside & ((fl & 0x400) != 0)).any(),
        "mtid != tid": (inside & passed & (mt != t)).any(),
        "x = 0": (inside & ok & (x == 0)).any(), "x = BINS - 1": (inside & ok & (x == BINS - 1)).any(), "x = BINS": (inside & ok & (x == BINS)).any(),
        "a negative isize on the lower mate": (inside & ok & (soa["isize"] < 0)).any(),
    }
    assert all(has.values()), [k for k, v in has.items() if not v]
    total = lambda w: int((obs & (t == w[0]) & (s >= w[1]) & (s < w[2])).sum())
    assert all(total(w) == k for w, k in exact.items())
    assert {k for k in exact.values()} >= {0, 1, 63, 64, 65, CAP - 1, CAP, CAP + 1}
    eq = (0, at0(EQUAL_AT), at0(EQUAL_AT + 64))
    m = obs & (t == 0) & (s >= eq[1]) & (s < eq[2])
    assert m.sum() == 64 and len(set(x[m].tolist())) == 1
    di = (0, at0(DISTINCT_AT), at0(DISTINCT_AT + 64))
    m = obs & (t == 0) & (s >= di[1]) & (s < di[2])
    assert m.sum() == 64 and len(set(x[m].tolist())) == 64
    if nlibs == 3:
        m = obs & (t == 0) & (s >= at0(SPLIT_AT)) & (s < at0(SPLIT_AT + 65))
        assert np.bincount(lib[m], minlength=3).tolist() == [64, 1, 0]
    return iv


def nulls_of(label, own):
    """named nulls hist[nlibs][BINS]: KH's own histogram of the store (given), one library emptied, one bin, all mass above / below"""
    nlibs = own.shape[0]
    out = {"own": own.copy()}
    one_empty = own.copy()
    one_empty[nlibs - 1] = 0
    out["N = 0 for one library"] = one_empty
    for name, b, c in (("one bin", 400, 1234), ("all above", BINS - 1, 1000), ("all below", 0, 2**51 - 1)):
        h = np.zeros((nlibs, BINS), np.uint64)
        h[:, b] = c
        out[name] = h
    return out


def as_array(rows):
    from breakdancer_amd import _lib
    return M.rows_array(rows, _lib.INSERT_SHIFT_DTYPE)


def assert_rows(got, exp, what):
    for k in ("n", "n_over", "saturated", "pad", "sum", "t_plus", "t_minus"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg="%s: %s" % (what, k))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. both routes against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["one", "three"])
def test_rows_equal_the_restatement_on_both_routes(label):
    from breakdancer_amd import _lib
    run, soa = case(label)
    iv = windows_of(label)                                   # (the conditions on the inputs: before the GPU is used)
    assert run.nlibs == (1 if label == "one" else 3) and len(soa["tid"]) > 20_000 and sorted(set(soa["tid"].tolist())) == [0, 1, 3]
    bd = product_from_oracle(run)
    cls = bd.read_class()
    np.testing.assert_array_equal(cls & 0x3F, run.cls)       # (what K1 wrote is what the restatement reads)
    own, _ = bd.insert_size_histogram()
    assert (own.sum(axis=1) > 100).all()
    arr = np.array(iv, dtype=_lib.INTERVAL_DTYPE)
    rng = np.random.default_rng(3)
    seen_full = {"all above": False, "all below": False}
    for name, hist in nulls_of(label, own).items():
        exp = as_array(M.expected_rows(soa, cls, run.nlibs, iv, hist))
        live = (exp["n"] > 0) & (exp["saturated"] == 0)
        N = hist.sum(axis=1).astype(np.int64)[None, :]
        if name == "own":
            assert exp["saturated"].any() and (exp["n_over"] > 0).any() and (exp["t_plus"] > 0).any() and (exp["t_minus"] > 0).any()
            assert (exp["saturated"].max(axis=1) == exp["saturated"].min(axis=1)).all()       # every row of a saturated window says so
        if name == "N = 0 for one library":
            assert (exp["n"][:, -1] > 0).any() and not exp["t_plus"][:, -1].any() and not exp["t_minus"][:, -1].any()
        if name == "all above":     # every observation below BINS - 1 lies below the null: t_plus = n N
            seen_full[name] = bool((live & (exp["t_plus"] == exp["n"].astype(np.int64) * N)).any())
        if name == "all below":     # x >= 1 everywhere: t_minus = n N
            seen_full[name] = bool((live & (exp["t_minus"] == exp["n"].astype(np.int64) * N)).any())
        bd.set_insert_null(hist)
        for staged in (0, 1):
            bd.set_debug("mini_staged", staged)
            what = "%s null=%s mini_staged=%d" % (label, name, staged)
            got = bd.window_insert_shift(arr)
            assert got.shape == (len(iv), run.nlibs) and got.dtype == _lib.INSERT_SHIFT_DTYPE
            assert_rows(got, exp, what)
            order = rng.permutation(len(iv))
            assert_rows(bd.window_insert_shift(arr[order]), exp[order], what + " permuted")
            for nq in (1, 4, 5):                             # one block with idle waves, a full one, and one wave into the second
                assert_rows(bd.window_insert_shift(arr[order[:nq]]), exp[order[:nq]], what + " nq=%d" % nq)
    assert all(seen_full.values()), seen_full
    bd.set_debug("mini_staged", 0)
    # more windows than the persistent grid has waves: every wave takes several
    many = np.array([(0, 1000 + 37 * k, 1000 + 37 * k + 400) for k in range(3000)], dtype=_lib.INTERVAL_DTYPE)
    bd.set_insert_null(own)
    assert_rows(bd.window_insert_shift(many), as_array(M.expected_rows(soa, cls, run.nlibs, many.tolist(), own)), "grid-stride")
    assert bd.window_insert_shift([]).shape == (0, run.nlibs)
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. state and argument errors; the null is replaced and freed
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_calls_and_the_null_in_between():
    import ctypes as C
    import breakdancer_amd as bda
    from breakdancer_amd import _lib
    from breakdancer_amd.api import LibraryConfig
    from runner import product_options
    run, soa = case("one")
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = np.array([(0, 1000, 3000)], dtype=_lib.INTERVAL_DTYPE)
    out = np.zeros(4, dtype=_lib.INSERT_SHIFT_DTYPE)
    call, setn = lib.bdx_window_insert_shift, lib.bdx_set_insert_null
    hist = np.zeros((1, BINS), np.uint64)
    hist[0, 380:420] = 50
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]))
            for i in range(run.nlibs)]
    fresh = bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0)
    assert setn(fresh.h, p(hist)) == 0                           # a null may be set before a run ...
    assert call(fresh.h, p(good), 1, p(out)) == 4                # ... but BDX_ESTATE: no run yet, ahead of every other check
    assert call(fresh.h, None, 1, None) == 4 and call(fresh.h, None, 0, None) == 4
    fresh.close()
    assert call(None, p(good), 1, p(out)) == 1 and setn(None, p(hist)) == 1      # no context
    bd = product_from_oracle(run)
    assert call(bd.h, p(good), 1, p(out)) == 4                   # BDX_ESTATE: no null set
    assert call(bd.h, None, 0, None) == 4
    assert setn(bd.h, p(hist)) == 0
    assert call(bd.h, p(good), 1, p(out)) == 0 and out[0]["n"] > 0
    assert call(bd.h, None, 0, None) == 0                        # n == 0, null pointers
    assert call(bd.h, None, 1, p(out)) == 1 and call(bd.h, p(good), 1, None) == 1      # BDX_EINVAL: a null array
    for bad in ((-1, 0, 10), (0, -1, 10), (0, 10, 9), (-2**31, 0, 0), (0, IMAX, 0)):
        a = np.array([good[0].tolist(), bad], dtype=_lib.INTERVAL_DTYPE)
        assert call(bd.h, p(a), 2, p(out)) == 1, bad
    for fine in ((0, 10, 10), (0, IMAX, IMAX), (IMAX, 0, IMAX)):
        assert call(bd.h, p(np.array([fine], dtype=_lib.INTERVAL_DTYPE)), 1, p(out)) == 0, fine
    assert call(bd.h, p(good), 2**31 + 1, p(out)) == 5           # BDX_ELIMIT
    big = hist.copy()
    big[0, 7] = 2**51
    assert setn(bd.h, p(big)) == 5                               # BDX_ELIMIT: N >= 2^51 ...
    big[0, 7] = 2**51 - 1 - int(hist.sum())
    assert setn(bd.h, p(big)) == 0 and setn(bd.h, p(hist)) == 0  # ... and N = 2^51 - 1 is taken
    # replacing the null changes the answer accordingly
    iv = [(0, 1000, 1400), (0, 2000, 9000), (1, 0, IMAX)]
    first = bd.window_insert_shift(iv)
    other = np.zeros((1, BINS), np.uint64)
    other[0, 300:500] = np.arange(200, dtype=np.uint64) + 1
    bd.set_insert_null(other)
    second = bd.window_insert_shift(iv)
    assert_rows(first, as_array(M.expected_rows(soa, run.cls, 1, iv, hist)), "first null")
    assert_rows(second, as_array(M.expected_rows(soa, run.cls, 1, iv, other)), "second null")
    assert (first["t_plus"] != second["t_plus"]).any() and (first["n"] == second["n"]).all()
    bd.set_insert_null(None)                                     # freed: BDX_ESTATE again
    assert call(bd.h, p(good), 1, p(out)) == 4
    bd.set_insert_null(hist)
    bd.run()                                                     # a second run, then a second call: the same answer
    assert_rows(bd.window_insert_shift(iv), first, "after a second run")
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. two ranks on one GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rank_contexts_give_the_single_context_rows():
    from breakdancer_amd import _lib
    from breakdancer_amd.shard import plan_chromosomes
    run, soa = case("three")
    iv = [w for w in windows_of("three") if w[0] in (0, 1, 3)]
    single = product_from_oracle(run)
    own, _ = single.insert_size_histogram()
    single.set_insert_null(own)
    want = single.window_insert_shift(iv)
    single.close()
    keep = []
    res = sharded_from_oracle(run, world=2, keep=keep)
    ranks = keep[0]._ranks
    hs = [r.insert_size_histogram()[0] for r in ranks]
    np.testing.assert_array_equal(sum(hs), own)                  # (the null of the sharded run: the ranks' histograms summed)
    counts = {int(t): int(c) for t, c in zip(*np.unique(soa["tid"], return_counts=True))}
    plan = plan_chromosomes(counts, 2)
    assert all(plan) and sorted(t for p in plan for t in p) == [0, 1, 3]
    arr = np.array(iv, dtype=_lib.INTERVAL_DTYPE)
    got = np.zeros_like(want)
    for r, tids in enumerate(plan):
        ranks[r].set_insert_null(own)
        mine = np.nonzero(np.isin(arr["tid"], tids))[0]
        assert len(mine)
        got[mine] = ranks[r].window_insert_shift(arr[mine])
        elsewhere = np.nonzero(~np.isin(arr["tid"], tids))[0][:5]         # a tid the rank holds nothing of: zero rows
        assert not ranks[r].window_insert_shift(arr[elsewhere]).view(np.uint8).any()
    assert_rows(got, want, "two ranks")
    assert (want["n"] > 0).any()
    del res


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def run_cli(args, cwd, cfg, env=None):
    p = subprocess.run([EXE] + args + [cfg], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env) if env else None, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode(), p.stderr.decode()


def table_of(path):
    text = open(path).read()
    head = [l for l in text.split("\n") if l.startswith("#") and not l.startswith("#Chr")]
    body = text[text.index("#Chr"):]
    return head, body, [l.split("\t") for l in body.rstrip("\n").split("\n")[1:]]


LENGTH, P, SEED = 200_000, 100_000, 1
PLANT_CFG = "readgroup:rg1\tplatform:illumina\tmap:%s\treadlen:50.00\tlib:lib1\tnum:10000\tlower:225.00\tupper:375.00\tmean:300.00\tstd:25.00\n"


def planted(change):
    """one library, one 200 kb sequence, a pair every 5 bp, inserts 300 +- 10 drawn once from SEED, reads of 50; every pair that starts in
    [P - 250, P - 50) has its insert changed by `change`"""
    from breakdancer_amd.synth import splitmix64
    rng = np.random.default_rng(SEED)
    start = np.arange(1000, LENGTH - 1000, 5, dtype=np.int64)
    n = len(start)
    ins = np.rint(rng.normal(300.0, 10.0, n)).astype(np.int64)
    ins[(start >= P - 250) & (start < P - 50)] += change
    key = splitmix64(np.arange(n, dtype=np.uint64))
    pos = np.concatenate([start, start + ins - 50])
    order = np.argsort(pos, kind="stable")
    first = np.concatenate([np.ones(n, bool), np.zeros(n, bool)])[order]
    return dict(tid=np.zeros(2 * n, np.int32), pos=pos[order].astype(np.int32), mtid=np.zeros(2 * n, np.int32),
                mpos=np.concatenate([start + ins - 50, start])[order].astype(np.int32), isize=np.concatenate([ins, -ins])[order].astype(np.int32),
                flag=np.where(first, 0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80).astype(np.uint16), qlen=np.full(2 * n, 50, np.uint16),
                mapq=np.full(2 * n, 60, np.uint8), lib=np.zeros(2 * n, np.uint8), bam=np.zeros(2 * n, np.uint8), name_key=np.concatenate([key, key])[order])


def restated_windows(soa, window, step, length):
    """{(0, j): call} of the grid over one sequence of `length`, every pair passing as NORMAL_FR, against the store's own KH histogram"""
    import estimate_cases as ec
    cls = np.full(len(soa["tid"]), 0x10 | 6, np.uint8)
    hist, _ = ec.observations(soa, 1, [35])
    N, mu, _ = M.null_figures(hist)
    grid = [(0, j * step, min(j * step + window, length)) for j in range(M.grid(length, step))]
    rows = M.expected_rows(soa, cls, 1, grid, hist)
    return {(0, j): M.window_call(r, N, mu, 20) for j, r in enumerate(rows)}


@pytest.mark.parametrize("change,kind", [(60, "DEL"), (-40, "INS"), (0, None)])
def test_cli_finds_the_planted_shift_and_nothing_else(change, kind, tmp_path):
    from breakdancer_amd.bamwrite import write_bam
    soa = planted(change)
    # the conditions, checked on the CPU with the restatement before the GPU run (over the sequence's first 200 kb: nothing lies beyond)
    calls = restated_windows(soa, 300, 150, LENGTH)
    W = sum(c is not None for c in calls.values())
    thr = M.default_threshold(W)
    hit = [j for (_, j), c in calls.items() if c is not None and j * 150 <= P < j * 150 + 300]
    best = max(calls[(0, j)]["score"] for j in hit)
    rest = max(c["score"] for (_, j), c in calls.items() if c is not None and not (P - 250 - 300 < j * 150 < P - 50))
    assert W > 1000 and rest < thr - 10, (rest, thr)
    if kind:
        assert best > thr + 100, (best, thr)
    write_bam(str(tmp_path / "p.bam"), soa, ["chrP"], seed=2)
    (tmp_path / "cfg").write_text(PLANT_CFG % "p.bam")
    out = str(tmp_path / "mini.txt")
    plain, _ = run_cli([], str(tmp_path), "cfg")
    stdout, err = run_cli(["--mini", out], str(tmp_path), "cfg", env=dict(BDX_TIMING="1"))
    assert filter_cmd_lines(stdout) == filter_cmd_lines(plain)
    assert len([l for l in err.split("\n") if l.startswith("[bdx timing] --mini:")]) == 1
    head, _, rows = table_of(out)
    assert "#Window: 300" in head and "#Step: 150" in head and "#MinPairs: 20" in head and any(l.startswith("#Threshold: ") for l in head)
    if kind is None:
        assert rows == []
        return
    assert len(rows) == 1, rows
    chrom, beg, end, typ, shift = rows[0][0], int(rows[0][1]), int(rows[0][2]), rows[0][3], float(rows[0][4])
    assert chrom == "chrP" and beg <= P <= end and typ == kind
    assert 20 <= abs(shift) <= abs(change) and (shift > 0) == (change > 0)
    if kind != "DEL":
        return
    # beside --estimate and --mark-dup: the null is taken behind the run, the default window from the estimated mean; still the one call
    # (the estimated cutoffs are tight around the true spread of 10, so the planted pairs are ARP_LARGE_INSERT now: observations all the same)
    both = str(tmp_path / "both.txt")
    run_cli(["--estimate", "--mark-dup", "--mini", both], str(tmp_path), "cfg")
    head, _, rows = table_of(both)
    assert len(rows) == 1 and rows[0][3] == "DEL" and int(rows[0][1]) <= P <= int(rows[0][2]) and 20 <= float(rows[0][4]) <= 60, rows
    assert any(l in ("#Window: 300", "#Window: 301") for l in head)
    # -t: no same-chromosome read passes; the table is empty, legally
    none = str(tmp_path / "t.txt")
    run_cli(["-t", "--mini", none], str(tmp_path), "cfg")
    assert table_of(none)[2] == []


def test_cli_on_the_golden_fixture_equals_the_check_tool(tmp_path):
    args = ["-o", "21", "--mini-window", "2000", "--mini-step", "1000"]
    f0, f1, out = str(tmp_path / "plain.vcf"), str(tmp_path / "mini.vcf"), str(tmp_path / "mini.txt")
    plain, _ = run_cli(["-o", "21", "--vcf", f0], CWD, "inv_del_bam_config")
    stdout, _ = run_cli(args + ["--vcf", f1, "--mini", out], CWD, "inv_del_bam_config")
    assert filter_cmd_lines(stdout) == filter_cmd_lines(plain)
    assert T.without_command(open(f1).read()) == T.without_command(open(f0).read())
    head, body, rows = table_of(out)
    length = [int(l[len("##contig=<ID=21,length="):-1]) for l in open(f0).read().split("\n") if l.startswith("##contig=<ID=21,")][0]
    # the rows, through api.py, of the same records
    run = load_chr21(make_opts(chr_tid=22)).run()
    bd = product_from_oracle(run)
    hist, _ = bd.insert_size_histogram()
    bd.set_insert_null(hist)
    nw = M.grid(length, 1000)
    got = bd.window_insert_shift([(22, j * 1000, min(j * 1000 + 2000, length)) for j in range(nw)])
    bd.close()
    assert (got["n"] > 0).any()
    N, mu, usable = M.null_figures(hist)
    assert any(usable)
    by_window = {j: [tuple(int(v) for v in got[j, L].tolist()) for L in range(run.nlibs)] for j in range(nw) if got[j].view(np.uint8).any()}
    (tmp_path / "rows.txt").write_text(M.rows_text(by_window))
    p = subprocess.run([CHECK, str(tmp_path / "rows.txt"), "--n", ",".join(str(v) for v in N), "--mu", ",".join(repr(float(v)) for v in mu), "--window", "2000",
                        "--step", "1000", "--contig", "21:%d" % length], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    text = p.stdout.decode()
    thr = [l.split("\t") for l in text.split("\n") if l.startswith("threshold\t")][0]
    assert "#Threshold: %s" % thr[1] in head and "#Window: 2000" in head and "#Step: 1000" in head and int(thr[3]) > 0
    assert body == text[text.index("#Chr"):]


def test_cli_sharded_equals_one_gpu(tmp_path):
    """two sequences with one planted shift each, on one GPU and on two and three ranks (each window answered by the rank that holds its
    sequence, the null summed over the ranks): the same file"""
    from breakdancer_amd.bamwrite import write_bam
    a, b = planted(60), planted(-40)
    b["tid"][:] = 1
    b["mtid"][:] = 1
    b["name_key"] = b["name_key"] ^ np.uint64(0x5555555555555555)
    soa = {k: np.concatenate([a[k], b[k]]) for k in a}
    write_bam(str(tmp_path / "p.bam"), soa, ["chrP", "chrQ"], seed=2, index=True)
    (tmp_path / "cfg").write_text(PLANT_CFG % "p.bam")
    one = str(tmp_path / "one.txt")
    table, _ = run_cli(["--mini", one], str(tmp_path), "cfg")
    _, body, rows = table_of(one)
    assert [(r[0], r[3]) for r in rows] == [("chrP", "DEL"), ("chrQ", "INS")] and all(int(r[1]) <= P <= int(r[2]) for r in rows)
    for gpus in ("0,0", "0,0,0"):
        f = str(tmp_path / ("ranks%d.txt" % len(gpus)))
        out, _ = run_cli(["--mini", f], str(tmp_path), "cfg", env=dict(BDX_GPUS=gpus))
        assert filter_cmd_lines(out) == filter_cmd_lines(table)
        assert table_of(f)[1] == body, gpus
    host = str(tmp_path / "host.txt")                            # BDX_DECODE=host: the same records are held
    run_cli(["--mini", host], str(tmp_path), "cfg", env=dict(BDX_DECODE="host"))
    assert table_of(host)[1] == body
