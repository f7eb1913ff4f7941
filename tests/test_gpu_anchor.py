"""GPU tests of --anchor: bdx_window_anchor_split (KA, csrc/ka_anchor.hip) against the numpy restatement of tests/anchor_cases.py, field by
field and exactly; its argument and state errors; two ranks on one GPU; and the command end to end on a small BAM with planted insertions
and on the chr21 golden fixture.

The stores come from test_gpu_sites.Store, with one-end-anchored records appended to Store.recs, through the oracle.  They are laid out by
record index: in the regions that are counted off, every record has a position of its own ten apart, so the windows are cut to hold exactly
0, 1, 63, 64, 65, 128 and 129 records -- the edges of the walk's 64-record steps.  Each test asserts from the restatement, before it uses
the GPU, that every class of window and record it means to submit is there."""
import os
import subprocess

import numpy as np
import pytest

import anchor_cases as A
import test_gpu_sites as T
from helpers import GOLDEN, ROOT, filter_cmd_lines, load_chr21, make_opts
from runner import oracle_case, product_from_oracle, sharded_from_oracle

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHECK = os.path.join(ROOT, "bin", "bdx-anchor-check")
CWD = os.path.join(GOLDEN, "chr21")
IMAX = 2**31 - 1
FAR = T.FAR
QUALS = (0, 20, 21, 35, 36, 60, 61, 255)         # on both sides of every minimum: 20, 35 (-q) and 60
MIXED = {"lib0": 20, "lib1": None, "lib2": 60}   # the three libraries' own mapqual:, lib1's left to -q
BETWEEN = 40                                     # a min_qual between the libraries' minima
A0, B0, C0, D0, E0, F0, F1, G0, H0 = 10_000, 20_000, 40_000, 60_000, 80_000, 100_000, 120_000, 140_000, 160_000
RUN_AT = 58                                      # regions B and C: the record index at which the run of equal positions begins


# ---------------------------------------------------------------------------------------------------------------------------------
# the store
# ---------------------------------------------------------------------------------------------------------------------------------
def mixed_config(libs):
    return "".join("readgroup:%s\tplatform:illumina\tmap:%s\treadlen:%d.00\tlib:%s\tlower:%.2f\tupper:%.2f\tmean:%.2f\tstd:%.2f%s\n"
                   % (rg, bam, T.RL, lib, mean - 3 * std, mean + 3 * std, mean, std, "" if MIXED[lib] is None else "\tmapqual:%d" % MIXED[lib])
                   for rg, bam, lib, mean, std in libs)


def anchor_store(libs, seed):
    rng = np.random.default_rng(seed)
    st = T.Store(libs)
    nl = len(libs)

    def rec(tid, pos, flag, qual, li=None):
        li = int(rng.integers(0, nl)) if li is None else li
        st.names += 1
        st.recs[st.bams.index(libs[li][1])].append(dict(tid=tid, pos=pos, mtid=tid, mpos=pos, isize=0, flag=flag, qlen=T.RL, bdqual=qual, rg=libs[li][0],
                                                        name=st.names))

    def anchor(tid, pos, rev, qual=255, extra=0, mate=False, li=None):
        """a mapped record whose mate is unmapped; mate=True: the unmapped mate's own record too, placed at the same position"""
        rec(tid, pos, 0x1 | 0x8 | 0x40 | (0x10 if rev else 0) | extra, qual, li)
        if mate:
            st.names -= 1
            rec(tid, pos, 0x1 | 0x4 | 0x80 | (0x20 if rev else 0), 0, li)

    def other(tid, pos, kind):
        if kind == "dup":
            anchor(tid, pos, bool(rng.integers(0, 2)), extra=0x400)
        elif kind == "unm":
            rec(tid, pos, 0x1 | 0x4 | 0x80, 0)
        elif kind == "low":
            anchor(tid, pos, bool(rng.integers(0, 2)), qual=0)
        else:                                         # a passing pair: its other mate far away on c3
            st.pair(int(rng.integers(0, nl)), tid, pos, 3, 500_000 + st.names, False, True, mapq=255, both=False)

    def mix(tid, base, n):
        """n records, one per position, ten apart: anchors of both directions and every quality, and records that are none"""
        for i in range(n):
            k = ("fwd", "rev", "fwd", "rev", "dup", "unm", "pair", "low")[int(rng.integers(0, 8))]
            if k in ("fwd", "rev"):
                anchor(tid, base + 10 * i, k == "rev", qual=QUALS[int(rng.integers(0, len(QUALS)))])
            else:
                other(tid, base + 10 * i, k)

    anchor(0, 5, False)                               # the store's first records
    anchor(0, 7, True)
    mix(0, A0, 400)
    # B: a run of equal positions of both directions across a step edge; C: the same with records inside it that are no anchors
    for base, inside in ((B0, False), (C0, True)):
        mix(1, base, RUN_AT)
        at = base + 10 * RUN_AT
        for k in range(12):
            if inside and k in (1, 5, 7, 10):
                other(1, at, ("pair", "unm", "dup", "low")[(1, 5, 7, 10).index(k)])
            else:
                anchor(1, at, rev=k % 2 == 1 if k < 6 else k % 3 == 0)
        mix(1, at + 10, 40)
    for i in range(70):                               # D: only right-pointing, two at every start; E: only left-pointing
        anchor(1, D0 + 10 * (i // 2), False)
        anchor(1, E0 + 10 * (i // 2), True)
    for i in range(66):                               # F0: alternating, a right-pointing one first; F1: a left-pointing one first
        anchor(1, F0 + 10 * i, i % 2 == 1)
        anchor(1, F1 + 10 * i, i % 2 == 0)
    for base, sizes in ((G0, (5, 8)), (H0, (6, 6))):  # two separated clusters in one window: the second better, and a tie
        for c, n in enumerate(sizes):
            for i in range(n):
                anchor(1, base + 3000 * c + 10 * i, False, mate=True)
                anchor(1, base + 3000 * c + 200 + 10 * i, True, mate=True)
        other(1, base, "pair")                        # a passing pair, an unmapped record and a duplicate AT an anchor's position
        other(1, base + 200, "unm")
        other(1, base + 3000, "dup")
    for i in range(5):                                # near 2^31, and the store's last record
        anchor(3, FAR + 10 * i, False)
        anchor(3, FAR + 100 + 10 * i, True)
    return st


LABELS = ["one", "three", "three/l"]
STORES = {}


def case(label):
    """(oracle run, merged stream, the libraries' resolved minima) of a labelled store: built and run through the oracle once"""
    if label not in STORES:
        libs = T.ONE_LIB if label == "one" else T.THREE_LIBS
        cfg = T.config_text(libs) if label == "one" else mixed_config(libs)
        run = oracle_case(cfg, anchor_store(libs, 5 + len(label)).streams(), T.TARGETS, make_opts(illumina_long_insert=int(label.endswith("/l"))))
        minima = np.array([int(run.lib_i[i, 0]) if int(run.lib_i[i, 0]) >= 0 else int(run.opts["min_map_qual"]) for i in range(run.nlibs)], np.int64)
        STORES[label] = (run, run.merged_soa(), minima)
    return STORES[label]


def windows_of(label):
    """the windows of a store, and the assertion that every class of window and record is among them"""
    run, soa, minima = case(label)
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    flag = soa["flag"].astype(np.int64)
    records = lambda w: int(((t == w[0]) & (s >= w[1]) & (s < w[2])).sum())
    iv = [(0, 5000, 5000), (0, 0, 0), (0, IMAX, IMAX), (2, 0, IMAX), (2, 100, 5000), (4, 0, IMAX), (1000, 0, IMAX), (IMAX, 0, IMAX),
          (0, 0, IMAX), (1, 0, IMAX), (3, 0, IMAX),
          (0, 5, 8), (0, 0, 6), (0, 5, 6), (0, 6, 8), (0, 0, 5),                                   # the store's first records as window edges
          (3, FAR, IMAX), (3, FAR - 5, FAR + 200), (3, FAR + 140, FAR + 141), (3, FAR + 140, IMAX), (3, FAR + 141, IMAX), (3, IMAX - 1, IMAX), (3, FAR + 50, IMAX)]   # .. and its last
    exact = {}
    for a in (3, 101):
        for k in (0, 1, 63, 64, 65, 128, 129):
            w = (0, A0 + 10 * a + 1, A0 + 10 * (a + 1)) if k == 0 else (0, A0 + 10 * a, A0 + 10 * (a + k))
            iv.append(w)
            exact[w] = k
    runs = []
    for base in (B0, C0):
        for a in range(6):                          # the run at window records RUN_AT - a .. RUN_AT - a + 11: across record 64
            w = (1, base + 10 * a, base + 10 * 110)
            iv.append(w)
            runs.append((w, base + 10 * RUN_AT, RUN_AT - a))
        iv += [(1, base + 10 * RUN_AT, base + 10 * RUN_AT + 1), (1, base, base + 10 * RUN_AT + 1), (1, base + 10 * RUN_AT, base + 2000)]
    only = {}
    for base in (D0, E0):
        only[base] = [(1, base, base + 10 * 35), (1, base - 100, base + 2000), (1, base + 10 * 3, base + 10 * 20)]
        iv += only[base]
    alt = {base: [(1, base, base + 660), (1, base - 50, base + 1000), (1, base + 10, base + 10 * 65)] for base in (F0, F1)}
    iv += alt[F0] + alt[F1]
    two = {base: [(1, base, base + 4000), (1, base - 500, base + 10_000)] for base in (G0, H0)}
    iv += two[G0] + two[H0] + [(1, G0, G0 + 500), (1, G0 + 3000, G0 + 3500), (1, G0 + 100, G0 + 3100)]
    order = np.random.default_rng(5).permutation(len(iv))
    iv = [iv[i] for i in order]                     # unsorted, and overlapping anyway
    # ---- what is there ----
    assert all(records(w) == k for w, k in exact.items()) and set(exact.values()) == {0, 1, 63, 64, 65, 128, 129}
    li = run.opts["illumina_long_insert"]
    right, left, low = A.record_kinds(soa, run.cls, minima, -1, li)
    for w, at, first in runs:                       # the run: 12 records at one position, from window record `first` on, across record 64
        idx = np.nonzero((t == w[0]) & (s >= w[1]) & (s < w[2]))[0]
        run_idx = np.nonzero(s[idx] == at)[0]
        assert run_idx.tolist() == list(range(first, first + 12)) and first < 64 <= first + 11
        here = idx[run_idx]
        assert right[here].any() and left[here].any()
        assert (~(right | left)[here]).any() == (at > C0)       # C's run holds records that are no anchors, B's does not
    inside = np.zeros(len(t), bool)
    for tid, beg, end in iv:
        inside |= (t == tid) & (s >= beg) & (s < end)
    cand = run.cls == 9
    anchor_pos = set(zip(t[right | left].tolist(), s[right | left].tolist()))
    at_anchor = np.array([(a, b) in anchor_pos for a, b in zip(t.tolist(), s.tolist())])
    has = {
        "anchors of both directions": (inside & right).any() and (inside & left).any(),
        "a candidate that fails quality": (inside & low).any(),
        "0x400 on a mate-unmapped record, which is no candidate": (inside & ~cand & ((flag & 0x408) == 0x408)).any(),
        "an unmapped record (0x4)": (inside & ~cand & ((flag & 0x4) != 0)).any(),
        "a passing pair at an anchor's position": (inside & at_anchor & ((run.cls & 0x10) != 0)).any(),
        "an unmapped record at an anchor's position": (inside & at_anchor & ((flag & 0x4) != 0)).any(),
        "a duplicate at an anchor's position": (inside & at_anchor & ((flag & 0x400) != 0)).any(),
        "every quality": set(soa["bdqual"][cand].tolist()) >= set(QUALS),
        "the store's first and last record are anchors": bool((right | left)[0] and (right | left)[-1]),
        "a sequence without reads": not (t == 2).any(),
    }
    assert all(has.values()), [k for k, v in has.items() if not v]
    assert (cand & ((flag & 0x40D) != 0x9)).sum() == 0 and ((flag & 0x40D) == 0x9).sum() == cand.sum()      # class 9 is what the rule says it is
    if run.nlibs == 3:
        assert sorted(minima.tolist()) == [20, 35, 60] and all((cand & (soa["lib"] == l)).any() for l in range(3))
    return iv, dict(only=only, alt=alt, two=two)


def assert_shapes(label, iv, marked, rows):
    """what the restatement's rows must show for the windows written to show it (min_qual = -1)"""
    run = case(label)[0]
    by = dict(zip(iv, rows))
    assert any(any(r[k] for k in A.FIELDS if k not in ("split", "last_left", "first_right")) for r in rows)          # not all zero
    flip = bool(run.opts["illumina_long_insert"])
    for w in marked["only"][D0 if not flip else E0]:
        assert by[w]["n_fwd"] > 0 and by[w]["n_rev"] == 0 and by[w]["n_left"] == by[w]["n_fwd"] and by[w]["u_left"] * 2 >= by[w]["n_left"] > by[w]["u_left"]
        assert by[w]["split"] == by[w]["last_left"] + 1 and by[w]["first_right"] == -1
    for w in marked["only"][E0 if not flip else D0]:
        assert by[w]["n_rev"] > 0 and by[w]["n_fwd"] == 0 and by[w]["n_right"] == by[w]["n_rev"] and by[w]["split"] == w[1] and by[w]["last_left"] == -1
    lead_right, lead_left = (F0, F1) if not flip else (F1, F0)
    w = marked["alt"][lead_right][0]                # right, left, right, ..: n / 2 + 1 ... at the first anchor already
    assert by[w]["n_left"] == 1 and by[w]["split"] == w[1] + 1 and by[w]["n_right"] == by[w]["n_rev"] == 33
    w = marked["alt"][lead_left][0]                 # left, right, left, ..: no S beats beg
    assert by[w]["n_left"] == 0 and by[w]["split"] == w[1] and by[w]["n_right"] == by[w]["n_rev"] == 33
    if not flip:
        g, h = by[marked["two"][G0][0]], by[marked["two"][H0][0]]
        assert (g["n_left"], g["n_right"], g["last_left"], g["first_right"]) == (13, 8, G0 + 3000 + 70, G0 + 3200)     # the second cluster's split
        assert (h["n_left"], h["n_right"], h["last_left"], h["first_right"]) == (6, 12, H0 + 50, H0 + 200)             # a tie: the first cluster's
    assert sum(r["n_low"] > 0 for r in rows) > 5 and any(r["u_left"] < r["n_left"] for r in rows) and any(r["u_right"] < r["n_right"] for r in rows)
    for w in ((0, 5000, 5000), (2, 0, IMAX), (4, 0, IMAX), (IMAX, 0, IMAX)):
        assert by[w] == dict({k: 0 for k in A.FIELDS}, split=w[1], last_left=-1, first_right=-1)
    far = by[(3, FAR, IMAX)]
    assert (far["n_left"], far["n_right"], far["split"], far["first_right"]) == ((5, 5, FAR + 41, FAR + 100) if not flip else (0, 5, FAR, FAR))
    assert by[(3, FAR + 140, FAR + 141)]["n_fwd"] + by[(3, FAR + 140, FAR + 141)]["n_rev"] == 1
    assert all(r["split"] == (r["last_left"] + 1 if r["n_left"] else w[1]) for w, r in by.items())


def as_array(rows):
    from breakdancer_amd import _lib
    return A.rows_array(rows, _lib.ANCHOR_SPLIT_DTYPE)


def assert_rows(got, exp, what):
    for k in A.FIELDS:
        np.testing.assert_array_equal(got[k], exp[k], err_msg="%s: %s" % (what, k))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. KA against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_rows_equal_the_restatement(label):
    from breakdancer_amd import _lib
    run, soa, minima = case(label)
    iv, marked = windows_of(label)                  # (the conditions on the inputs: before the GPU is used)
    li = bool(run.opts["illumina_long_insert"])
    expected = {q: A.expected_rows(soa, run.cls, minima, iv, q, li) for q in (-1, 0, BETWEEN, 255)}
    assert_shapes(label, iv, marked, expected[-1])
    assert run.nlibs == (1 if label == "one" else 3) and li == label.endswith("/l")
    differ = lambda a, b: any(x != y for x, y in zip(expected[a], expected[b]))
    assert differ(-1, 0) and differ(0, BETWEEN) and differ(BETWEEN, 255) and differ(-1, BETWEEN)
    assert all(r["n_low"] == 0 for r in expected[0])
    bd = product_from_oracle(run)
    cls = bd.read_class()
    np.testing.assert_array_equal(cls & 0x3F, run.cls)            # (what K1 wrote is what the restatement reads,
    assert (cls[run.cls == 9] == 9).all()                         #  and a candidate's byte is 9 as a whole)
    arr = np.array(iv, dtype=_lib.INTERVAL_DTYPE)
    rng = np.random.default_rng(3)
    for q, rows in expected.items():
        exp = as_array(rows)
        what = "%s min_qual=%d" % (label, q)
        got = bd.window_anchor_split(arr, q)
        assert got.shape == (len(iv),) and got.dtype == _lib.ANCHOR_SPLIT_DTYPE
        assert_rows(got, exp, what)
        order = rng.permutation(len(iv))
        assert_rows(bd.window_anchor_split(arr[order], q), exp[order], what + " permuted")
        for nq in (1, 4, 5):                        # one block with idle waves, a full one, and one wave into the second
            assert_rows(bd.window_anchor_split(arr[order[:nq]], q), exp[order[:nq]], what + " nq=%d" % nq)
    # more windows than the persistent grid has waves: every wave takes several
    many = [(k % 2, 9000 + 23 * (k // 2), 9000 + 23 * (k // 2) + 700) for k in range(9000)]
    assert_rows(bd.window_anchor_split(many), as_array(A.expected_rows(soa, run.cls, minima, many, -1, li)), "grid-stride")
    assert bd.window_anchor_split([]).shape == (0,)
    bd.close()


def test_equal_positions_give_the_same_row_in_any_store_order():
    """the records of every position of the store dealt out anew: the rule speaks of positions"""
    from breakdancer_amd import _lib
    run, soa, minima = case("one")
    iv, _ = windows_of("one")
    want = as_array(A.expected_rows(soa, run.cls, minima, iv))
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    rng = np.random.default_rng(11)
    order = np.lexsort((rng.random(len(t)), s, t))
    assert (order != np.arange(len(t))).sum() > 20 and (t[order] == t).all() and (s[order] == s).all()
    shuffled = {k: v[order] for k, v in soa.items()}
    assert_rows(as_array(A.expected_rows(shuffled, run.cls[order], minima, iv)), want, "the restatement, shuffled")
    import breakdancer_amd as bda
    from breakdancer_amd.api import LibraryConfig
    from runner import product_options
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]))
            for i in range(run.nlibs)]
    bd = bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0)
    bd.push_reads(shuffled)
    bd.run()
    np.testing.assert_array_equal(bd.read_class() & 0x3F, run.cls[order])
    assert_rows(bd.window_anchor_split(np.array(iv, dtype=_lib.INTERVAL_DTYPE)), want, "shuffled store")
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. state and argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_calls():
    import ctypes as C
    import breakdancer_amd as bda
    from breakdancer_amd import _lib
    from breakdancer_amd.api import LibraryConfig
    from runner import product_options
    run, soa, minima = case("one")
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = np.array([(1, D0, D0 + 500)], dtype=_lib.INTERVAL_DTYPE)
    out = np.zeros(4, dtype=_lib.ANCHOR_SPLIT_DTYPE)
    call = lib.bdx_window_anchor_split
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]))
            for i in range(run.nlibs)]
    fresh = bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0)
    assert call(fresh.h, p(good), 1, -1, p(out)) == 4            # BDX_ESTATE: no run yet, ahead of every other check
    assert call(fresh.h, None, 1, -1, None) == 4 and call(fresh.h, None, 0, -7, None) == 4
    fresh.close()
    assert call(None, p(good), 1, -1, p(out)) == 1               # no context
    bd = product_from_oracle(run)
    assert call(bd.h, p(good), 1, -1, p(out)) == 0 and out[0]["n_fwd"] > 0
    assert call(bd.h, None, 0, -1, None) == 0                    # n == 0, null pointers
    assert call(bd.h, None, 1, -1, p(out)) == 1 and call(bd.h, p(good), 1, -1, None) == 1      # BDX_EINVAL: a null array
    for q in (-2, 256, -2**31, IMAX):
        assert call(bd.h, p(good), 1, q, p(out)) == 1, q         # BDX_EINVAL: min_qual outside -1 .. 255
    for q in (-1, 0, 255):
        assert call(bd.h, p(good), 1, q, p(out)) == 0, q
    for bad in ((-1, 0, 10), (0, -1, 10), (0, 10, 9), (-2**31, 0, 0), (0, IMAX, 0)):
        a = np.array([good[0].tolist(), bad], dtype=_lib.INTERVAL_DTYPE)
        assert call(bd.h, p(a), 2, -1, p(out)) == 1, bad
    for fine in ((0, 10, 10), (0, IMAX, IMAX), (IMAX, 0, IMAX)):
        assert call(bd.h, p(np.array([fine], dtype=_lib.INTERVAL_DTYPE)), 1, -1, p(out)) == 0, fine
        assert out[0]["split"] == fine[1] and out[0]["last_left"] == -1 and out[0]["first_right"] == -1 and out[0]["n_fwd"] == 0
    assert call(bd.h, p(good), 2**31 + 1, -1, p(out)) == 5       # BDX_ELIMIT
    iv = [(1, D0, D0 + 500), (1, G0, G0 + 4000), (0, 0, IMAX)]
    first = bd.window_anchor_split(iv)
    bd.run()                                                     # a second run, then a second call: the same answer
    assert_rows(bd.window_anchor_split(iv), first, "after a second run")
    assert_rows(first, as_array(A.expected_rows(soa, run.cls, minima, iv)), "the three windows")
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. two ranks on one GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rank_contexts_give_the_single_context_rows():
    from breakdancer_amd import _lib
    from breakdancer_amd.shard import plan_chromosomes
    run, soa, minima = case("three")
    iv = [w for w in windows_of("three")[0] if w[0] in (0, 1, 3)]
    want = as_array(A.expected_rows(soa, run.cls, minima, iv, BETWEEN))
    assert (want["n_left"] > 0).any() and (want["n_low"] > 0).any()
    keep = []
    res = sharded_from_oracle(run, world=2, keep=keep)
    ranks = keep[0]._ranks
    counts = {int(t): int(c) for t, c in zip(*np.unique(soa["tid"], return_counts=True))}
    plan = plan_chromosomes(counts, 2)
    assert all(plan) and sorted(t for p in plan for t in p) == [0, 1, 3]
    arr = np.array(iv, dtype=_lib.INTERVAL_DTYPE)
    got = np.zeros_like(want)
    for r, tids in enumerate(plan):
        mine = np.nonzero(np.isin(arr["tid"], tids))[0]
        assert len(mine)
        got[mine] = ranks[r].window_anchor_split(arr[mine], BETWEEN)
        elsewhere = np.nonzero(~np.isin(arr["tid"], tids))[0]           # a tid the rank holds nothing of: empty rows
        empty = ranks[r].window_anchor_split(arr[elsewhere])
        assert not any(empty[k].any() for k in A.FIELDS[:7]) and (empty["split"] == arr[elsewhere]["beg"]).all() and (empty["last_left"] == -1).all()
    assert_rows(got, want, "two ranks")
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


def restated_table(soa, cls, minima, names, lengths, window, step, minimum, min_qual):
    """the file's table by the restatement: only the grid windows that hold a candidate are looked at, all others give empty rows"""
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    grid = set()
    for tid, p in zip(t[cls == 9].tolist(), s[cls == 9].tolist()):
        grid |= {(tid, j) for j in range(max(0, (p - window) // step + 1), p // step + 1)}
    grid = sorted(grid)
    assert all(j < A.grid(lengths[tid], step) for tid, j in grid)
    iv = [(tid, j * step, min(j * step + window, lengths[tid])) for tid, j in grid]
    rows = A.expected_rows(soa, cls, minima, iv, min_qual)
    return A.table_of_rows([(tid, r) for (tid, _), r in zip(grid, rows)], minimum, names), rows


PLANT_CFG = "readgroup:rg1\tplatform:illumina\tmap:%s\treadlen:50.00\tlib:lib1\tnum:10000\tlower:225.00\tupper:375.00\tmean:300.00\tstd:25.00\n"
SITE_P, SITE_Q, ONE_SIDED, DUPLICATES = 10_000, 20_000, 25_000, 30_000


def planted_records():
    """two sequences of normal pairs; on chrP an insertion at SITE_P (8 anchors with distinct starts either side) and a one-sided pile at
    ONE_SIDED; on chrQ an insertion at SITE_Q (5 + 6, one start doubled) and a pile of duplicates, every anchor at one start, at DUPLICATES"""
    rng = np.random.default_rng(4)
    recs, n = [], [0]

    def add(tid, pos, flag, mtid, mpos, isize, mapq=60):
        recs.append(dict(tid=tid, pos=pos, mtid=mtid, mpos=mpos, isize=isize, flag=flag, qlen=50, mapq=mapq, name="r%06d" % n[0], rg="rg1"))

    def anchor(tid, pos, rev, mapq=60):
        n[0] += 1
        add(tid, pos, 0x1 | 0x8 | 0x40 | (0x10 if rev else 0), tid, pos, 0, mapq)
        add(tid, pos, 0x1 | 0x4 | 0x80 | (0x20 if rev else 0), tid, pos, 0, 0)

    for tid in (0, 1):
        for start in range(1000, 40_000, 40):
            n[0] += 1
            ins = int(round(rng.normal(300.0, 10.0)))
            add(tid, start, 0x1 | 0x2 | 0x20 | 0x40, tid, start + ins - 50, ins)
            add(tid, start + ins - 50, 0x1 | 0x2 | 0x10 | 0x80, tid, start, -ins)
    for i in range(8):
        anchor(0, SITE_P - 170 + 20 * i, False)
        anchor(0, SITE_P + 10 + 20 * i, True)
    anchor(0, SITE_P - 100, False, mapq=0)                  # a candidate of low quality beside them
    for i in range(6):
        anchor(0, ONE_SIDED - 200 + 30 * i, False)
    for i in range(5):
        anchor(1, SITE_Q - 250 + 50 * (i if i < 4 else 3), False)
    for i in range(6):
        anchor(1, SITE_Q + 20 + 40 * i, True)
    for i in range(5):
        anchor(1, DUPLICATES - 100, False)
        anchor(1, DUPLICATES + 100, True)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs


def test_cli_finds_the_planted_insertions_and_nothing_else(tmp_path):
    from breakdancer_amd.bamwrite import write_bam_records
    recs = planted_records()
    names, lengths = ["chrP", "chrQ"], [300000000, 300000000]
    soa = dict(tid=np.array([r["tid"] for r in recs]), pos=np.array([r["pos"] for r in recs]), flag=np.array([r["flag"] for r in recs]),
               bdqual=np.array([r["mapq"] for r in recs]), lib=np.zeros(len(recs), np.int64))
    cls = np.where((soa["flag"] & 0x40D) == 0x9, 9, 0)      # (the classifier's rule for class 9; the other bytes do not matter to the rule)
    window, step = A.default_window([375.0]), A.default_step(A.default_window([375.0]))
    assert (window, step) == (750, 375)
    want, rows = restated_table(soa, cls, [35], names, lengths, window, step, 3, -1)
    body = [l.split("\t") for l in want.rstrip("\n").split("\n")[1:]]
    assert [(b[0], int(b[1]), int(b[2]), b[3]) for b in body] == [("chrP", SITE_P - 170 + 20 * 7 + 1, SITE_P + 10 + 1, "INS"), ("chrQ", SITE_Q - 100 + 1, SITE_Q + 20 + 1, "INS")]
    assert [(int(b[4]), int(b[5]), int(b[6]), int(b[7])) for b in body] == [(8, 8, 8, 8), (5, 6, 4, 6)] and int(body[0][9]) >= 2
    assert any(r["n_left"] >= 5 and r["n_right"] >= 5 and r["u_left"] == 1 and r["u_right"] == 1 for r in rows)       # the pile of duplicates
    assert any(r["u_left"] >= 6 and r["n_right"] == 0 for r in rows) and any(r["n_low"] for r in rows)               # the one-sided pile
    write_bam_records(str(tmp_path / "p.bam"), recs, names, rgs=("rg1",), seed=2, index=True)
    (tmp_path / "cfg").write_text(PLANT_CFG % "p.bam")
    f0, f1, out = str(tmp_path / "plain.vcf"), str(tmp_path / "anchor.vcf"), str(tmp_path / "anchor.txt")
    plain, _ = run_cli(["--vcf", f0], str(tmp_path), "cfg")
    stdout, err = run_cli(["--vcf", f1, "--anchor", out], str(tmp_path), "cfg", env=dict(BDX_TIMING="1"))
    assert filter_cmd_lines(stdout) == filter_cmd_lines(plain)
    assert T.without_command(open(f1).read()) == T.without_command(open(f0).read())
    timing = [l for l in err.split("\n") if l.startswith("[bdx timing] --anchor:")]
    assert len(timing) == 1 and " %d candidates, %d anchors, 2 calls;" % (int((cls == 9).sum()), int((cls == 9).sum()) - 1) in timing[0], timing
    assert "WARNING: --anchor" not in err
    head, got, _ = table_of(out)
    assert got == want
    assert "#Window: 750" in head and "#Step: 375" in head and "#Min: 3" in head and "#Mapq: -1" in head and any(l.startswith("#Command: ") for l in head)
    # the same file through the host decode, on two ranks, beside --mini, --mark-dup and -t (the rule does not ask whether a record passes)
    for k, (args, env) in enumerate([([], dict(BDX_DECODE="host")), ([], dict(BDX_GPUS="0,0")), (["--mini", str(tmp_path / "mini.txt")], None),
                                     (["--mark-dup"], None), (["-t"], None), (["-a"], None)]):
        f = str(tmp_path / ("again%d.txt" % k))
        text, _ = run_cli(args + ["--anchor", f], str(tmp_path), "cfg", env=env)
        assert table_of(f)[1] == want, (args, env)
        if not args:
            assert filter_cmd_lines(text) == filter_cmd_lines(plain)
    # other options: a step that does not divide the window leaves the sums out of the timing line; a larger --anchor-min drops chrQ's call
    f = str(tmp_path / "opts.txt")
    _, err = run_cli(["--anchor", f, "--anchor-window", "1000", "--anchor-step", "300", "--anchor-min", "5", "--anchor-mapq", "0"], str(tmp_path), "cfg",
                     env=dict(BDX_TIMING="1"))
    want5, _ = restated_table(soa, cls, [35], names, lengths, 1000, 300, 5, 0)
    head, got, rows5 = table_of(f)
    assert got == want5 and [r[0] for r in rows5] == ["chrP"] and int(rows5[0][8]) == 0
    assert "#Window: 1000" in head and "#Step: 300" in head and "#Min: 5" in head and "#Mapq: 0" in head
    timing = [l for l in err.split("\n") if l.startswith("[bdx timing] --anchor:")]
    assert len(timing) == 1 and "candidates" not in timing[0] and " 1 calls;" in timing[0]


def chr21_length(vcf_text):
    return [int(l[len("##contig=<ID=21,length="):-1]) for l in vcf_text.split("\n") if l.startswith("##contig=<ID=21,")][0]


def test_cli_on_the_golden_fixture_warns_about_am_and_calls_with_mapq_0(tmp_path):
    run = load_chr21(make_opts(chr_tid=22)).run()
    soa = run.merged_soa()
    cand = run.cls == 9
    assert cand.sum() == 7 and not soa["bdqual"][cand].any()             # the fixture's candidates all carry AM = 0
    f0, f1, out = str(tmp_path / "plain.vcf"), str(tmp_path / "anchor.vcf"), str(tmp_path / "anchor.txt")
    plain, _ = run_cli(["-o", "21", "--vcf", f0], CWD, "inv_del_bam_config")
    stdout, err = run_cli(["-o", "21", "--vcf", f1, "--anchor", out], CWD, "inv_del_bam_config")
    assert filter_cmd_lines(stdout) == filter_cmd_lines(plain)
    assert T.without_command(open(f1).read()) == T.without_command(open(f0).read())
    warning = [l for l in err.split("\n") if l.startswith("WARNING: --anchor")]
    assert len(warning) == 1 and "AM" in warning[0] and "--anchor-mapq 0" in warning[0]
    head, body, rows = table_of(out)
    assert rows == [] and body == A.HEADER
    window = A.default_window([float(run.lib_f[i][2]) for i in range(run.nlibs)])
    assert "#Window: %d" % window in head and "#Step: %d" % A.default_step(window) in head and "#Min: 3" in head and "#Mapq: -1" in head
    # --anchor-mapq 0 --anchor-min 1: the restatement's rows over the 7 candidates
    length = chr21_length(open(f0).read())
    names = {22: "21"}
    lengths = {22: min(length, 2**31 - 2)}
    minima = np.array([int(run.lib_i[i, 0]) if int(run.lib_i[i, 0]) >= 0 else int(run.opts["min_map_qual"]) for i in range(run.nlibs)], np.int64)
    want, exp = restated_table(soa, run.cls, minima, names, lengths, window, A.default_step(window), 1, 0)
    _, err = run_cli(["-o", "21", "--anchor", out, "--anchor-mapq", "0", "--anchor-min", "1"], CWD, "inv_del_bam_config")
    assert "WARNING: --anchor" not in err
    head, body, rows = table_of(out)
    assert body == want and "#Mapq: 0" in head and "#Min: 1" in head
    assert sum(r["n_fwd"] + r["n_rev"] for r in exp) >= 7 and all(r["n_low"] == 0 for r in exp)
