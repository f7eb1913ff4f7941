"""The region cut (launch_k3: head scan, accept scan, region table, k3_region_of_kernel) and the mate join (launch_k4_join_only: the direct
join with its fused region-of and its forward of the region table, the bucketed join with its scan and both of its tables) on their
own, through tests/prims/stages.hip, against the references of tests/region_cases.py (held to the oracle and to all-pairs statements by
tests/test_region_cases.py).  Every comparison is exact, word for word; what a launch must not touch has to come back as the 0xA5 bytes
it started as, and the guards behind every array intact.  The cut cases that a read stream can say also go through the whole product
against the oracle, once with the direct and once with the bucketed join.

The harness keeps the launchers' preconditions (look-back words zero once, a fresh stamp per call, c_maxq zero, counts inside their
arrays) and refuses a call that would break one; no launch here is meant to fault or to spin.  What no result shows: which mate
partner[] of a name seen three times holds (those entries are left out of the comparison; irregular = 1 is what counts)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import region_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "tests/prims/libbdx_stages.so"
HIP_INVALID_VALUE = 1
FILL = np.uint32(rc.FILL)
LOOP_MAX = 100000

_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")


def _opt(a, dtype):
    """a pointer the callee may get as null"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype)
    return a.ctypes.data_as(ctypes.c_void_p), a


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        env = dict(os.environ)
        env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call(["make", "-C", ROOT, TARGET], env=env)
    so = ctypes.CDLL(path)
    u32, i32, vp, ci = ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int
    so.stages_constants.argtypes = [_u32p]
    so.stages_constants.restype = None
    so.stages_cut_open.argtypes = [u32, ci, u32, ctypes.POINTER(vp)]
    so.stages_cut_close.argtypes = [vp]
    so.stages_cut_close.restype = None
    so.stages_cut_run.argtypes = [vp, _i32p, _i32p, _u32p, _u32p, _u32p, i32, u32, u32, u32, ci, ci, vp, ci, ci, u32] + [_i32p, _u32p, _i32p, _i32p, _i32p] + [_u32p] * 6
    so.stages_join_open.argtypes = [u32, u32, u32, u32, u32, ctypes.POINTER(vp)]
    so.stages_join_close.argtypes = [vp]
    so.stages_join_close.restype = None
    so.stages_join_run.argtypes = [vp, _u64p, vp, vp, vp, vp, u32, u32, ci, vp, vp, vp, u32, u32, ci, ci, ci, vp, vp, u32, ci, u32, u32] + [_i32p] * 3 + [_u32p] * 5
    k = np.zeros(4, np.uint32)
    so.stages_constants(k)
    assert k.tolist() == [rc.SCAN_BLOCK, rc.JOIN_LDS_SLOTS, rc.MAX_BUCKETS, rc.REC_WORDS]      # what the models are built on
    return so


class Cut:
    """one buffer set of the cut, kept from call to call; hands out the stamps: never the same one twice"""

    def __init__(self, so, cap, nkeys=1, ntids=0):
        self.so, self.cap, self.nkeys, self.ntids, self.stamp = so, cap, nkeys, ntids, 0
        self.h = ctypes.c_void_p()
        assert so.stages_cut_open(cap, nkeys, ntids, ctypes.byref(self.h)) == 0

    def close(self):
        self.so.stages_cut_close(self.h)

    def run(self, c, host_copy_later=0, region_of_launch=1, n=None, n_host=None, stamp=None):
        n = c["n"] if n is None else n
        n_host = max(c["n_host"], n) if n_host is None else n_host
        if stamp is None:
            self.stamp += 1
            stamp = self.stamp
        cap, nk = self.cap, self.nkeys
        o = dict(cand=np.zeros(cap, np.int32), c_first=np.zeros(cap, np.uint32), c_maxq=np.zeros(cap, np.int32), c_rid=np.zeros(cap, np.int32),
                 region_of=np.zeros(cap, np.int32), scratch=np.zeros((6, cap), np.uint32), rec_host=np.zeros((cap, rc.REC_WORDS), np.uint32),
                 pk_host=np.zeros((cap, 2 * nk), np.uint32), rec_dev=np.zeros((cap, rc.REC_WORDS), np.uint32), pk_dev=np.zeros((cap, 2 * nk), np.uint32),
                 counts=np.zeros(8, np.uint32))
        tail = _opt(c["tail"], np.uint32)
        if tail is not None and self.ntids:
            assert len(c["tail"]) == self.ntids
        pk = np.ascontiguousarray(c["pk"][:, :n])
        o["rc"] = self.so.stages_cut_run(self.h, np.ascontiguousarray(c["tid"][:n]), np.ascontiguousarray(c["pos"][:n]), np.ascontiguousarray(c["meta"][:n]),
                                         np.ascontiguousarray(c["nn"][:n]), pk, c["W"], n, c["n_normal"], n_host, c["min_len"], c["lim"],
                                         tail[0] if tail else None, host_copy_later, region_of_launch, stamp, o["cand"], o["c_first"], o["c_maxq"], o["c_rid"],
                                         o["region_of"], o["scratch"], o["rec_host"], o["pk_host"], o["rec_dev"], o["pk_dev"], o["counts"])
        return o


class Join:
    def __init__(self, so, cap, fcap=0, ccap=0, slots=0, rcap=0):
        self.so, self.cap, self.fcap, self.ccap, self.slots, self.rcap = so, cap, fcap, ccap, slots, rcap
        self.h = ctypes.c_void_p()
        assert so.stages_join_open(cap, fcap, ccap, slots, rcap, ctypes.byref(self.h)) == 0

    def close(self):
        self.so.stages_join_close(self.h)

    def run(self, c, region=True, cand=None, c_rid=None, want_pair_lo=1, with_scratch=0, forward=None, nkeys2=2, nbuckets=0, n_host=None):
        cap, r = self.cap, max(self.rcap, 1)
        o = dict(partner=np.zeros(cap, np.int32), pair_lo=np.zeros(cap, np.int32), region_out=np.zeros(cap, np.int32), scratch=np.zeros((6, cap), np.uint32),
                 fwd_rec=np.zeros((r, rc.REC_WORDS), np.uint32), fwd_pk=np.zeros(r * 16, np.uint32), boff=np.zeros(rc.MAX_BUCKETS + 1, np.uint32),
                 counts=np.zeros(8, np.uint32))
        keep = [_opt(c["check"], np.uint64), _opt(c["region"] if region else None, np.int32), _opt(cand, np.int32), _opt(c_rid, np.int32),
                _opt(c["fkey"], np.uint64), _opt(c["fcheck"], np.uint64), _opt(c["fregion"], np.int32),
                _opt(forward[0] if forward else None, np.uint32), _opt(forward[1] if forward else None, np.uint32)]
        p = [k[0] if k else None for k in keep]
        o["rc"] = self.so.stages_join_run(self.h, c["key"], p[0], p[1], p[2], p[3], 0 if c_rid is None else len(c_rid), c["n"], 1 if c["nf"] else 0, p[4], p[5], p[6],
                                          c["nf"], c["n_host"] if n_host is None else n_host, want_pair_lo, with_scratch, 1 if forward else 0, p[7], p[8],
                                          len(forward[0]) if forward else 0, nkeys2, nbuckets, nbuckets.bit_length() - 1 if nbuckets else 0,
                                          o["partner"], o["pair_lo"], o["region_out"], o["scratch"], o["fwd_rec"], o["fwd_pk"], o["boff"], o["counts"])
        return o


@pytest.fixture(scope="module")
def handles(lib):
    """buffer sets by shape, opened when first asked for and kept for the module: a case runs on what earlier cases left behind"""
    pool = {}

    def get(kind, *shape):
        if (kind,) + shape not in pool:
            pool[(kind,) + shape] = (Cut if kind == "cut" else Join)(lib, *shape)
        return pool[(kind,) + shape]

    yield get
    for h in pool.values():
        h.close()


_REFS = {}


def cut_ref(c):
    if c["name"] not in _REFS:
        _REFS[c["name"]] = rc.cut_reference(c) if c["n"] <= LOOP_MAX else rc.cut_vectorised(c)
    return _REFS[c["name"]]


def cut_cap(c):
    return next(cap for cap in (2048, 80000, rc.TWO_PER_LANE + 513) if c["n_host"] <= cap)


def untouched(a, what):
    assert (a.view(np.uint32) == FILL).all(), (what, "written")


def check_cut(c, o, ref, host_copy_later, region_of_launch):
    name = c["name"]
    assert o["rc"] == 0, (name, o["rc"])
    n, nc, nr = c["n"], ref["n_cand"], ref["n_regions"]
    want_counts = [nc, nr, ref["last_maxq"]]
    assert o["counts"][:3].tolist() == want_counts, (name, "device counts", o["counts"].tolist(), want_counts)
    assert o["counts"][3:6].tolist() == want_counts, (name, "host mirror", o["counts"].tolist(), want_counts)
    assert o["counts"][6] == 0, (name, "a guard was written")
    for k, m in (("cand", n), ("c_first", nc), ("c_maxq", nc), ("c_rid", nc)):
        bad = np.flatnonzero(o[k][:m] != ref[k])
        assert bad.size == 0, (name, k, "first wrong", int(bad[0]), int(o[k][bad[0]]), int(ref[k][bad[0]]), "wrong", int(bad.size))
    untouched(o["cand"][n:], (name, "cand past n"))
    untouched(o["c_first"][nc:], (name, "c_first past n_cand"))
    untouched(o["c_rid"][nc:], (name, "c_rid past n_cand"))
    assert (o["c_maxq"][nc:] == 0).all(), (name, "c_maxq past n_cand")
    if region_of_launch:
        np.testing.assert_array_equal(o["region_of"][:n], ref["region_of"], err_msg=name)
        untouched(o["region_of"][n:], (name, "region_of past n"))
        want = np.zeros((6, n), np.uint32)
        want[1] = np.arange(n)
        np.testing.assert_array_equal(o["scratch"][:, :n], want, err_msg=name + " scratch")
        untouched(o["scratch"][:, n:], (name, "scratch past n"))
    else:
        untouched(o["region_of"], (name, "region_of without its launch"))
        untouched(o["scratch"], (name, "scratch without its launch"))
    for side in ("dev",) + (() if host_copy_later else ("host",)):
        for k in ("rec", "pk"):
            got = o[k + "_" + side]
            bad = np.flatnonzero((got[:nr] != ref[k]).any(axis=1))
            assert bad.size == 0, (name, k, side, "first wrong region", int(bad[0]), got[bad[0]].tolist(), ref[k][bad[0]].tolist(), "wrong", int(bad.size))
            untouched(got[nr:], (name, k, side, "past n_regions"))
    if host_copy_later:
        untouched(o["rec_host"], (name, "host table with host_copy_later"))
        untouched(o["pk_host"], (name, "host samples with host_copy_later"))


CUT_NAMES = [c["name"] for c in rc.cut_cases()]


@pytest.mark.parametrize("name", CUT_NAMES)
def test_cut(handles, name):
    c = rc.cut_case_named(name)
    i = CUT_NAMES.index(name)
    hcl, rol = i & 1, (i >> 1) & 1 ^ 1
    h = handles("cut", cut_cap(c), c["nkeys"], 0 if c["tail"] is None else len(c["tail"]))
    check_cut(c, h.run(c, hcl, rol), cut_ref(c), hcl, rol)


@pytest.mark.parametrize("name", ["n513", "run257_straddle", "tail_raises_maxq", "counts_wrap_3_keys", "n%d" % (rc.TWO_PER_LANE + 1)])
def test_cut_with_every_pair_of_flags(handles, name):
    c = rc.cut_case_named(name)
    h = handles("cut", cut_cap(c), c["nkeys"], 0 if c["tail"] is None else len(c["tail"]))
    for hcl in (0, 1):
        for rol in (0, 1):
            check_cut(c, h.run(c, hcl, rol), cut_ref(c), hcl, rol)


def test_four_cuts_of_shrinking_size_on_one_buffer_set(lib):
    h = Cut(lib, 1100)
    try:
        for name in ("n1025", "n513", "n65", "n2"):
            c = rc.cut_case_named(name)
            check_cut(c, h.run(c, 0, 1), cut_ref(c), 0, 1)
    finally:
        h.close()


def test_cut_of_no_reads_writes_nothing(handles):
    c = rc.cut_case_named("n65")
    o = handles("cut", 2048, 1, 0).run(c, 0, 1, n=0, n_host=0)
    assert o["rc"] == 0 and o["counts"].tolist() == [0, 0, 0, rc.FILL, rc.FILL, rc.FILL, 0, 0]
    for k in ("cand", "c_first", "c_rid", "region_of", "scratch", "rec_host", "pk_host", "rec_dev", "pk_dev"):
        untouched(o[k], k)


def test_cut_calls_that_break_a_precondition_are_refused(lib):
    h = Cut(lib, 512)
    try:
        c = rc.cut_case_named("n257")
        assert h.run(c, stamp=0)["rc"] == HIP_INVALID_VALUE
        assert h.run(c, stamp=1 << 30)["rc"] == HIP_INVALID_VALUE
        assert h.run(c, stamp=7)["rc"] == 0
        assert h.run(c, stamp=7)["rc"] == HIP_INVALID_VALUE                    # a stamp the look-back words have seen
        assert h.run(c, n_host=100, stamp=8)["rc"] == HIP_INVALID_VALUE        # more reads on the device than the launches are sized for
        assert h.run(c, n_host=513, stamp=8)["rc"] == HIP_INVALID_VALUE        # more than the arrays hold
        assert h.run(rc.cut_case_named("tail_raises_maxq"), stamp=8)["rc"] == HIP_INVALID_VALUE      # a tail table without room for one
        check_cut(c, h.run(c, stamp=8), cut_ref(c), 0, 1)                      # (a refused call leaves the stamp free and the buffers usable)
    finally:
        h.close()


# ---- the join ---------------------------------------------------------------------------------------------------------------------

def check_join(c, o, ref, direct, nbuckets=0):
    name, n = c["name"], c["n"]
    assert o["rc"] == 0, (name, o["rc"])
    assert o["counts"][2] == 0, (name, "a guard was written")
    assert o["counts"][0] == ref["irregular"], (name, "irregular", int(o["counts"][0]))
    keep = ~ref["loose"]
    bad = np.flatnonzero((o["partner"][:n] != ref["partner"]) & keep)
    assert bad.size == 0, (name, "partner: first wrong", int(bad[0]), int(o["partner"][bad[0]]), int(ref["partner"][bad[0]]), "wrong", int(bad.size))
    untouched(o["partner"][n:], (name, "partner past n"))
    if direct:
        bad = np.flatnonzero((o["pair_lo"][:n] != ref["pair_lo"]) & keep)
        assert bad.size == 0, (name, "pair_lo: first wrong", int(bad[0]), int(o["pair_lo"][bad[0]]), int(ref["pair_lo"][bad[0]]), "wrong", int(bad.size))
        untouched(o["pair_lo"][n:], (name, "pair_lo past n"))
        assert o["counts"][1] == rc.FILL, (name, "n_entries is the bucket scan's")
    else:
        untouched(o["pair_lo"], (name, "pair_lo is the direct join's"))
        assert o["counts"][1] == n, (name, "n_entries", int(o["counts"][1]))
        np.testing.assert_array_equal(o["boff"][:nbuckets + 1], rc.bucket_offsets(c, nbuckets), err_msg=name + " bucket offsets")
        assert o["counts"][3] == 0, (name, "bcnt not left clean", int(o["counts"][3]))


DIRECT = [c["name"] for c in rc.join_cases() if c["direct"]]
BUCKETED = [(c["name"], nb) for c in rc.join_cases() if c["bucketed"] for nb in c["nbuckets"]]


@pytest.mark.parametrize("name", DIRECT)
def test_direct_join(handles, name):
    c = rc.join_case_named(name)
    h = handles("join", c["slots"] // 2, 64, 0, c["slots"], 0)
    o = h.run(c)
    check_join(c, o, rc.join_reference(c), True)
    untouched(o["region_out"], "region_out without the fused region-of")
    untouched(o["scratch"], "scratch without the fused region-of")


@pytest.mark.parametrize("name,nbuckets", BUCKETED)
def test_bucketed_join(handles, name, nbuckets):
    c = rc.join_case_named(name)
    o = handles("join", 16384).run(c, nbuckets=nbuckets)         # one buffer set for all of them: bcnt is zero at allocation only
    check_join(c, o, rc.join_reference(c), False, nbuckets)


def test_two_bucketed_joins_on_one_buffer_set(lib):
    h = Join(lib, 4096)
    try:
        for name, nb in (("mates_in_different_workgroups", 2048), ("n513", 2), ("mates_in_different_workgroups", 8192), ("names_seen_once", 1024)):
            c = rc.join_case_named(name)
            check_join(c, h.run(c, nbuckets=nb), rc.join_reference(c), False, nb)
    finally:
        h.close()


def test_join_of_no_entries_writes_nothing(handles):
    c = rc.join_case_named("n257")
    empty = dict(c, n=0, n_host=0, key=c["key"][:1], region=c["region"][:1])
    for h, nb in ((handles("join", 512, 64, 0, 1024, 0), 0), (handles("join", 16384), 2)):
        o = h.run(empty, nbuckets=nb)
        assert o["rc"] == 0 and o["counts"].tolist() == [0, rc.FILL, 0, 0, 0, 0, 0, 0]
        for k in ("partner", "pair_lo", "region_out", "scratch"):
            untouched(o[k], k)


def test_join_calls_that_break_a_precondition_are_refused(handles):
    c = rc.join_case_named("n513")
    assert handles("join", 512, 64, 0, 1024, 0).run(c)["rc"] == HIP_INVALID_VALUE                # a table more than half full
    assert handles("join", 16384).run(c, nbuckets=3)["rc"] == HIP_INVALID_VALUE
    assert handles("join", 16384).run(c, nbuckets=2 * rc.MAX_BUCKETS)["rc"] == HIP_INVALID_VALUE
    assert handles("join", 16384).run(rc.join_case_named("foreign_entries"), nbuckets=2)["rc"] == HIP_INVALID_VALUE      # foreign entries: the direct table only


@pytest.mark.parametrize("name", ["n513", "run65_end63", "coverage_at_lim_3", "one_candidate"])
def test_fused_region_of_is_k3_region_of_kernel(handles, name):
    """the same cut once with k3_region_of_kernel's launch and once through the join's replacement of it: region ids and K6's scratch"""
    c = rc.cut_case_named(name)
    cap = 8192
    o = handles("cut", cap, 1, 0).run(c, 0, 1)
    ref = cut_ref(c)
    check_cut(c, o, ref, 0, 1)
    n = c["n"]
    keys = rc.paired(n, 31)
    j = dict(rc.join_case("fused_" + name, keys, np.zeros(n, np.int32), slots=4 * cap))
    f = handles("join", cap, 64, cap, 4 * cap, 0).run(j, region=False, cand=o["cand"][:n], c_rid=o["c_rid"][:ref["n_cand"]], with_scratch=1, want_pair_lo=0)
    jref = rc.join_reference(dict(j, region=ref["region_of"]))
    check_join(j, f, jref, True)                                  # pair_lo without want_pair_lo: single-context runs derive it from c_rid
    np.testing.assert_array_equal(f["region_out"], o["region_of"])
    np.testing.assert_array_equal(f["scratch"], o["scratch"])


@pytest.mark.parametrize("nkeys2", rc.FORWARD_NKEYS2)
def test_forward_of_the_region_table(handles, nkeys2):
    c = rc.join_case_named("n257")
    h = handles("join", 512, 64, 0, 1024, max(rc.FORWARD_REGIONS))
    for nr in rc.FORWARD_REGIONS:
        rec, pk = rc.forward_table(nr, nkeys2)
        o = h.run(c, forward=(rec, pk), nkeys2=nkeys2)
        check_join(c, o, rc.join_reference(c), True)
        np.testing.assert_array_equal(o["fwd_rec"][:nr], rec, err_msg="records of %d regions" % nr)
        untouched(o["fwd_rec"][nr:], ("records past", nr))
        np.testing.assert_array_equal(o["fwd_pk"][:nr * nkeys2], pk.reshape(-1), err_msg="samples of %d regions" % nr)
        untouched(o["fwd_pk"][nr * nkeys2:], ("samples past", nr))


# ---- the same boundaries in a real run ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bucketed", [0, 1], ids=["direct", "bucketed"])
@pytest.mark.parametrize("name", [c["name"] for c in rc.cut_cases() if c["stream"]])
def test_cut_cases_through_the_whole_product(monkeypatch, name, bucketed):
    from helpers import make_opts
    from runner import compare, oracle_case, product_from_oracle
    c = rc.cut_case_named(name)
    config, streams, targets = rc.stream_of(c)
    run = oracle_case(config, streams, targets, make_opts(min_len=c["min_len"], seq_coverage_lim=c["lim"], min_read_pair=1))
    if bucketed:
        monkeypatch.setenv("BDX_BUCKETED_JOIN", "1")
    bd = product_from_oracle(run)
    s = compare(run, bd)
    assert s["window"] == c["W"]
    assert run.n_regions == cut_ref(c)["n_regions"] + (1 if c["min_len"] < 0 else 0)
