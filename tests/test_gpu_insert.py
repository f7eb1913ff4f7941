"""K6's order-key insertion merge on its own, through tests/prims/prims.hip: k6_ranksort_kernel and k6_insert_kernel of
csrc/bdx_insert.h, launched by the header's own two launch functions as the product launches them, against the plain stable merge
of tests/insert_cases.py on every ranking route -- rank counting, buckets, the crowded fallback to the two bitonic sorts, the rank
sort, the bitonic sorts -- at the sizes where the routes, the home of the host's keys and the home of the running totals change.
Every comparison is exact: the four arrays up to n, the totals at [n], the filler beyond, n_ins, overflow and the guards.

The harness refuses a call that breaks a precondition of the kernel (equal device keys, a start vertex on both sides, descending
host keys, a list beyond a capacity, a count beyond 16 bits); no such launch is ever made."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import insert_cases as ic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "tests/prims/libbdx_prims.so"
HIP_INVALID_VALUE = 1

_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, TARGET)
    if not os.path.exists(path):
        env = dict(os.environ)
        env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call(["make", "-C", ROOT, TARGET], env=env)
    so = ctypes.CDLL(path)
    u32, vp, i = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int
    so.prims_insert_constants.argtypes = [_u32p]
    so.prims_insert_constants.restype = None
    so.prims_insert_bucket.argtypes = [_u64p, u32, u32, i, _u32p]
    so.prims_insert_open.argtypes = [u32, i, ctypes.POINTER(vp)]
    so.prims_insert_close.argtypes = [vp]
    so.prims_insert_close.restype = None
    so.prims_insert_run.argtypes = [vp, _u64p, _u32p, _u32p, u32, _u64p, _u32p, u32, u32, i, i, _u32p, _u32p, _u32p, _u32p, _u32p]
    return so


class Handle:
    def __init__(self, so, sv_cap, with_rank):
        self.so, self.sv_cap = so, sv_cap
        self.h = ctypes.c_void_p()
        assert so.prims_insert_open(sv_cap, with_rank, ctypes.byref(self.h)) == 0

    def run(self, c, d, expect_rc=0):
        out = [np.zeros(self.sv_cap + 1, np.uint32) for _ in range(4)]
        counts = np.zeros(3, np.uint32)
        rc = self.so.prims_insert_run(self.h, d["old_key"], d["old_slot"], d["cnt_by_slot"], len(d["old_key"]), d["hs_key"], d["hs_cnt"], len(d["hs_key"]),
                                      c["n_regions"], c["period"], c["ins_plain"], *out, counts)
        assert rc == expect_rc, (c["name"], rc)
        return out, counts

    def close(self):
        self.so.prims_insert_close(self.h)
        self.h = None


@pytest.fixture(scope="module")
def handles(lib):
    """one buffer set per size for the whole module: like a context's, it goes from launch to launch uncleared"""
    open_ = {}

    def get(key):
        if key not in open_:
            open_[key] = Handle(lib, *key)
        return open_[key]
    yield get
    for h in open_.values():
        h.close()


NAMES = ("ins_T", "ins_src", "ins_pre_l", "ins_pre_c")


def check(c, d, got, counts):
    want, n_ins, overflow = ic.reference(c, d)
    n = c["nd"] + c["nh"]
    assert counts.tolist() == [n_ins, overflow, 0], (c["name"], "n_ins, overflow, guard bytes changed", counts.tolist(), [n_ins, overflow, 0])
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (c["name"], c["expect"], name, "n", n, "first wrong entry", int(bad[0]), hex(int(g[bad[0]])), "want", hex(int(w[bad[0]])),
                               "wrong entries", int(bad.size), "of them behind the list", int((bad >= n).sum()))


def run_family(handles, fam):
    seen = 0
    for c in ic.CASES:
        if ic.family(c) == fam:
            d = ic.build(c)
            check(c, d, *handles(c["handle"]).run(c, d))
            seen += 1
    assert seen


def test_the_constants_of_the_header_are_the_models(lib):
    got = np.zeros(len(ic.CONSTANTS), np.uint32)
    lib.prims_insert_constants(got)
    assert got.tolist() == ic.CONSTANTS


def test_the_bucket_function_is_the_models_on_every_key_of_every_case(lib):
    """ins_bucket_of with ins_bucket_span's span, a lane per key, over the host's and the device's keys of all cases"""
    for c in ic.CASES + ic.SEQUENCE:
        d = ic.build(c)
        k = np.ascontiguousarray(np.concatenate([d["old_key"], d["hs_key"]]))
        if not len(k):
            continue
        got = np.zeros(len(k), np.uint32)
        assert lib.prims_insert_bucket(k, len(k), c["n_regions"], c["period"], got) == 0
        bad = np.flatnonzero(got != ic.bucket_model(k, c["n_regions"], c["period"]))
        assert bad.size == 0, (c["name"], "first wrong key", hex(int(k[bad[0]])), int(got[bad[0]]), "wrong", int(bad.size))
    k = np.array([0], np.uint64)   # period 0 and below count as 1
    got = np.zeros(1, np.uint32)
    for period in (0, -5):
        assert lib.prims_insert_bucket(k, 1, 1000, period, got) == 0 and got[0] == ic.bucket_model(k, 1000, period)[0]


def test_rank_counting_route(handles):
    """nd <= 1,024, one entry per thread: 0, 1, 63 ... 1,024 device entries beside 0 ... 10,241 host entries -- the host's keys in LDS and
    (above 2,048) in HBM, the totals in LDS and (n above 10,240) scanned in place; all host keys 0 with an empty device list"""
    run_family(handles, "rank")


def test_bucket_route(handles):
    """1,025 ... 8,192 device entries through the buckets: both ends, a bucket of exactly kInsBucketDepth entries as bucket 0, a middle
    one and bucket 2,047 with host keys inside it, host lists of 1,023 ... 2,049 entries (the prefetched counts hc[0] / hc[1], then HBM),
    device keys wholly below / above / alternating with the host's, runs of equal host keys between device keys of their threshold,
    period 1, a span below kInsBuckets, 2^26 - 2 regions, T = 0, start vertices at and behind T"""
    run_family(handles, "bucket")


def test_crowded_buckets_fall_back_to_the_bitonic_sorts(handles):
    """one bucket of kInsBucketDepth + 1 entries (first, middle, last), ins_plain = 2, and a period above the region count (every key in
    one bucket): the LDS sort up to 2,048 entries, the sort in HBM over old_key above"""
    run_family(handles, "crowded")


def test_rank_sort_route(handles):
    """k6_ranksort_kernel's partial ranks added up and placed: 8,193 ... 2^17 entries, and from 2,049 with ins_plain = 1 -- 16 / 15 and
    2 / 1 slices, more work items than workgroups, a partial last tile, slices that end before k0 + per"""
    run_family(handles, "ranksort")


def test_bitonic_routes(handles):
    """2^17 + 1 entries (one workgroup's sort in HBM), and ins_plain = 1 without rank_part (sv_cap <= 2,048: the LDS sort)"""
    run_family(handles, "bitonic")


def test_capacity_edges(handles):
    """n == sv_cap writes the totals into the last word; n == sv_cap + 1 sets overflow, n_ins = 0, zeros at [0] and writes nothing else;
    n == 0 writes the two zeros only"""
    run_family(handles, "capacity")


def test_a_result_does_not_depend_on_the_call_before(lib):
    """a buffer set of its own: 2^17 entries, then 2,049 with ins_plain = 1, then 1,025, then 3 -- rank_part, sorted_key / sorted_slot,
    hs_key_dev and the keys behind old_key[nd] still hold the earlier calls'"""
    h = Handle(lib, *ic.SEQUENCE[0]["handle"])
    try:
        for c in ic.SEQUENCE:
            assert c["handle"] == ic.SEQUENCE[0]["handle"]
            d = ic.build(c)
            check(c, d, *h.run(c, d))
    finally:
        h.close()


def test_the_harness_refuses_a_launch_that_would_break_the_preconditions(lib):
    """equal device keys, a device key with a host key's (T, own, start), descending host keys, a slot beyond the staging records, a count
    of 2^16, a device list beyond old_key's capacity: hipErrorInvalidValue and no launch; the same call without the fault runs"""
    c = ic.BY_NAME["nd-65-nh-700"]
    d = ic.build(c)
    h = Handle(lib, 1000, 1)
    try:
        small = dict(c, handle=(1000, 1))
        ok = dict(d, cnt_by_slot=ic.stage_counts(1000, "rand"), old_slot=np.arange(65, dtype=np.uint32))
        check(small, ok, *h.run(small, ok))

        def refused(**kw):
            h.run(small, dict(ok, **kw), expect_rc=HIP_INVALID_VALUE)
        dup = d["old_key"].copy()
        dup[7] = dup[40]
        refused(old_key=dup)
        both = d["old_key"].copy()
        both[3] = d["hs_key"][100] | np.uint64(5)
        refused(old_key=both)
        refused(hs_key=np.ascontiguousarray(d["hs_key"][::-1]))
        slot = np.arange(65, dtype=np.uint32)
        slot[9] = 2000
        refused(old_slot=slot)
        wide = ic.stage_counts(1000, "rand").copy()
        wide[12, 1] = 65536
        refused(cnt_by_slot=wide)
        big = ic.device_pool(np.random.default_rng(1), 1100, ic.REGIONS, ic.PERIOD)[:1025]
        refused(old_key=np.ascontiguousarray(big), old_slot=np.arange(1025, dtype=np.uint32), hs_key=np.zeros(0, np.uint64), hs_cnt=np.zeros(0, np.uint32))
    finally:
        h.close()
