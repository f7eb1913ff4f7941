"""The cases of tests/test_gpu_insert.py without a GPU (tests/insert_cases.py): the reference against a naive O(n^2) placement, the
route model against the routes, boundaries and bucket depths the cases are there for, the bucket function's order, and the cases'
strength against slips of the two index computations no library restates (placement through buckets, rank by slices and tiles)."""
import numpy as np
import pytest

import insert_cases as ic

ALL = ic.CASES + ic.SEQUENCE


@pytest.fixture(scope="module")
def built():
    out = {}
    for c in ALL:
        d = ic.build(c)
        for a in d.values():
            a.setflags(write=False)
        out[c["name"]] = d
    return out


def same(a, b):
    return a[1:] == b[1:] and all((x == y).all() for x, y in zip(a[0], b[0]))


def test_the_generators_keep_the_kernels_preconditions(built):
    """device keys that differ, with the own bit clear, T a multiple of the period and a sequence number inside its bits; host keys ascending with
    sequence number 0 and runs of equal keys somewhere; no (T, own, start) on both sides; slots that differ, below the staging size"""
    runs = 0
    for c in ALL:
        d = built[c["name"]]
        dk, hk = d["old_key"], d["hs_key"]
        assert len(dk) == c["nd"] and len(hk) == c["nh"], c["name"]
        assert len(np.unique(dk)) == len(dk), c["name"]
        assert ((dk >> np.uint64(ic.SHIFT_OWN)) & np.uint64(1) == 0).all(), c["name"]
        assert ((dk >> np.uint64(ic.SHIFT_T)) % np.uint64(max(c["period"], 1)) == 0).all(), c["name"]
        assert (hk[1:] >= hk[:-1]).all() and (hk & np.uint64(ic.SEQ_MASK) == 0).all(), c["name"]
        assert not np.isin(dk >> np.uint64(ic.SHIFT_START), hk >> np.uint64(ic.SHIFT_START)).any(), c["name"]
        assert len(np.unique(d["old_slot"])) == c["nd"] and (d["old_slot"] < 2 * c["handle"][0]).all(), c["name"]
        assert d["cnt_by_slot"].max(initial=0) < 65536
        runs += int((hk[1:] == hk[:-1]).any())
    assert runs > 100


def test_the_reference_is_the_naive_placement(built):
    seen = 0
    for c in ALL:
        if 0 < c["nd"] + c["nh"] <= 4096 and c["nd"] + c["nh"] <= c["handle"][0]:
            assert same(ic.reference(c, built[c["name"]]), ic.naive_reference(c, built[c["name"]])), c["name"]
            seen += 1
    assert seen > 50


def test_every_route_is_reached_and_every_case_takes_the_one_it_is_there_for(built):
    routes = {}
    for c in ALL:
        r = ic.route_of(c, built[c["name"]])
        assert r == c["expect"], (c["name"], r, c["expect"])
        routes.setdefault(r, []).append(c)
    assert set(routes) == set(ic.ROUTES) | {"overflow", "empty"}
    assert {ic.family(c) for c in ic.CASES} == set(ic.FAMILIES)
    # host keys in LDS and in HBM, totals in LDS and in place, on every ranking route that can hold that many
    for r in ic.ROUTES:
        assert {ic.host_keys_in_lds(c["nh"]) for c in routes[r]} == {True, False}, r
        assert {ic.totals_in_lds(c["nd"], c["nh"]) for c in routes[r]} == {True, False}, r
    # the three counts on every route
    for r in ic.ROUTES:
        assert {c["counts"] for c in routes[r]} == {"rand", "zero", "max"}, r
    # the rank sort without rank_part, and ins_plain's three values
    assert any(c["handle"][1] == 0 and c["ins_plain"] == 1 and c["nd"] > ic.INS_THREADS for c in ALL)
    assert {c["ins_plain"] for c in ALL} == {0, 1, 2}


def test_each_boundary_pair_falls_on_two_sides():
    e = {c["name"]: c["expect"] for c in ic.CASES}
    for nh in (0, 1, 700):
        def r(nd):
            return e["nd-%d-nh-%d" % (nd, nh)]
        assert (r(1024), r(1025)) == ("rank", "bucket")
        assert (r(8192), r(8193)) == ("bucket", "ranksort")
        assert (r(1 << 17), r((1 << 17) + 1)) == ("ranksort", "hbm_bitonic")
    assert (e["plain1-nd-2048"], e["plain1-nd-2049"]) == ("lds_bitonic", "ranksort")
    assert (e["plain2-nd-2048"], e["plain2-nd-2049"]) == ("lds_bitonic", "hbm_bitonic")
    assert (e["norank-plain1-nd-1025"], e["norank-plain1-nd-2048"]) == ("lds_bitonic", "lds_bitonic")
    assert (e["one-too-many"], e["one-too-many-host"], e["nothing"]) == ("overflow", "overflow", "empty")
    assert ic.host_keys_in_lds(2048) and not ic.host_keys_in_lds(2049)
    for a, b in (((8192, 2048), (8192, 2049)), ((1024, 9216), (1024, 9217)), ((0, 10240), (0, 10241)), ((10240, 0), (10241, 0))):
        assert "n-%d+%d" % a in e and "n-%d+%d" % b in e
        assert ic.totals_in_lds(*a) and not ic.totals_in_lds(*b)
    assert (5000 + 6264) % ic.INS_THREADS == 0 and (1024 + 10240) % ic.INS_THREADS == 0
    # rank_layout: 16 / 15 and 2 / 1 slices, more work items than workgroups, a partial last tile, a slice that ends before k0 + per
    assert [ic.rank_layout(nd)[1] for nd in (4096, 4097, 32768, 32769)] == [16, 15, 2, 1]
    nchunk, nslice, _ = ic.rank_layout(65537)
    assert nchunk * nslice > ic.RANK_GRID
    assert any(ic.rank_layout(c["nd"])[2] % ic.RANK_TILE for c in ic.CASES if c["expect"] == "ranksort")
    assert any(ic.rank_layout(c["nd"])[1] * ic.rank_layout(c["nd"])[2] > c["nd"] for c in ic.CASES if c["expect"] == "ranksort")
    full = e["full-%d" % ic.TIGHT[0]]
    assert full == "bucket" and 2300 + 700 == ic.TIGHT[0]


def test_the_bucket_cases_are_as_deep_as_they_say(built):
    """no bucket above kInsBucketDepth on the bucket route; exactly 128 and exactly 129 entries in the deep cases' bucket -- the first,
    a middle one, the last -- with host keys of the list inside it"""
    wheres = set()
    for c in ic.CASES:
        d = built[c["name"]]
        deepest = ic.deepest_bucket(c, d)
        if c["expect"] == "bucket":
            assert deepest <= ic.INS_BUCKET_DEPTH, c["name"]
        if c["gen"] == "deep":
            b = np.bincount(ic.bucket_model(d["old_key"], c["n_regions"], c["period"]), minlength=ic.INS_BUCKETS)
            assert deepest == c["args"]["depth"] and (b == deepest).sum() == 1 and np.sort(b)[-2] <= 64, c["name"]
            where = int(b.argmax())
            wheres.add(where)
            hb = ic.bucket_model(d["hs_key"], c["n_regions"], c["period"])
            assert (hb == where).sum() >= 40, c["name"]
            inside = d["old_key"][ic.bucket_model(d["old_key"], c["n_regions"], c["period"]) == where]
            hin = d["hs_key"][hb == where]
            assert inside.min() < hin.max() and hin.min() < inside.max(), c["name"]
        elif c["crowded"]:
            assert deepest > ic.INS_BUCKET_DEPTH, c["name"]
    assert 0 in wheres and ic.INS_BUCKETS - 1 in wheres and len(wheres) == 3


def test_the_bucket_model_does_not_decrease_along_the_keys(built):
    """over every case's keys, host and device together: the merge through buckets rests on that"""
    for c in ALL:
        d = built[c["name"]]
        k = np.sort(np.concatenate([d["old_key"], d["hs_key"]]))
        b = ic.bucket_model(k, c["n_regions"], c["period"]).astype(np.int64)
        assert (np.diff(b) >= 0).all(), c["name"]
        assert b.max(initial=0) < ic.INS_BUCKETS


def test_the_clamp_of_the_second_half_window_never_binds(built):
    """sub = kSub / 2 + min(kSub / 2 - 1, (start + period - T) * (kSub / 2) / period) is reached with T - period <= start < T only, so the
    quotient's numerator is below period * (kSub / 2) and the quotient below kSub / 2 whatever the key: the min() cannot change a result, and
    no case can tell a kernel without it from one with it.  Held here over every key of every case, and over the whole window before a threshold"""
    for c in ALL:
        d = built[c["name"]]
        k = np.concatenate([d["old_key"], d["hs_key"]])
        assert (ic.bucket_model(k, c["n_regions"], c["period"]) == ic.bucket_model(k, c["n_regions"], c["period"], clamp=False)).all(), c["name"]
    for period in (1, 2, 31, 32, 33, 101, 4096):
        for W in (1, 2, 77):
            k = ic.window_pool(W, period)
            assert (ic.bucket_model(k, 100 * period, period) == ic.bucket_model(k, 100 * period, period, clamp=False)).all()


def test_the_model_of_the_two_index_computations_passes_every_case(built):
    for c in ALL:
        d = built[c["name"]]
        got, route = ic.model(c, d)
        assert route == c["expect"], c["name"]
        assert same(got, ic.reference(c, d)), c["name"]


@pytest.mark.parametrize("slip", ic.SLIPS)
def test_a_slip_in_the_model_fails_a_case(built, slip):
    """a slice's end taken as k0 + per without min(nd, ...); hc[0] used for the host entries j >= 1,024; 'totals in LDS' decided by nd
    instead of n; the crowding test at > kInsBucketDepth instead of >=.  (The fifth slip of the bucket function, its second half-window
    without the clamp, changes no result: test_the_clamp_of_the_second_half_window_never_binds)"""
    failed = []
    for c in ic.CASES:
        if slip == "slice_end" and c["expect"] != "ranksort":
            continue
        if slip == "hc0" and not (c["expect"] == "bucket" and c["nh"] > ic.INS_THREADS):
            continue
        if slip == "small_by_nd" and not (c["nd"] <= ic.INS_CNT_LDS < c["nd"] + c["nh"] <= c["handle"][0]):
            continue
        if slip == "depth_gt" and c["gen"] != "deep":
            continue
        d = built[c["name"]]
        got, route = ic.model(c, d, slip)
        if route != c["expect"] or not same(got, ic.reference(c, d)):
            failed.append(c["name"])
    assert failed, slip
