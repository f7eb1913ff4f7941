"""Ground truth for tests/assemble_cases.py, without a GPU: the read-level reference of the walk against the oracle on every case a read
stream can say, the models of the groups stage against plain loops, the coverage the cases are there for asserted from the models, and
a list of slips applied to the reference or the models, each of which must fail at least one case."""
import math

import numpy as np
import pytest

import assemble_cases as ac
from helpers import oracle_lib

CASES = ac.table_cases()
WALKED = [c for c in CASES if not c["groups_only"]]
STREAMS = [(seed, o) for seed in (1, 2, 3) for o in ac.STREAM_SETS]


@pytest.fixture(scope="module")
def tail():
    L = oracle_lib()

    def f(lam, k):
        p = L.bdo_poisson_upper_tail(float(lam), int(k))
        return math.log(p) if p > 0 else -math.inf
    return f


@pytest.fixture(scope="module")
def refs():
    return {c["name"]: ac.walk_reference(c) for c in WALKED}


@pytest.fixture(scope="module")
def models():
    return {c["name"]: ac.groups_model(c) for c in CASES}


@pytest.mark.parametrize("seed,optset", STREAMS, ids=["%d-%s" % (s, "-".join("%s%d" % kv for kv in sorted(o.items())) or "defaults") for s, o in STREAMS])
def test_the_reference_is_the_oracles_walk_on_every_stream_case(tail, seed, optset):
    run, c = ac.stream_case(seed, optset)
    assert c["n_regions"] == run.n_regions and run.n_svs > 10
    np.testing.assert_array_equal(c["rec"][:, :3].view(np.int32), run.regions[:, 1:4])
    assert ac.differs_from_oracle(run, ac.walk_reference(c, tail=tail)) is None


def test_every_table_case_says_why_no_stream_can_say_it_or_could_be_one():
    for c in CASES:
        assert c["why_no_stream"] is None or len(c["why_no_stream"]) > 20, c["name"]
        assert c["n_regions"] <= 300 and c["n_reads"] <= ac.MAX_CAP, c["name"]
        first, n = c["rec"][:, 8].astype(np.int64), c["rec"][:, 3].astype(np.int64)
        assert (first + n <= c["n_reads"]).all() and (np.diff(first) >= 0).all(), c["name"]


def test_the_models_against_plain_loops(models):
    """every part, weight and count of the model from a loop over all pairs of reads; the part order is the order of (lo, library, flag)"""
    for c in CASES:
        m = models[c["name"]]
        for r in range(c["n_regions"]):
            first, n = int(c["rec"][r, 8]), int(c["rec"][r, 3])
            pairs = []
            for j in range(first, first + n):
                for i in range(j):
                    if c["names"][i] == c["names"][j] and c["region_of"][i] >= 0:
                        pairs.append((int(c["region_of"][i]), (int(c["meta"][j]) >> 8) & 255, int(c["meta"][j]) & 15, int(c["isize"][j])))
            assert int(m["rs"][r, 5]) == len(pairs), (c["name"], r)
            assert int(m["rs"][r, 3]) == sum(1 for p in pairs if p[0] == r), (c["name"], r)
            if m["route"][r] == "big":
                assert sum(p for _, p, _ in m["raw"][r]) == len(pairs)
                continue
            if not pairs:
                assert r not in m["parts"]
                continue
            keys = sorted({p[:3] for p in pairs})
            assert [(k >> 12 & 0x3FFFFFF, (k >> 4) & 255, k & 15) for k, _, _ in m["parts"][r]] == keys, (c["name"], r)
            for (k, cnt, sm), key in zip(m["parts"][r], keys):
                assert cnt == sum(1 for p in pairs if p[:3] == key) and sm == sum(p[3] for p in pairs if p[:3] == key)
                w = sum(1 for p in pairs if p[0] == key[0])
                assert bool(k & ac.WEAK) == (key[0] < r and w < max(c["min_read_pair"], 0)), (c["name"], r, key)
            ins = sorted({p[0] for p in pairs if p[0] < r and sum(1 for q in pairs if q[0] == p[0]) >= max(c["min_read_pair"], 0)})
            assert int(m["rs"][r, 4]) == len(ins)
            if len(ins) <= ac.MAX_IN:
                assert sorted(m["rs"][r, 8:8 + len(ins)].tolist()) == ins
                for e, lo in enumerate(m["rs"][r, 8:8 + len(ins)].tolist()):
                    off, cnt = int(m["rs"][r, 14 + e]), int(m["rs"][r, 17 + e])
                    assert all((k >> 12) & 0x3FFFFFF == lo for k, _, _ in m["parts"][r][off:off + cnt])
                    assert int(m["rs"][r, 11 + e]) == sum(p for _, p, _ in m["parts"][r][off:off + cnt])
        # out_deg: the gate-passing groups that leave a region
        od = np.zeros(c["n_regions"], np.int64)
        for r in range(c["n_regions"]):
            if m["route"][r] != "big":
                for lo in m["rs"][r, 8:8 + min(int(m["rs"][r, 4]), ac.MAX_IN)]:
                    od[lo] += 1
        easy = [r for r in range(c["n_regions"]) if not m["hub"].any()]
        np.testing.assert_array_equal(m["out_deg"][easy], od[easy])


def test_the_aggregate_form_is_the_same_model(models):
    for c in CASES:
        if (c["rec"][:, 3] > 64).any():
            continue
        for split in (1, 2, 5):
            d = ac.as_aggregates(c, split)
            m = ac.groups_model(d)
            np.testing.assert_array_equal(m["rs"][:, :8], models[c["name"]]["rs"][:, :8], err_msg=c["name"])     # (the order of e_lo is the lanes')
            assert m["parts"] == models[c["name"]]["parts"]


def test_the_cases_reach_what_they_are_there_for(models, refs):
    routes, walkers, pair_idx, eidx, old_by, lib_routes, sizes, in_counts = set(), set(), set(), set(), set(), set(), set(), set()
    for c in WALKED:
        m, ref = models[c["name"]], refs[c["name"]]
        routes |= set(m["route"])
        sizes |= {int(x) for x in c["rec"][:, 3]}
        in_counts |= {int(x) for x in m["rs"][:, 4]}
        for v in ac.components(c, m).values():
            if not ac.settles_at_once(c, m, v):
                continue
            w = ac.walker_of(c, m, v)
            walkers.add(w)
            if w == "host":
                continue
            if any(x["from_old"] for x in ref if x["region"][0] in v):
                old_by.add(w)
            for r in v:
                for e in range(int(m["rs"][r, 4])):
                    eidx.add(e)
                    if w == "lane":
                        x, y = v.index(int(m["rs"][r, 8 + e])), v.index(r)
                        pair_idx.add(y - 1 if x == 0 else (y + 1 if x == 1 else 5))
        few = 2 <= c["nlibs"] <= 4 and not c["asm_plain"]
        lib_routes.add("few" if few else ("one" if c["nlibs"] == 1 else "merge"))
    assert routes == {"none", "wave", "fits", "big"}                      # every route of k6_pairs_kernel's per-read side
    assert walkers == {"lane", "wave", "host"} and old_by == {"lane", "wave"}   # both walks, a from-old candidate in each
    assert pair_idx == set(range(6)) and eidx == {0, 1, 2}
    assert lib_routes == {"one", "few", "merge"}
    assert {1, 63, 64, 65, 128, 129} <= sizes and {3, 4} <= in_counts
    assert {c["nkeys"] for c in CASES} >= {1, 2, 16, 17} and {c["nlibs"] for c in CASES} >= {1, 2, 4, 5, 17}
    assert {c["period"] for c in CASES} >= {1, 2, 3} and any(c["period"] > c["n_regions"] for c in CASES)
    assert {c["min_read_pair"] for c in CASES} >= {-1, 0, 1, 2}
    libs = {(int(k) >> 4) & 255 for ps in models["lib-bytes"]["parts"].values() for k, _, _ in ps}
    assert libs == {0, 255}
    agg = ac.as_aggregates(next(c for c in CASES if c["name"] == "many-parts"))
    assert {int(x) for x in np.diff(agg["in_goff"])} >= {0, 1, 64, 65} and set(ac.groups_model(agg)["route"]) == {"none", "wave", "big"}
    sizes_q = ac.quotient_search()
    d32 = np.float32(np.float32(sum(sizes_q)) - np.float32(len(sizes_q)) * np.float32(300.25))
    assert int(float(np.float32(d32 / np.float32(len(sizes_q)))) + 0.5) != int(float(d32) / len(sizes_q) + 0.5)
    flags = {x["flag"] for c in WALKED for x in refs[c["name"]]}
    assert flags >= {ac.NA, ac.FF, ac.LARGE, ac.SMALL, ac.RF, ac.RR, ac.CTX, ac.MATE_UNMAPPED}
    assert any(x["size"] < 0 for c in WALKED for x in refs[c["name"]])
    assert any(np.float32(x["af"]).view(np.uint32) == 0xFFC00000 for x in refs["no-normal-reads"])
    assert any(lam == 1.0e-10 for c in WALKED for x in refs[c["name"]] for _, _, lam in x["terms"])
    assert len(refs["order-key-128"]) == 128 and len(refs["order-key-129"]) == 129
    assert all(x["from_old"] and x["start"] == 39 for x in refs["order-key-129"])
    for name, want in (("big-64-in1", "wave"), ("big-64-in3", "wave"), ("big-65-in1", "host")):      # kK6BigMembers and one more, on the walk they are there for
        c = next(c for c in CASES if c["name"] == name)
        (v,) = ac.components(c, models[name]).values()
        assert len(v) == int(name.split("-")[1]) and ac.settles_at_once(c, models[name], v) and ac.walker_of(c, models[name], v) == want, name
    # more regions than the pairs grid has waves and the lane walk's grid has lanes (the grid-stride loops), at the host count the tests launch with
    assert any(c["n_regions"] > max(ac.launch_grids(c["n_regions"])) for c in WALKED if c["name"].startswith("shapes"))
    m = models["big-64-in3"]
    assert (m["rs"][4:65, 4] == 3).all() and (m["rs"][1:65, 2] > 0).all()    # 64 regions, three incoming groups and a self group each


@pytest.mark.parametrize("slip", ac.WALK_SLIPS)
def test_every_slip_of_the_walk_fails_a_case(refs, slip):
    assert any(ac.differs(refs[c["name"]], ac.walk_reference(c, slip=slip)) for c in WALKED), slip


def test_every_slip_of_the_models_fails_a_case(models):
    for slip in ac.MODEL_SLIPS:
        assert any((ac.groups_model(c, slip=slip)["rs"] != models[c["name"]]["rs"]).any() for c in CASES), slip


def test_a_sequence_number_kept_to_seven_bits_fails_the_129_candidate_case(refs):
    """the keys the walks would write differ in every case; kept to 7 bits, the 129th candidate of the one (window, start) gets the key of
    the first -- and only there"""
    for c in WALKED:
        keys = [k for k in ac.reference_keys(refs[c["name"]]) if k is not None]
        assert len(set(keys)) == len(keys), c["name"]
        short = [k for k in ac.reference_keys(refs[c["name"]], seq_bits=7) if k is not None]
        assert (len(set(short)) != len(short)) == (c["name"] == "order-key-129"), c["name"]


def test_the_holes_of_a_sharded_table_taint_both_regions_of_a_group():
    c = next(c for c in CASES if c["name"] == "shapes-p3-k2-b0")
    d, want = ac.with_holes(c, (2, 13, 23))
    assert np.flatnonzero(want).tolist() == [2, 3, 13, 14, 15, 16, 23, 24]
