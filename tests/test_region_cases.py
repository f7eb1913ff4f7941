"""The cases of tests/test_gpu_regions.py without a GPU (tests/region_cases.py): the cut reference against the oracle on every case that a
read stream can say; the vectorised restatement against the loop; the join reference against all pairs; the cases against the lanes,
instantiations, bucket routes, probe runs and forward turns they are there for (read off the models); and the cases' strength: each of a
list of slips, applied to a reference or a model copy, must fail at least one case."""
import numpy as np
import pytest

import region_cases as rc
from helpers import make_opts
from runner import oracle_case

STREAMS = [c["name"] for c in rc.cut_cases() if c["stream"]]
LOOP_MAX = 100000         # reads up to which the one-read-at-a-time loop is run


def small_cut_cases():
    return [c for c in rc.cut_cases() if c["n"] <= LOOP_MAX]


def model_join_cases():
    """direct cases the index-order model walks (a name carried by thousands of reads is millions of probes in Python)"""
    return [c for c in rc.join_cases() if c["direct"] and not c["name"].startswith("name_carried_by")]


@pytest.mark.parametrize("name", STREAMS)
def test_the_cut_reference_is_the_oracle(name):
    c = rc.cut_case_named(name)
    config, streams, targets = rc.stream_of(c)
    run = oracle_case(config, streams, targets, make_opts(min_len=c["min_len"], seq_coverage_lim=c["lim"], min_read_pair=1))
    assert run.W == c["W"]
    anomalous = ((run.cls & 0x10) != 0) & ~np.isin(run.cls & 0xF, (6, 7))
    assert int(anomalous.sum()) == c["n"]                      # the stream says the case: these reads and no others enter the accumulator
    regs = run.regions
    if c["min_len"] < 0:      # the empty accumulator the first read breaks passes 0 > min_len: the reference's read-less region 0 (the host adds it, not K3)
        assert regs[0, 1:4].tolist() == [-1, -1, -1] and regs[0, 7] == 0
        regs = regs[1:]
    ref = rc.cut_reference(c)
    assert len(regs) == ref["n_regions"]
    rec = ref["rec"].astype(np.int64)
    want = np.stack([rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 6], rec[:, 3] - rec[:, 4], rec[:, 4], rec[:, 3]], axis=1) if len(rec) else np.zeros((0, 7), np.int64)
    np.testing.assert_array_equal(regs[:, 1:8], want)          # tid, start, end, normal_read_pairs, fwd, rev, n_reads


def test_the_vectorised_restatement_is_the_loop():
    for c in small_cut_cases():
        assert rc.cut_differs(rc.cut_reference(c), rc.cut_vectorised(c)) is None, c["name"]
    assert any(c["n"] > LOOP_MAX for c in rc.cut_cases())      # ... and stands in for it where the loop would take minutes


def test_headout_model_is_the_reference():
    for c in rc.cut_cases():
        np.testing.assert_array_equal(rc.headout_model(c)[0], rc.cut_vectorised(c)["c_maxq"], err_msg=c["name"])


def test_the_join_reference_is_all_pairs():
    checked = 0
    for c in rc.join_cases():
        if c["n"] + c["nf"] > 5000:
            continue
        a, b = rc.join_reference(c), rc.join_all_pairs(c)
        assert a["irregular"] == b["irregular"], c["name"]
        np.testing.assert_array_equal(a["loose"], b["loose"], err_msg=c["name"])
        assert rc.join_differs(a, b) is None, c["name"]
        assert a["irregular"] == c["expect"].get("irregular", 0), c["name"]     # no repeated name: no irregular
        checked += 1
    assert checked >= 25


def test_direct_model_is_the_reference():
    for c in model_join_cases():
        got, seen = rc.direct_model(c)
        assert rc.join_differs(got, rc.join_reference(c)) is None, c["name"]
        for what in ("wrap", "tag_clash", "check_split"):
            if c["expect"].get(what):
                assert seen[what] > 0, (c["name"], what)


def test_mix64_and_its_inverse():
    assert int(rc.mix64(np.uint64(0))) == 0
    # MurmurHash3's 64-bit finaliser: its published test value
    assert int(rc.mix64(np.uint64(1))) == 0xB456BCFC34C2CB2C
    for k in (1, 0xDEADBEEF, (1 << 64) - 1, 0x0123456789ABCDEF):
        assert rc.unmix64(int(rc.mix64(np.uint64(k)))) == k


# ---- the cases against what they are there for --------------------------------------------------------------------------------------

def test_runs_start_and_end_on_lane_0_and_63_under_both_instantiations():
    starts, ends, inst = set(), set(), set()
    for c in rc.cut_cases():
        _, s, e = rc.headout_model(c)
        starts |= s
        ends |= e
        inst.add(rc.instantiation(c))
    assert {0, 63} <= starts and {0, 63} <= ends
    assert inst == {rc.SCAN_BLOCK, 2 * rc.SCAN_BLOCK}
    by = {c["name"]: c for c in rc.cut_cases()}
    assert by["n%d" % rc.TWO_PER_LANE]["n_host"] == rc.TWO_PER_LANE and rc.instantiation(by["n%d" % rc.TWO_PER_LANE]) == rc.SCAN_BLOCK
    assert rc.instantiation(by["n%d" % (rc.TWO_PER_LANE + 1)]) == 2 * rc.SCAN_BLOCK
    assert (rc.TWO_PER_LANE + 513) % (2 * rc.SCAN_BLOCK) == 1               # a last workgroup of the 512-wide one with a single read
    c = by["host_count_above_two_per_lane"]
    assert c["n"] <= rc.TWO_PER_LANE < c["n_host"]


def test_the_run_layouts_are_what_their_names_say():
    for L in (1, 2, 64, 65, 257, 600):
        for how in rc.RUN_LAYOUTS:
            c = rc.cut_case_named("run%d_%s" % (L, how))
            r = rc.cut_reference(c)
            first = rc.run_lead(L, how)
            last = first + L - 1
            firsts = r["c_first"].tolist()
            assert first in firsts and last + 1 in firsts and not set(range(first + 1, last + 1)) & set(firsts)     # the run is one candidate
            if how == "lane0":
                assert first % 64 == 0
            elif how == "end63":
                assert last % 64 == 63
            else:
                edge = 256 if how == "straddle" else 512
                assert first < edge <= last + 1       # the run, or the read that breaks it, lies across the boundary


def test_the_largest_read_length_sits_where_the_case_says():
    for where, counted in (("first", False), ("second", True), ("last", True), ("breaking", True)):
        c = rc.cut_case_named("maxq_" + where)
        r = rc.cut_reference(c)
        k = int(np.flatnonzero(r["c_first"] == 60)[0])
        assert (r["c_maxq"][k] == 60000) == counted, where
    r = rc.cut_reference(rc.cut_case_named("maxq_last_of_list"))
    assert r["last_maxq"] == 60000
    c = rc.cut_case_named("maxq_alone_in_its_wave")
    assert c["n"] == 65 and int(c["qlen"].argmax()) == 64 and rc.cut_reference(c)["c_maxq"].tolist() == [60000]
    c = rc.cut_case_named("maxq_breaking_on_another_chromosome")
    j = int(c["qlen"].argmax())
    assert c["tid"][j] != c["tid"][j - 1] and 60000 in rc.cut_reference(c)["c_maxq"].tolist()


def test_the_edges_of_the_two_tests_are_met():
    c = rc.cut_case_named("gaps_W-1_W_W+1")
    assert {rc.W0 - 1, rc.W0, rc.W0 + 1} <= set(np.diff(c["pos"]).tolist()) and rc.cut_reference(c)["n_cand"] == 2
    c = rc.cut_case_named("chromosome_change_+1_0_negative_far")
    ch = np.flatnonzero(np.diff(c["tid"]) != 0)
    d = np.diff(c["pos"])[ch]
    assert 1 in d and 0 in d and (d < 0).any() and (d > rc.W0).any() and rc.cut_reference(c)["n_cand"] == 5
    for ml in (-1, 0, 7):
        c = rc.cut_case_named("min_len_%d" % ml)
        r = rc.cut_reference(c)
        spans = c["pos"][np.append(r["c_first"][1:], c["n"]) - 1] - c["pos"][r["c_first"]]
        assert {max(ml, 0), ml + 1} <= set(spans.tolist())
        assert [int(x) >= 0 for x in r["c_rid"]] == [int(s) > ml for s in spans]
    for lim in (1, 3, 1000):
        r = rc.cut_reference(rc.cut_case_named("coverage_at_lim_%d" % lim))
        assert (r["c_rid"][:3] >= 0).tolist() == [True, False, False]          # below, exactly at, above the limit


def test_float32_and_exact_verdicts_differ_where_the_cases_say():
    for lim in (1, 3, 1000):
        strict, loose = rc.verdict_pairs(lim)
        for qsum, den in strict:
            assert qsum > 1 << 24 and not rc.accept_f32(qsum, den, lim) and qsum < lim * den and float(qsum) / float(den) < lim
        for qsum, den in loose:
            assert qsum > 1 << 24 and rc.accept_f32(qsum, den, lim) and qsum >= lim * den and float(qsum) / float(den) >= lim
        c = rc.cut_case_named("float32_verdict_lim_%d" % lim)
        got = rc.cut_reference(c)["c_rid"][:len(strict) + len(loose)] >= 0
        assert got.tolist() == [False] * len(strict) + [True] * len(loose)
        for slip in ("div_exact", "div_double"):
            flipped = rc.cut_reference(c, slip)["c_rid"][:len(got)] >= 0
            assert (flipped != got).all(), (lim, slip)
    assert len(rc.verdict_pairs(3)[1]) == 2
    c = rc.cut_case_named("running_sum_past_2^32")
    k = int(np.flatnonzero(c["tid"] == 1)[0])
    assert int(c["qlen"][:k].sum()) > 1 << 32
    assert rc.cut_reference(c)["c_rid"][-2] != rc.cut_reference(c, "div_exact")["c_rid"][-2]


def test_both_bucket_routes_the_wrap_and_the_equal_tags():
    routes = set()
    for c in rc.join_cases():
        for nb, want in (c["routes"] or {}).items():
            got = rc.bucket_routes(c, nb)
            assert got == want, c["name"]
            routes |= {(k, r) for k, r in got.values()}
    assert (4096, "lds") in routes and (4097, "hbm") in routes and (10000, "hbm") in routes
    nbs = set()
    for c in rc.join_cases():
        if c["bucketed"]:
            nbs |= set(c["nbuckets"])
    assert {1, 2, 1024, 2048, 8192} <= nbs
    c = rc.join_case_named("mates_in_different_workgroups")
    assert (np.diff(rc.bucket_offsets(c, 8192)) == 0).any()                  # empty buckets
    c = rc.join_case_named("table_1023_half_full")
    assert c["slots"] == 1024 and c["n"] == 512
    c = rc.join_case_named("equal_tags_on_one_probe_run")
    h = rc.mix64(c["key"][:4])
    assert len(set(c["key"][:4].tolist())) == 4 and len(set((h >> np.uint64(32)).tolist())) == 1 and len(set((h & np.uint64(1023)).tolist())) == 1
    c = rc.join_case_named("wrap_from_the_last_slot")
    assert (rc.mix64(c["key"]) & np.uint64(1023) == np.uint64(1023)).sum() == 10


def test_the_forward_sizes_lie_on_every_edge():
    words = [rc.REC_WORDS * nr for nr in rc.FORWARD_REGIONS]
    assert {w % 4 for w in words if w} == {0, 1, 2, 3} and 0 in words
    assert min(w for w in words if w) // 4 < rc.FWD_BLOCKS * 256               # fewer quads than lanes
    q = {nr: rc.REC_WORDS * nr // 4 for nr in rc.FORWARD_REGIONS}
    assert q[14563] < rc.FWD_TURN_QUADS <= q[14564] and q[29127] < 2 * rc.FWD_TURN_QUADS <= q[29128]
    for nr in rc.FORWARD_REGIONS:
        for w in [rc.REC_WORDS * nr] + [k2 * nr for k2 in rc.FORWARD_NKEYS2]:
            dst, src = rc.forward_model(w)
            np.testing.assert_array_equal(dst, src)


# ---- the cases' strength ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slip", rc.CUT_SLIPS)
def test_a_slip_in_the_cut_fails_a_case(slip):
    failing = [c["name"] for c in small_cut_cases() if c["n"] <= 6000 and rc.cut_differs(rc.cut_reference(c, slip), rc.cut_reference(c)) is not None]
    assert failing, slip


@pytest.mark.parametrize("slip", rc.HEADOUT_SLIPS)
def test_a_slip_in_the_segmented_maximum_fails_a_case(slip):
    failing = [c["name"] for c in rc.cut_cases() if (rc.headout_model(c, slip)[0] != rc.cut_vectorised(c)["c_maxq"]).any()]
    assert failing, slip


@pytest.mark.parametrize("slip", rc.DIRECT_SLIPS)
def test_a_slip_in_the_join_fails_a_case(slip):
    failing = [c["name"] for c in model_join_cases() if rc.join_differs(rc.direct_model(c, slip)[0], rc.join_reference(c)) is not None]
    assert failing, slip


def test_a_slip_in_the_bucket_route_fails_a_case():
    failing = [c["name"] for c in rc.join_cases() for nb, want in (c["routes"] or {}).items() if rc.bucket_routes(c, nb, "bucket_route_ge") != want]
    assert failing == ["bucket_of_4096"]


@pytest.mark.parametrize("slip", ("forward_no_tail_words", "forward_last_turn_dropped"))
def test_a_slip_in_the_forward_fails_a_case(slip):
    failing = [nr for nr in rc.FORWARD_REGIONS if (rc.forward_model(rc.REC_WORDS * nr, slip)[0] != rc.forward_model(rc.REC_WORDS * nr, slip)[1]).any()]
    assert failing, slip
