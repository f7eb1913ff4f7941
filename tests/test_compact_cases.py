"""The cases of tests/test_gpu_compact.py without a GPU (tests/compact_cases.py): K2's reference against the loop and against the all-pairs
statement; K2's route model against the reference, with and without the ready-made records, under both templates; the cases against the
routes they are there for (read off the model); the finalisation's reference against closed forms; and the cases' strength: each of a list
of slips, applied to a reference or a model, must fail at least one case."""
import numpy as np
import pytest

import compact_cases as cc

PAIRS_MAX = 3000       # reads up to which the O(n^2) statement is made
LOOP_MAX = 20000


def test_the_reference_is_the_loop_and_the_all_pairs_statement():
    loops = pairs = 0
    for c in cc.k2_cases():
        ref = cc.k2_reference(c)
        if c["n"] <= LOOP_MAX:
            assert cc.differs(ref, cc.k2_loop(c)) is None, c["name"]
            loops += 1
        if c["n"] <= PAIRS_MAX:
            assert cc.differs(ref, cc.k2_all_pairs(c), ("idx", "nn", "pk")) is None, c["name"]
            pairs += 1
    assert loops > 60 and pairs > 50


def test_nothing_is_written_at_or_behind_the_capacity():
    for c in cc.k2_cases():
        ref = cc.k2_reference(c)
        written = min(c["cap"], c["count"]) if not c["pre_off"][cc.COL_ANOM] else None
        for f in ("tid", "idx", "nn", "key"):
            a = np.asarray(ref[f]).view(np.uint8).reshape(len(ref[f]), -1)
            if written is not None:
                assert (a[written:] == 0xA5).all(), (c["name"], f)
        pk = ref["pk"].reshape(-1)
        for k in range(c["nkeys"]):
            if written is not None and c["cap"]:
                assert (pk[k * c["cap"] + written:(k + 1) * c["cap"]] == cc.FILL).all(), c["name"]
        if c["cap"]:
            assert (pk[c["nkeys"] * c["cap"]:] == cc.FILL).all(), c["name"]
    caps = {c["name"]: (c["cap"], c["count"]) for c in cc.k2_cases() if c["name"].startswith("cap_")}
    assert caps["cap_count"][0] == caps["cap_count"][1] and caps["cap_count_minus_1"][0] == caps["cap_count"][1] - 1 and caps["cap_count_plus_7"][0] == caps["cap_count"][1] + 7
    assert cc.SLICE < caps["cap_inside_a_slice_round"][0] < 2 * cc.SLICE and caps["cap_1"][0] == 1


def test_the_model_of_k2_is_the_reference():
    for c in cc.k2_cases():
        ref = cc.k2_reference(c)
        t = cc.k1_model(c)
        for stash in (True, False):
            for side in (0, 1):
                assert cc.differs(ref, cc.k2_model(c, stash, side, tables=t)) is None, (c["name"], stash, side)


def test_the_model_of_k1_is_consistent():
    for c in cc.k2_cases():
        t, m = cc.k1_model(c), cc.masks(c)
        nt = c["ntiles"]
        assert int(t["tile_tot"][cc.COL_ANOM].sum()) == c["count"] and not t["tile_tot"][:, nt:].any()
        assert int(t["tile_tot"][cc.COL_KEY0:].sum()) == int(m["proper"].sum())
        written = (t["stash"] != cc.FILL).any(axis=2).sum(axis=1)
        np.testing.assert_array_equal(written, np.minimum(t["tile_tot"][cc.COL_ANOM, :nt], cc.STASH_CAP))
        rec = t["stash"][(t["stash"][:, :, 4] != cc.M32) & (t["stash"][:, :, 4] != cc.FILL)]
        assert not rec[:, 6:].any() and ((rec[:, 4] >> 20) < c["nkeys"]).all()


def routes_of(cases, stash=True, side=0):
    R = {}
    for c in cases:
        cc.k2_model(c, stash, side, routes=R)
    return R


def test_the_cases_reach_what_they_are_there_for():
    C = cc.k2_cases()
    R = routes_of(C)
    assert R["route"] == {"records", "marked", "columns"}
    assert R["rounds"] >= {1, 2, 3, 4}
    assert R["tq"] == {0, 1, 2, 3}
    assert R["rec_key"] == {0, 1}
    assert R["last_key"] >= {0, 1, None}                      # col_prefix for an even and an odd last key, and the runs of one and two keys
    assert {0, 1, 62, 63} <= R["chunk"]
    assert R["seg_edge"] == {"first", "last"}
    both = routes_of(C[:4], side=1)
    assert both["template"] == {"sums"} and R["template"] == {"bases"}
    words = {w % 4 for c in C for w, _ in c["fills"]}
    assert words == {0, 1, 2, 3}
    assert any(w // 4 > 256 * cc.k2_grid(c) for c in C for w, _ in c["fills"])      # more quads than grid threads
    assert {w for c in C for w, _ in c["fills"]} >= {0, 1, 3, 4, 5, 1027}
    assert len({v for c in C if c["name"] == "fills_5_1027_2047_1026" for _, v in c["fills"]}) == 4
    # the record route at its edges
    name = {c["name"]: c for c in C}
    tot = lambda n: cc.k1_model(name[n])["tile_tot"][cc.COL_ANOM]
    assert tot("counts_16_16_16_16")[:4].tolist() == [16] * 4 and tot("counts_16_16_16_17")[:4].tolist() == [16, 16, 16, 17]
    assert routes_of([name["counts_16_16_16_16"]])["route"] == {"records"} and routes_of([name["counts_16_16_16_17"]])["route"] == {"columns"}
    assert routes_of([name["one_marked_among_four"]])["route"] == {"records", "marked", "columns"}
    assert cc.k1_model(name["marked_ragged_end"])["marked"][-1]
    for n, rounds in (("counts_64_64_64_64", 1), ("counts_64_64_64_65", 2), ("counts_128_128_128_128", 2), ("counts_128_128_128_129", 3), ("counts_256_256_256_256", 4)):
        assert routes_of([name[n]], stash=False)["rounds"] == {rounds}
    c = name["lane_0_and_lane_63"]
    m = cc.masks(c)["anom"]
    assert m[0] and m[cc.TILE2 - 1] and m[cc.TILE2] and m[2 * cc.TILE2 - 1]
    t = cc.k1_model(name["tile_counts_0_1_255_256"])
    assert {0, 1, 255, 256} <= set(t["tile_tot"][cc.COL_NORMAL].tolist()) and {0, 1, 256} <= set(t["tile_tot"][cc.COL_KEY0].tolist())
    assert ((t["stash"][:, :, 4] >> 8) & 511 == 255).any()          # the 9-bit field at 255
    assert any(c["ntiles"] % cc.SUB for c in C) and any(c["n"] % cc.PER_LANE for c in C)
    assert any((c["lib"] >= c["nlibs"]).any() and c["nlibs"] > 1 for c in C)
    assert any(len(set(c["lib_key"].tolist())) < c["nlibs"] and c["nkeys"] > 1 for c in C)
    assert {c["nkeys"] for c in C} >= {1, 2, 3, 4, 5, 60}
    assert {len(c["seg"]) - 1 for c in C if c["seg"] is not None} == {1, 2, 3, 17}
    assert any(not c["has_check"] and c["seg"] is not None for c in C) and any(not c["has_check"] and c["seg"] is None for c in C)
    assert all(c["pre_off"].all() for c in C if c["name"].startswith("prefixes_wrap"))
    s = cc.k2_case_named("empty_super_tile_between")
    a = cc.k1_model(s)["tile_tot"][cc.COL_ANOM, :12].reshape(3, 4).sum(axis=1)
    assert a[0] and not a[1] and a[2]
    assert cc.STRIDED_SUPER > cc.K2_GRID_CAP * 4 and (cc.STRIDED_SUPER + cc.ROUND - 1) // cc.ROUND == 9


def _fails(cases, run):
    """the first case that run() fails, the small ones first"""
    return next((c["name"] for c in sorted(cases, key=lambda c: c.get("n", c["ntiles"])) if run(c)), None)


@pytest.mark.parametrize("slip", cc.K2_REFERENCE_SLIPS)
def test_a_slip_of_the_reference_fails_a_case(slip):
    assert _fails(cc.k2_cases(), lambda c: cc.differs(cc.k2_reference(c), cc.k2_reference(c, slip)) is not None)


@pytest.mark.parametrize("slip", cc.INVISIBLE_SLIPS)
def test_what_no_case_can_show(slip):
    assert _fails(cc.k2_cases(), lambda c: cc.differs(cc.k2_reference(c), cc.k2_reference(c, slip)) is not None) is None
    assert all(not (cc.masks(c)["anom"] & cc.masks(c)["nleft"]).any() for c in cc.k2_cases())


@pytest.mark.parametrize("slip", cc.K2_MODEL_SLIPS)
def test_a_slip_of_the_model_fails_a_case(slip):
    def run(c):
        ref, t = cc.k2_reference(c), cc.k1_model(c)
        return any(cc.differs(ref, cc.k2_model(c, stash, side, slip, tables=t)) is not None for stash in (True, False) for side in (0, 1))
    assert _fails(cc.k2_cases(), run)


def test_a_dropped_fill_tail_fails_a_case():
    assert _fails(cc.k2_cases(), lambda c: any(not np.array_equal(a, b) for a, b in zip(cc.fill_model(c), cc.fill_model(c, "fill_tail_dropped"))))


# ---- the finalisation -------------------------------------------------------------------------------------------------------------------------

def test_the_finalisation_reference_against_closed_forms():
    for c in cc.fin_cases():
        r = cc.fin_reference(c)
        nt, ns, cs = c["ntiles"], c["nsuper"], c["chunk_super"]
        tt = c["tile_tot"].astype(np.uint64)
        # a prefix plus the totals of the chunks before is the sum over all earlier tiles, mod 2^32
        for s in sorted({0, 1, ns // 2, ns - 1} & set(range(ns))):
            whole = (tt[:, :s * cc.SUB].sum(axis=1) & cc.M32).astype(np.uint32)
            np.testing.assert_array_equal((r["tile_pre"][:, s] + r["chunk_base"][:, s // cs]).astype(np.uint32), whole, err_msg=c["name"])
        np.testing.assert_array_equal(r["p1"][2:2 + c["ncols"]] if not (c["na_cap"] and r["n_anom"] > c["na_cap"]) else r["p1_host"][2:2 + c["ncols"]],
                                      (tt.sum(axis=1) & cc.M32).astype(np.uint32), err_msg=c["name"])
        assert (r["count_host"][:c["nchunk"]] >> np.uint64(32) == c["stamp"]).all() and (r["count_host"][c["nchunk"]:] == cc.FILL64).all()
        assert int((r["count_host"][:c["nchunk"]] & np.uint64(cc.M32)).sum()) & cc.M32 == int(tt[cc.COL_ANOM].sum()) & cc.M32
        # the fold of the folds is the fold of the whole table, whatever nfold
        one = cc.fin_reference(dict(c, nfold=1))
        np.testing.assert_array_equal(r["p1"][cc.P1_REF_WORD:], one["p1"][cc.P1_REF_WORD:], err_msg=c["name"])
        assert not np.isnan(r["density"][:c["nkeys"]]).any()
        assert (r["p1"][2 + c["ncols"]:cc.P1_REF_WORD] == cc.FILL).all() and not r["p1_host"][2 + c["ncols"]:cc.P1_REF_WORD].any()


def test_the_finalisation_cases_reach_what_they_are_there_for():
    C = {c["name"]: c for c in cc.fin_cases()}
    assert {c["ntiles"] for c in C.values()} >= {0, 1, 3, 4, 5, 16380, 16383, 16384, 16385, 65537, 64 * 16384, 64 * 16384 - 1}
    assert {c["ncols"] for c in C.values()} >= {3, 4, 62} and {c["nfold"] for c in C.values()} >= {1, 2, 64} and {c["nlibs"] for c in C.values()} >= {1, 4, 255}
    assert {c["nsuper"] for c in C.values()} >= {4095, 4096, 4097}
    assert C["chunks_64"]["nchunk"] == 64 and C["chunks_64_one_tile_less"]["nchunk"] == 64 and C["chunks_64_mostly_empty"]["nchunk"] == 64
    r = cc.fin_reference(C["chunks_64_mostly_empty"])
    assert (r["count_host"][2:64] == np.uint64(C["chunks_64_mostly_empty"]["stamp"] << 32)).all()      # an empty chunk's word: the stamp, count 0
    per = lambda c: ((c["ntiles"] + c["nfold"] - 1) // c["nfold"] + 1023) // 1024
    assert per(C["nfold_64_per_1"]) == 1 and per(C["nfold_1_per_2"]) == 2 and per(C["nfold_2_per_2"]) == 2
    wrap = C["columns_4_wrap"]["tile_tot"].astype(np.uint64).sum(axis=1)
    assert (wrap > cc.M32).all()
    wide = cc.fin_reference(C["sums_of_64_bits"])
    assert any(abs(int(s)) > 1 << 33 for s in wide["fold"]["sum"].ravel())
    t = C["ntiles_65537"]["tile_mono"]
    assert (t["ft"][1, 1025 * 3:1025 * 4] == -1).all() and t["ft"][1, 0] == -1 and t["ft"][0, 65536] == -1            # a whole fold slice, the first, the last tile
    ft, lt = t["ft"][0, :65537], t["lt"][0, :65537]
    here = np.flatnonzero(ft != -1)
    joins = lt[here[:-1]] == ft[here[1:]]
    assert joins.any() and not joins.all()                                                                          # a.lt == b.ft and not
    assert cc.fin_reference(C["w_no_deletion_reads_large_w0"])["W"] == 50 and cc.fin_reference(C["w_no_deletion_reads_small_w0"])["W"] == 7
    differ = [n for n, c in C.items() if n.startswith("w_quotient") and cc.fin_reference(c)["W"] != cc.fin_reference(c, "w_double_division")["W"]]
    assert len(differ) >= 3                                                                                         # quotients that float32 rounds across an integer
    assert cc.fin_reference(C["covered_0"])["covered"] == 0 and np.isinf(cc.fin_reference(C["covered_0"])["density"][:2]).all()
    d = cc.fin_reference(C["density_by_library"])
    assert d["density"][2] == np.float32(0.000001) and C["density_by_library"]["cn_lib"] == 1                       # lib_cnt == 0
    for delta, zeroed in ((-1, True), (0, False), (1, False)):
        r = cc.fin_reference(C["na_cap_count%+d" % delta])
        assert (r["p1"][2] == 0) == zeroed and r["p1_host"][2] == r["n_anom"] > 0
    blank = cc.fin_reference(C["ntiles_5"], second_level=False)
    assert (blank["p1"] == cc.FILL).all() and (blank["chunk_base"] == cc.FILL).all() and (blank["chunk_tot"][:, 0] != cc.FILL).all()


@pytest.mark.parametrize("slip", cc.FIN_SLIPS)
def test_a_slip_of_the_finalisation_fails_a_case(slip):
    assert _fails(cc.fin_cases(), lambda c: cc.fin_differs(cc.fin_reference(c), cc.fin_reference(c, slip)) is not None)
