"""The cases of tests/test_gpu_classify.py without a GPU (tests/classify_cases.py): the plain restatement of the classifier, the filter
chain and the pass-1 counters against the oracle on every layout, order and option set; the layouts against the tile bodies, slots, wave
halves and record routes they are there for (conditions on the inputs, read off K1's dispatch model and the oracle's class bytes); and the
table's strength: the restatement with each of a list of slips must differ from the oracle somewhere."""
import numpy as np
import pytest

import classify_cases as cc
from helpers import oracle_lib

_RUNS = {}


def oracle(layout, order, opts=()):
    """(class bytes, lib_read_count, bam_read_count, flag_hist, n_svs, SV rows with copy numbers) of one oracle run, kept for the tests
    that share it"""
    key = (layout, order, tuple(sorted(dict(opts).items())))
    if key not in _RUNS:
        run = cc.oracle_run(layout, order, dict(opts))
        d = cc.store(layout, order)
        assert run.n_merged == len(d["tid"])
        if run.nbams > 1:      # positions differ, so the merge of the files is the store itself
            soa = run.merged_soa()
            assert (soa["pos"] == d["pos"]).all() and (soa["lib"] == d["lib"]).all() and (soa["bam"] == d["bam"]).all()
        _RUNS[key] = (run.cls.copy(), run.lib_cnt.copy(), run.bam_cnt.copy(), run.hist.copy(), run.n_svs, int((run.sv_i[:, 14] > 0).sum()) if run.n_svs else 0)
    return _RUNS[key]


def differs(r, o):
    """class bytes (the oracle's six bits) that differ + counters that differ"""
    return int(((r["cls"] & 0x3F) != o[0]).sum()) + int((r["lib_read_count"] != o[1]).sum()) + int((r["bam_read_count"] != o[2]).sum()) + \
        int((r["flag_hist"] != o[3]).sum())


orders_of = cc.orders_of


@pytest.mark.parametrize("layout", list(cc.LAYOUTS))
def test_the_restatement_is_the_oracle(layout):
    spec = cc.LAYOUTS[layout]
    for order in orders_of(layout):
        d = cc.store(layout, order)
        for opts in cc.OPTION_SETS:
            if order not in orders_of(layout, opts):
                continue
            o = oracle(layout, order, opts.items())
            assert o[4] > 0, (layout, order, opts)     # the ready-made records' fields reach SV rows ...
            assert order == "table" or o[5] > 100, (layout, order, opts)     # ... their proper-read counts through the copy numbers
            r = cc.restate(d, cc.lib_params(spec, opts), opts, cc.nbams(spec))
            assert differs(r, o) == 0, (layout, order, opts, np.flatnonzero((r["cls"] & 0x3F) != o[0])[:5])
            np.testing.assert_array_equal(cc.normal_left_bit(o[0], d), (r["cls"] & cc.CLS_NORMAL_LEFT) != 0)


def test_the_per_read_classifier_is_bdo_classify_row_by_row():
    L = oracle_lib()
    t = cc.TABLE
    n = len(t)
    pos = np.full(n, 1000, np.int64)
    d = dict(tid=np.zeros(n, np.int32), pos=pos, mtid=t[:, 2], mpos=pos + t[:, 1], isize=t[:, 3], flag=t[:, 0], bdqual=t[:, 4])
    for k, (_, lo, up, _) in enumerate(cc.LIBS9):
        d["lib"] = np.full(n, k, np.int64)
        raw = cc.restate(d, cc.lib_params(dict(libs=cc.LIBS9)))["raw"]
        lo, up = float(np.float32(lo)), float(np.float32(up))
        want = [L.bdo_classify(int(f), 0, int(mt), 1000, int(1000 + dp), abs(int(isz)), up, lo) for f, dp, mt, isz in t[:, :4].tolist()]
        np.testing.assert_array_equal(raw, np.array(want, np.uint8))


def test_rows_with_secondary_qc_fail_and_supplementary_bits_come_out_as_their_base_rows():
    extra = np.flatnonzero(cc.TABLE[:, 5] >= 0)
    assert len(extra) == 128 and all(((cc.TABLE[extra, 0] & x) != 0).sum() >= 32 for x in (0x100, 0x200, 0x800))
    d = cc.store("mixed", "table")
    cls = oracle("mixed", "table")[0]
    by = {}
    for key, c in zip((d["row"] * 16 + d["lib"]).tolist(), cls.tolist()):
        assert by.setdefault(key, c) == c       # a (row, library) has one class byte wherever it lies
    for e in extra.tolist():
        for lib in range(4):
            assert by[e * 16 + lib] == by[int(cc.TABLE[e, 5]) * 16 + lib]


def test_every_layout_sends_its_tiles_to_the_body_it_is_there_for():
    seen = set()
    for layout, spec in cc.LAYOUTS.items():
        for order in orders_of(layout):
            d = cc.store(layout, order)
            body = cc.tile_body(d, len(spec["libs"]), cc.nbams(spec))
            nfull = len(d["tid"]) // cc.TILE
            if layout in cc.BODY_OF:
                assert (body == cc.BODY_OF[layout]).all(), (layout, order)
            elif layout == "three-bodies":
                assert np.bincount(body, minlength=3).min() >= nfull // 3, (layout, order)
            else:
                assert (body[:nfull] == cc.MIXED).all() and body[nfull:].tolist() == [cc.GENERAL], (layout, order)
                assert len(d["tid"]) - nfull * cc.TILE == spec["tail"]
            seen.update(body.tolist())
            if len(spec["libs"]) > 1 and spec["deal"] == "row":      # several libraries in every full tile
                lib = d["lib"][:nfull * cc.TILE].reshape(nfull, cc.TILE)
                assert ((lib != lib[:, :1]).any(axis=1)).all(), (layout, order)
            if layout == "two-files":
                bam = d["bam"].reshape(nfull, cc.TILE)
                assert ((bam != bam[:, :1]).any(axis=1)).all(), (layout, order)
    assert seen == {cc.UNIFORM, cc.MIXED, cc.GENERAL}


def _reached():
    """[body][slot 0-3, lower half, upper half][row * 4 + library]: where the rows of the four-library layouts lie"""
    reach = np.zeros((3, 6, cc.T * 4), bool)
    for layout in ("uniform", "mixed", "two-files", "three-bodies"):
        spec = cc.LAYOUTS[layout]
        for order in cc.ORDERS:
            d = cc.store(layout, order)
            i = np.arange(len(d["tid"]))
            body = cc.tile_body(d, 4, cc.nbams(spec))[i // cc.TILE]
            key = d["row"] * 4 + d["lib"]
            reach[body, i % 4, key] = True
            reach[body, 4 + ((i % cc.TILE) >= cc.TILE // 2), key] = True
    return reach


def test_every_row_meets_every_library_in_every_body_slot_and_wave_half():
    reach = _reached()
    for b, name in enumerate(cc.BODIES):
        for what in range(6):
            missing = np.flatnonzero(~reach[b, what])
            assert len(missing) == 0, (name, what, len(missing), missing[:5])


@pytest.mark.parametrize("layout", ["uniform", "mixed", "two-files"])
def test_every_passing_anomalous_row_lies_in_a_tile_that_fits_the_ready_made_records_and_in_one_that_does_not(layout):
    """at most kStashCap anomalous reads: K1 leaves the tile's records ready-made; more: K2 compacts the tile from the columns"""
    fits, over = np.zeros(cc.T * 4, bool), np.zeros(cc.T * 4, bool)
    anomalous = np.zeros(cc.T * 4, bool)
    exact = 0
    for order in cc.ORDERS:
        d = cc.store(layout, order)
        c = oracle(layout, order)[0].astype(np.int64)
        an = ((c & cc.CLS_PASS) != 0) & ((c & 14) != cc.NORMAL_FR)
        per = an.reshape(-1, cc.TILE).sum(axis=1)
        exact += int((per == cc.STASH_CAP).sum())
        if order == "table":
            assert per.min() == 0 and per.max() > 100
        per = np.repeat(per, cc.TILE)
        key = d["row"] * 4 + d["lib"]
        anomalous[key[an]] = True
        fits[key[an & (per <= cc.STASH_CAP)]] = True
        over[key[an & (per > cc.STASH_CAP)]] = True
    assert anomalous.sum() > 4000 and exact > 0
    assert (fits == anomalous).all(), np.flatnonzero(fits != anomalous)[:5]
    assert (over == anomalous).all(), np.flatnonzero(over != anomalous)[:5]


def test_the_general_body_meets_tiles_that_fit_the_ready_made_records_with_one_counter_key():
    """nine libraries in one file: the general body with one counter key in the tile, the only way to its own record assembly"""
    for order, lo, hi in (("table", 0, 100), ("spread", cc.STASH_CAP, cc.STASH_CAP), ("perm", cc.STASH_CAP, cc.STASH_CAP + 1)):
        c = oracle("nine-libraries", order)[0].astype(np.int64)
        per = (((c & cc.CLS_PASS) != 0) & ((c & 14) != cc.NORMAL_FR)).reshape(-1, cc.TILE).sum(axis=1)
        assert per.min() <= lo and per.max() >= hi, (order, per.min(), per.max())
        assert order == "table" or ((per > 0) & (per <= cc.STASH_CAP)).sum() > 20, order


def test_every_class_occurs():
    seen = set()
    for layout in ("uniform", "mixed", "two-files"):
        seen.update(np.unique(oracle(layout, "table")[0] & 15).tolist())
    assert seen == set(range(11)) - {cc.NORMAL_RF}
    c = oracle("mixed", "table", dict(illumina_long_insert=1).items())
    assert cc.NORMAL_RF in (c[0] & 15) and c[3][:, cc.ARP_RF].sum() > 0
    # the passing reads' classes: RR is folded into FF, the unmapped classes and NA never pass
    c = oracle("mixed", "table")[0]
    assert set(np.unique(c[(c & cc.CLS_PASS) != 0] & 15).tolist()) == {cc.ARP_FF, cc.ARP_LARGE, cc.ARP_SMALL, cc.ARP_RF, cc.NORMAL_FR, cc.ARP_CTX}


@pytest.mark.parametrize("slip", list(cc.SLIPS))
def test_a_slip_of_the_classifier_differs_from_the_oracle(slip):
    opts = cc.SLIPS[slip]
    spec = cc.LAYOUTS["mixed"]
    d = cc.store("mixed", "table")
    o = oracle("mixed", "table", opts.items())
    assert differs(cc.restate(d, cc.lib_params(spec, opts), opts, 1), o) == 0
    n = differs(cc.restate(d, cc.lib_params(spec, opts), opts, 1, slip=slip), o)
    assert n > 0, slip


def test_the_first_long_insert_line_is_dead_in_the_reference():
    """NORMAL_RF exists only behind the second line, for reads below the upper cutoff: no row of any layout tells whether the first is there"""
    for slip, opts in cc.INVISIBLE_SLIPS.items():
        for layout in ("uniform", "mixed", "two-files", "nine-libraries"):
            spec = cc.LAYOUTS[layout]
            r = cc.restate(cc.store(layout, "table"), cc.lib_params(spec, opts), opts, cc.nbams(spec), slip=slip)
            assert differs(r, oracle(layout, "table", opts.items())) == 0


@pytest.mark.parametrize("slip,layouts", [("mapq_of_slot_0", ("one-library", "uniform", "mixed", "nine-libraries", "two-files")),
                                          ("lib_of_slot_0", ("mixed", "eight-libraries", "nine-libraries", "two-files"))])
def test_a_body_that_takes_slot_0_s_byte_for_the_whole_lane_differs_from_the_oracle(slip, layouts):
    """(applied to the laid-out store: it shows only where the reads of a lane really differ)"""
    for layout in layouts:
        spec = cc.LAYOUTS[layout]
        for order in cc.ORDERS:
            d = cc.lay_out_slip(cc.store(layout, order), slip)
            n = differs(cc.restate(d, cc.lib_params(spec), {}, cc.nbams(spec)), oracle(layout, order))
            assert n > 0, (slip, layout, order)


def test_numpy_class_bytes_keeps_its_six_bits():
    d = cc.store("mixed", "perm")
    spec = cc.LAYOUTS["mixed"]
    lp = cc.lib_params(spec)
    for kw, opts in ((dict(), {}), (dict(opt_t=True), dict(transchr_rearrange=1)), (dict(max_sd=cc.SMALL_MAX_SD), dict(max_sd=cc.SMALL_MAX_SD))):
        got = cc.numpy_class_bytes(d, [l[1] for l in lp], [l[0] for l in lp], [l[2] for l in lp], **kw)
        np.testing.assert_array_equal(got, oracle("mixed", "perm", opts.items())[0])
