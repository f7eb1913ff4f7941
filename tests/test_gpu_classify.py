"""K1's three tile bodies (csrc/k1_classify.hip: the usual tile of one library and one file, the tile of several libraries in one file,
the general body) against the oracle on the classifier truth table of tests/classify_cases.py: every combination of the flag bits the
classifier reads, both mate geometries, |isize| either side of every cutoff, of -m and of 2^24, mapping qualities either side of every
minimum -- laid out so that every row meets every library in every body, slot of a lane and half of the wave, in tiles that fit K1's
ready-made records for K2 and in tiles that do not.  tests/test_classify_cases.py holds those conditions and the table's strength
without a GPU.  Here: the whole product against ONE oracle run per case (class bytes, counters, W, ref_len, regions, every SV field),
bit 6 of the class byte, the runs without ready-made records, bdx_classify, indices out of range and a sharded run."""
import functools

import numpy as np
import pytest

import classify_cases as cc
from runner import compare, product_from_oracle, product_options, sharded_from_oracle

import breakdancer_amd as bda
from breakdancer_amd import api
from breakdancer_amd.api import LibraryConfig

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=3)
def oracle(layout, order, opts=()):
    run = cc.oracle_run(layout, order, dict(opts))
    assert run.n_svs > 0
    return run


def library_configs(run, one_file=False):
    return [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]),
                          bam_file_index=0 if one_file else int(run.lib_i[i, 1]), name=run.lib_names[i]) for i in range(run.nlibs)]


def product(run, soa, **debug):
    """runner.product_from_oracle with the store given (the oracle's merged stream, or one that differs from it on purpose) and debug switches"""
    bd = bda.BreakDancer(product_options(run.opts), library_configs(run), run.nbams, ntids=0, max_read_window_size=run.w0)
    for name, value in debug.items():
        bd.set_debug(name, value)
    bd.push_reads(soa)
    bd.run()
    return bd


def check_class_bytes(run, bd, d, layout):
    """the full byte: bit 6 from the oracle's own byte (pass & NORMAL_* & pos < mpos), and the whole of it against the restatement"""
    cls = bd.read_class()
    np.testing.assert_array_equal(cls & 0x3F, run.cls)
    np.testing.assert_array_equal((cls & cc.CLS_NORMAL_LEFT) != 0, cc.normal_left_bit(run.cls, d))
    assert not (cls & 0x80).any()
    spec = cc.LAYOUTS[layout]
    np.testing.assert_array_equal(cls, cc.restate(d, cc.lib_params(spec, run.opts), run.opts, cc.nbams(spec))["cls"])


# every layout under every option set, the order going round; and every layout in every order under the default options
def _order(layout, i, j):
    orders = cc.orders_of(layout, cc.OPTION_SETS[j])
    return orders[(i + j) % len(orders)]


PARITY = [(layout, _order(layout, i, j), j) for i, layout in enumerate(cc.LAYOUTS) for j in range(len(cc.OPTION_SETS))]
PARITY += [(layout, order, 0) for layout in cc.LAYOUTS for order in cc.orders_of(layout) if (layout, order, 0) not in PARITY]


@pytest.mark.parametrize("layout,order,k", PARITY, ids=["%s-%s-%d" % c for c in PARITY])
def test_the_product_equals_the_oracle_on_the_truth_table(layout, order, k):
    opts = cc.OPTION_SETS[k]
    run = oracle(layout, order, tuple(opts.items()))
    d = cc.store(layout, order)
    bd = product_from_oracle(run)
    compare(run, bd)
    check_class_bytes(run, bd, d, layout)
    bd.close()
    if order == "perm":     # the same store without K1's ready-made records: K2 compacts every tile from the columns
        bd = product(run, run.merged_soa(), no_stash=1)
        compare(run, bd)
        check_class_bytes(run, bd, d, layout)
        bd.close()


@pytest.mark.parametrize("layout", ["mixed", "two-files"])
def test_bdx_classify_equals_the_context_route_in_the_full_byte(layout):
    """api.classify (bdx_classify: a context of its own, the file count taken from the batch) on the first 1, 255, 256 and 257 records
    of the permuted store, against read_class() of a context built with the layout's own file count, and against the restatement"""
    spec = cc.LAYOUTS[layout]
    run = oracle(layout, "perm")
    full = cc.store(layout, "perm")
    for opts in (cc.OPTION_SETS[0], cc.OPTION_SETS[1], cc.OPTION_SETS[3]):
        orun = type("O", (), dict(opts=dict(run.opts, **opts), lib_f=run.lib_f, lib_i=run.lib_i, lib_names=run.lib_names, nlibs=run.nlibs,
                                  nbams=run.nbams, w0=run.w0))
        for n in (1, 255, 256, 257):
            d = {k: v[:n] for k, v in full.items()}
            got = api.classify(product_options(orun.opts), library_configs(run, one_file=True), d)
            bd = product(orun, d)
            np.testing.assert_array_equal(got, bd.read_class())
            bd.close()
            np.testing.assert_array_equal(got, cc.restate(d, cc.lib_params(spec, opts), opts, cc.nbams(spec))["cls"])


def test_library_and_file_indices_out_of_range_count_as_0_in_all_three_bodies():
    """bdx_push takes the index columns as they come; K1's comment says an index out of range counts as 0 in all three bodies (K2, K9
    and the query kernels say the same of the library).  Tiles of every body get libraries >= nlibs where the oracle's store has library
    0 and files >= nbams where it has file 0; everything must come out as from the oracle's store"""
    layout = "three-bodies"
    spec = cc.LAYOUTS[layout]
    for order, opts in (("table", {}), ("spread", dict(cn_lib=1, print_af=1)), ("perm", {})):
        run = oracle(layout, order, tuple(opts.items()))
        d = cc.store(layout, order)
        soa = run.merged_soa()
        lib, bam = soa["lib"].astype(np.int64), soa["bam"].astype(np.int64)
        tile = np.arange(len(lib)) // cc.TILE
        hit = (tile % 2 == 0)                                   # (every other tile: the three bodies come round every three tiles)
        lib = np.where(hit & (lib == 0), 4 + (tile * 7) % 252, lib)     # one value per tile, 4 ... 255: a uniform tile stays uniform
        bam = np.where(hit & (bam == 0), 2 + (tile * 5) % 254, bam)     # 2 ... 255: a tile of one file stays one
        raw = dict(soa, lib=lib.astype(np.uint8), bam=bam.astype(np.uint8))
        before, after = cc.tile_body(soa, 4, 2), cc.tile_body(raw, 4, 2)
        np.testing.assert_array_equal(before, after)
        for body in (cc.UNIFORM, cc.MIXED, cc.GENERAL):
            changed = ((raw["lib"] != soa["lib"]) | (raw["bam"] != soa["bam"])).reshape(-1, cc.TILE).any(axis=1)
            assert (changed & (after == body)).sum() > 20
        assert (raw["lib"] >= 4).sum() > 1000 and (raw["bam"] >= 2).sum() > 1000
        r = cc.restate(raw, cc.lib_params(spec, opts), opts, 2)
        np.testing.assert_array_equal(r["cls"] & 0x3F, run.cls)
        np.testing.assert_array_equal(r["lib_read_count"], run.lib_cnt)
        np.testing.assert_array_equal(r["bam_read_count"], run.bam_cnt)
        for debug in (dict(), dict(no_stash=1)):
            bd = product(run, raw, **debug)
            compare(run, bd)
            check_class_bytes(run, bd, d, layout)
            bd.close()


def test_a_sharded_run_over_the_permuted_table():
    """K9 takes its totals from these class bytes again"""
    run = oracle("mixed", "perm")
    compare(run, sharded_from_oracle(run, world=2), check_cls=False)
