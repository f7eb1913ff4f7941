"""GPU tests of --estimate: KH (bdx_insert_size_histogram) against a brute-force numpy restatement, exact, on every way into the store;
bdx_set_libs / bdx_dist_set_libs against contexts created with the new libraries; and the CLI on the chr21 fixture.

All counts are integers, so every histogram comparison is for equality.  Stores are as small as the code paths allow: record counts around
the 256-record tile, one store of ~300 k records (293 workgroups, one tile per wave) and the 1.2 M records of the set_libs tests (more
tiles than the 1,024 persistent workgroups' waves: the grid-stride loop), library counts that give each library 8192, 4096, 2048, 910, 409
and 32 LDS bins, values inside and outside those windows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import estimate_cases as ec
from helpers import GOLDEN, ROOT, assert_same, filter_cmd_lines, load_chr21, make_opts, snapshot

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHR21 = os.path.join(GOLDEN, "chr21")
BINS = ec.BINS
ISIZE_EDGES = (-1, 0, 1, BINS - 1, BINS, 2**31 - 1)


def libs_of(nlibs, minq=None, nbams=1):
    from breakdancer_amd.api import LibraryConfig
    return [LibraryConfig(400.0, 30.0, 490.0, 310.0, 100.0, min_mapping_quality=-1 if minq is None else int(minq[i]), bam_file_index=i % nbams)
            for i in range(nlibs)]


def new_ctx(nlibs, minq=None, opts=None):
    import breakdancer_amd as bda
    from breakdancer_amd.api import Options
    return bda.BreakDancer(opts or Options(), libs_of(nlibs, minq), 1, max_read_window_size=200)


def resolved(nlibs, minq):
    return [35 if minq is None or minq[i] < 0 else int(minq[i]) for i in range(nlibs)]


def store(n, nlibs, seed, minq=None, centre=400, spread=30, lib_values=None):
    """n records on one sequence in position order: two thirds of them observations-to-be around `centre`, the rest drawn from the flag
    truth table, the isize edges and qualities at the library's minimum and one above it"""
    rng = np.random.default_rng(seed)
    q = np.asarray(resolved(nlibs, minq))
    lib = rng.integers(0, nlibs, n) if lib_values is None else rng.choice(np.asarray(lib_values), n)
    ql = q[np.where(lib < nlibs, lib, 0)]
    flag = np.where(rng.random(n) < 0.66, 0x3 | np.where(rng.random(n) < 0.5, 0x10, 0x20),
                    rng.choice(np.array([0x1, 0x2, 0x4, 0x8, 0x400, 0x10]), (n, 6)).sum(axis=1) if n else 0).astype(np.uint16)
    isize = np.rint(rng.normal(centre, spread, n)).astype(np.int64) * np.where(rng.random(n) < 0.5, 1, -1)
    e = rng.random(n) < 0.05
    isize = np.where(e, rng.choice(np.array(ISIZE_EDGES), n), isize)
    mapq = np.clip(np.where(rng.random(n) < 0.3, ql, np.where(rng.random(n) < 0.5, ql + 1, 60)), 0, 255)
    mtid = np.where(rng.random(n) < 0.04, 1, 0)
    pos = np.sort(rng.integers(0, 40_000_000, n))
    return dict(tid=np.zeros(n, np.int32), pos=pos.astype(np.int32), mtid=mtid.astype(np.int32), mpos=(pos + 300).astype(np.int32),
                isize=isize.astype(np.int32), flag=flag, qlen=np.full(n, 100, np.uint16), mapq=mapq.astype(np.uint8),
                lib=lib.astype(np.uint8), bam=np.zeros(n, np.uint8), name_key=rng.integers(1, 2**62, n).astype(np.uint64))


def check_store(soa, nlibs, minq=None, bd=None):
    own = bd is None
    if own:
        bd = new_ctx(nlibs, minq)
        if len(soa["tid"]):
            bd.push_reads(soa)
    hist, over = bd.insert_size_histogram()
    want_h, want_o = ec.observations(soa, nlibs, resolved(nlibs, minq))
    np.testing.assert_array_equal(over, want_o)
    np.testing.assert_array_equal(hist, want_h)
    if own:
        bd.close()
    return want_h, want_o


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
@pytest.mark.parametrize("nlibs", [1, 2])
def test_histogram_at_tile_edges(n, nlibs):
    check_store(store(n, nlibs, seed=100 + n), nlibs, minq=None if nlibs == 1 else [20, 50])


@pytest.mark.parametrize("nlibs", [1, 2, 4, 9])
def test_histogram_of_300k_records(nlibs):
    minq = None if nlibs == 1 else [(7 * i) % 61 for i in range(nlibs)]
    h, o = check_store(store(300_007, nlibs, seed=nlibs, minq=minq), nlibs, minq)
    assert h.sum() > 50_000 and o.sum() > 100 and (h.sum(axis=1) > 1000).all()


def test_histogram_of_255_libraries():
    minq = [(11 * i) % 70 for i in range(255)]
    h, _ = check_store(store(20_000, 255, seed=255, minq=minq, centre=40, spread=30), 255, minq)   # (32 LDS bins each: both routes)
    assert (h.sum(axis=1) > 0).sum() > 240


def test_histogram_of_20_libraries_with_windows_around_their_means():
    """from nine libraries on a library's LDS window no longer starts at 0: with 20 libraries of mean 400 it is [196, 605), so inserts
    around 400 are counted in LDS at an offset and the edge values on the global route"""
    minq = [(13 * i) % 50 for i in range(20)]
    h, _ = check_store(store(120_000, 20, seed=20, minq=minq, centre=400, spread=90), 20, minq)
    assert (h[:, 196:605].sum(axis=1) > 500).all() and (h[:, :196].sum(axis=1) > 5).all() and (h[:, 605:].sum(axis=1) > 5).all()


def test_one_library_never_reads_the_lib_column():
    s = store(3000, 1, seed=5)
    s["lib"] = np.full(3000, 7, np.uint8)        # (not copied with one library; the restatement ignores it too)
    check_store(s, 1)


def test_library_index_out_of_range_is_library_0():
    s = store(4000, 3, seed=6, minq=[10, 40, 60], lib_values=[0, 1, 2, 3, 200, 255])
    h, _ = check_store(s, 3, [10, 40, 60])
    assert h[0].sum() > h[1].sum() + h[2].sum()


def test_truth_table_of_flags_isizes_and_qualities():
    rows = []
    minq = [30, 45]
    for bits in range(128):
        flag = sum(b for k, b in enumerate((0x1, 0x2, 0x4, 0x8, 0x400, 0x10)) if bits >> k & 1)
        for isize in ISIZE_EDGES:
            for lib in (0, 1):
                for dq in (0, 1):
                    rows.append((flag, bits >> 6 & 1, isize, lib, minq[lib] + dq))
    r = np.array(rows, dtype=np.int64)
    n = len(r)
    soa = dict(tid=np.zeros(n, np.int32), pos=np.arange(n, dtype=np.int32), mtid=r[:, 1].astype(np.int32), mpos=np.arange(n, dtype=np.int32),
               isize=r[:, 2].astype(np.int32), flag=r[:, 0].astype(np.uint16), qlen=np.full(n, 100, np.uint16), mapq=r[:, 4].astype(np.uint8),
               lib=r[:, 3].astype(np.uint8), bam=np.zeros(n, np.uint8), name_key=np.arange(1, n + 1, dtype=np.uint64))
    h, o = check_store(soa, 2, minq)
    # of the 128 flag / mtid rows exactly two are observations (0x10 either way); of the isizes -1 is none and two lie beyond the bins
    for lib in (0, 1):
        assert h[lib].sum() == 2 * 3 and o[lib] == 2 * 2
        assert [int(h[lib][x]) for x in (0, 1, BINS - 1)] == [2, 2, 2]


def test_100000_equal_observations():
    n = 100_000
    s = store(n, 1, seed=8)
    s["flag"][:] = 0x23
    s["isize"][:] = 377
    s["mtid"][:] = 0
    s["mapq"][:] = 60
    h, _ = check_store(s, 1)
    assert h[0][377] == n


def test_values_around_30000_in_nine_libraries():
    s = store(60_000, 9, seed=9, centre=30_000, spread=200)     # (far outside every library's 910 LDS bins)
    h, _ = check_store(s, 9)
    # (of 60,000 records about 0.66 * 0.5 * 0.7 are observations: proper flags, a positive isize, a quality above the minimum)
    assert h[:, 29_000:31_000].sum() > 10_000 and (h[:, 29_000:31_000].sum(axis=1) > 800).all()


# ---- the ways in ----------------------------------------------------------------------------------------------------------------

def test_adopted_device_arrays():
    from breakdancer_amd.api import BATCH_FIELDS
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    n, nlibs, minq = 70_001, 4, [0, 35, 36, 59]
    s = store(n, nlibs, seed=12, minq=minq)
    dev, ptrs = [], {}
    for k, dt in BATCH_FIELDS:
        a = np.ascontiguousarray(s[k], dtype=dt)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        dev.append(p)
        ptrs[k] = p.value
    bd = new_ctx(nlibs, minq)
    bd.set_device_reads(ptrs, n)
    check_store(s, nlibs, minq, bd=bd)
    bd.close()
    for p in dev:
        hip.hipFree(p)


def test_staged_batches_and_a_call_before_and_after_the_run():
    from breakdancer_amd.synth import make_chromosome
    s = make_chromosome(n_pairs=20_000, length=3_000_000, seed=3)
    bd = new_ctx(1)
    bd.stream_reads(s, batch=7000)
    before = check_store(s, 1, bd=bd)
    bd.run()
    after = bd.insert_size_histogram()
    np.testing.assert_array_equal(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])
    assert before[0].sum() > 15_000
    bd.close()


def test_records_decoded_on_the_device(tmp_path):
    from breakdancer_amd import bamdec
    from breakdancer_amd.bamwrite import write_bam
    from breakdancer_amd.synth import make_chromosome
    s = make_chromosome(n_pairs=6000, length=1_000_000, seed=4)
    bam = str(tmp_path / "small.bam")
    write_bam(bam, s, ["chrS"], seed=1)
    bd = new_ctx(1)
    _, _, stats = bamdec.decode_file(bam, rg_ids=["rg1"], rg_lib=[0], sink=bd)
    check_store(s, 1, bd=bd)
    bd.close()


# ---- bdx_set_libs ----------------------------------------------------------------------------------------------------------------

LIB_B = dict(mean_insertsize=395.0, std_insertsize=25.0, uppercutoff=452.0, lowercutoff=348.0, readlens=100.0)
W_A, W_B = 200, 195


def ctx_with(lib, w0):
    import breakdancer_amd as bda
    from breakdancer_amd.api import LibraryConfig, Options
    return bda.BreakDancer(Options(), [LibraryConfig(**lib)], 1, max_read_window_size=w0)


def push_in(bd, s, cuts):
    edges = [0] + list(cuts) + [len(s["tid"])]
    for lo, hi in zip(edges[:-1], edges[1:]):
        bd.push_reads({k: v[lo:hi] for k, v in s.items()})


@pytest.fixture(scope="module")
def big_store():
    """1,200,000 records, the result of a fresh context created with libraries B, and the class bytes of one created with A"""
    from breakdancer_amd.synth import LIB_C2, make_chromosome
    s = make_chromosome(n_pairs=600_000, length=60_000_000, seed=21)
    out = []
    for lib, w0 in ((LIB_B, W_B), (LIB_C2, W_A)):
        bd = ctx_with(lib, w0)
        bd.push_reads(s)
        bd.run()
        out.append(snapshot(bd))
        bd.close()
    return s, out[0], out[1]["cls"]


def test_histogram_of_the_1200000_record_store(big_store):
    """4,688 tiles for 1,024 workgroups of four waves: some waves take a second tile (the grid-stride loop)"""
    s = big_store[0]
    assert (len(s["tid"]) + 255) // 256 > 1024 * 4
    h, _ = check_store(s, 1)
    assert h.sum() > 500_000


@pytest.mark.parametrize("route", ["push", "stream"])
def test_set_libs_behind_a_live_classifier_equals_a_fresh_context(big_store, route):
    """The store is reserved up front, as the CLI does, so that no batch grows it (a grown store drops the live pass 1 by itself): the first
    batch completes at least 4,096 tiles and the classifier has run over them under libraries A when bdx_set_libs arrives.  Were the live
    pass 1 kept, those tiles' class bytes would stay A's, and they differ from B's (asserted below)."""
    from breakdancer_amd.api import LibraryConfig
    from breakdancer_amd.synth import LIB_C2
    s, ref, cls_a = big_store
    first = 4096 * 256
    assert not np.array_equal(cls_a[:first], ref["cls"][:first])
    bd = ctx_with(LIB_C2, W_A)
    bd._chk(bd.lib.bdx_reserve(bd.h, len(s["tid"])), "bdx_reserve")
    if route == "push":
        push_in(bd, s, (1_100_000, 1_150_000))     # 4,296 whole tiles in the first batch
    else:
        bd.stream_reads(s, batch=first)            # the staged route (bdx_acquire_batch / bdx_submit_batch): 4,096 tiles in the first batch
    bd.set_libs([LibraryConfig(**LIB_B)], W_B)
    bd.run()
    assert_same(snapshot(bd), ref)
    bd.close()
    assert ref["summary"]["n_svs"] > 0


def test_run_set_libs_run_again(big_store):
    from breakdancer_amd.api import LibraryConfig
    from breakdancer_amd.synth import LIB_C2
    s, ref, cls_a = big_store
    bd = ctx_with(LIB_C2, W_A)
    bd.push_reads(s)
    bd.run()
    a = snapshot(bd)
    np.testing.assert_array_equal(a["cls"], cls_a)
    assert not np.array_equal(a["cls"], ref["cls"])            # (the two sets of cutoffs do tell reads apart)
    bd.set_libs([LibraryConfig(**LIB_B)], W_B)
    with pytest.raises(Exception):
        bd.summary()                                            # (the finished run belonged to libraries A)
    bd.run()
    assert_same(snapshot(bd), ref)
    bd.close()


def test_set_libs_on_1000_records():
    from breakdancer_amd.api import LibraryConfig
    from breakdancer_amd.synth import LIB_C2, make_chromosome
    s = make_chromosome(n_pairs=500, length=200_000, seed=22, discordant=0.1)
    fresh = ctx_with(LIB_B, W_B)
    fresh.push_reads(s)
    fresh.run()
    bd = ctx_with(LIB_C2, W_A)
    push_in(bd, s, (300, 700))
    bd.set_libs([LibraryConfig(**LIB_B)], W_B)
    bd.run()
    assert_same(snapshot(bd), snapshot(fresh))
    bd.close()
    fresh.close()


def test_set_libs_on_the_chr21_store_equals_the_oracle():
    """(The issue asks for the oracle comparison on the 1,000-record synthetic store; it is made on the chr21 fixture instead, the store the
    oracle harness of the other parity tests reads -- records, read groups and configuration text -- and through runner.compare, which
    holds every table to the oracle.  test_set_libs_on_1000_records compares the synthetic store with a fresh context.)
    The product created with the fixture's configuration, then given other cutoffs: what the oracle computes from a configuration
    that states those cutoffs"""
    import re
    import breakdancer_amd as bda
    import runner
    from breakdancer_amd.api import LibraryConfig
    opts = make_opts()
    text_a = open(os.path.join(CHR21, "inv_del_bam_config")).read()
    text_b = re.sub(r"lower:[0-9.]+\tupper:[0-9.]+\tmean:[0-9.]+\tstd:[0-9.]+", "lower:371.88\tupper:501.50\tmean:466.86\tstd:22.53", text_a)
    assert text_b != text_a

    def with_text(text):
        import helpers
        run = helpers.OracleRun(text, opts)
        base = load_chr21(opts)
        run.set_targets(base.targets)
        for b, ((targets, recs), nid) in enumerate(zip(base.decoded, helpers.name_ids(*[d[1]["name"] for d in base.decoded]))):
            r = dict(recs)
            r["lib"] = np.array([run.lib_of_rg(g) for g in recs["rg"]], dtype=np.int32)
            r["name_id"] = nid
            run.set_stream(b, r)
        return run

    def libs_from(run):
        return [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]),
                              name=run.lib_names[i]) for i in range(run.nlibs)]
    run_a, run_b = with_text(text_a), with_text(text_b)
    run_a.run()
    run_b.run()
    bd = bda.BreakDancer(runner.product_options(opts), libs_from(run_a), run_a.nbams, ntids=0, max_read_window_size=run_a.w0)
    bd.push_reads(run_a.merged_soa())
    bd.set_libs(libs_from(run_b), run_b.w0)
    bd.run()
    runner.compare(run_b, bd)
    bd.close()


def test_argument_and_state_errors():
    from breakdancer_amd import _lib as L
    from breakdancer_amd.api import lib_array
    lib = L.load()
    bd = new_ctx(2)
    two = lib_array(libs_of(2))
    hist, over = np.zeros((2, BINS), np.uint64), np.zeros(2, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.bdx_insert_size_histogram(None, p(hist), p(over)) == 1
    assert lib.bdx_insert_size_histogram(bd.h, None, p(over)) == 1
    assert lib.bdx_insert_size_histogram(bd.h, p(hist), None) == 1
    hist[:] = 7
    over[:] = 7
    assert lib.bdx_insert_size_histogram(bd.h, p(hist), p(over)) == 0 and not hist.any() and not over.any()    # an empty store: zeros
    assert lib.bdx_set_libs(None, two, 2, 200) == 1
    assert lib.bdx_set_libs(bd.h, None, 2, 200) == 1
    assert lib.bdx_set_libs(bd.h, two, 1, 200) == 1 and lib.bdx_set_libs(bd.h, lib_array(libs_of(3)), 3, 200) == 1
    moved = lib_array(libs_of(2))
    moved[1].bam_index = 1
    assert lib.bdx_set_libs(bd.h, moved, 2, 200) == 1                  # the key map cannot move
    assert lib.bdx_set_libs(bd.h, two, 2, 200) == 0
    # the class bytes of a finished run belong to the old libraries: the query calls refuse until the next run
    from breakdancer_amd.synth import make_chromosome
    bd.push_reads(make_chromosome(n_pairs=1000, length=200_000, seed=30))
    bd.run()
    iv = np.zeros(1, dtype=L.INTERVAL_DTYPE)
    iv["end"] = 1000
    out = np.zeros(1, np.uint32)
    assert lib.bdx_count_interval_reads(bd.h, p(iv), 1, 0, p(out)) == 0
    assert lib.bdx_set_libs(bd.h, two, 2, 200) == 0
    assert lib.bdx_count_interval_reads(bd.h, p(iv), 1, 0, p(out)) == 4
    bd.run()
    assert lib.bdx_count_interval_reads(bd.h, p(iv), 1, 0, p(out)) == 0
    bd.close()


# ---- sharded ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_genome():
    from breakdancer_amd.synth import concat, make_chromosome
    parts = [make_chromosome(n_pairs=4000 + 500 * t, length=1_500_000, seed=40 + t, tid=t, name_base=t << 36, discordant=0.05) for t in range(4)]
    return concat(parts), parts


def table_of(bd):
    svs, (li, lp), (ck, cv) = bd.svs()
    return dict(summary=bd.summary(), svs=svs, sv_lists=(li, lp, ck, cv), regions=bd.regions(), counters=bd.counters(), cls=np.zeros(0, np.uint8))


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_histograms_sum_and_set_libs_equals_a_run_created_with_them(small_genome, world):
    from breakdancer_amd import dist as D
    from breakdancer_amd.api import LibraryConfig, Options
    from breakdancer_amd.shard import plan_chromosomes
    from breakdancer_amd.synth import LIB_C2
    whole, parts = small_genome
    single = ctx_with(LIB_C2, W_A)
    single.push_reads(whole)
    want = single.insert_size_histogram()
    single.close()

    def fed(lib, w0):
        ranks = D.DistRun.threads(Options(), [LibraryConfig(**lib)], 1, len(parts), w0, [0] * world)
        for r, tids in enumerate(plan_chromosomes({t: len(p["tid"]) for t, p in enumerate(parts)}, world)):
            for t in tids:
                ranks[r].chromosome(t).push_reads(parts[t])
        return ranks
    ranks = fed(LIB_C2, W_A)
    hs = [r.insert_size_histogram() for r in ranks]
    assert all(h[0].sum() > 0 for h in hs)
    np.testing.assert_array_equal(sum(h[0] for h in hs), want[0])
    np.testing.assert_array_equal(sum(h[1] for h in hs), want[1])
    for r in ranks:
        r.set_libs([LibraryConfig(**LIB_B)], W_B)
    got = table_of(D.run_threads(ranks))
    ranks_b = fed(LIB_B, W_B)
    ref = table_of(D.run_threads(ranks_b))
    assert_same(got, ref)
    assert ref["summary"]["n_svs"] > 0
    for r in ranks + ranks_b:
        r.close()


# ---- the CLI on chr21 --------------------------------------------------------------------------------------------------------------

def run_cli(args, cfg="inv_del_bam_config", env=None):
    p = subprocess.run([EXE] + args + [cfg], cwd=CHR21, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode(), p.stderr.decode()


@pytest.fixture(scope="module")
def estimated(tmp_path_factory):
    """the --estimate run on chr21 with default options, its stdout and the configuration it wrote"""
    cfg = str(tmp_path_factory.mktemp("est") / "out.cfg")
    out, err = run_cli(["--estimate", "--estimate-config", cfg], env=dict(BDX_TIMING="1"))
    return out, err, cfg


def test_cli_estimate_equals_a_plain_run_on_the_written_configuration(estimated, tmp_path):
    out, err, cfg = estimated
    plain, _ = run_cli([], cfg=cfg)
    assert filter_cmd_lines(out) == filter_cmd_lines(plain)
    assert "[bdx timing] --estimate: library H_IJ-NA19238-NA19238-extlibs: n=1279 n_over=0 n_kept=1279 " in err and " valid" in err
    cfg2 = str(tmp_path / "out2.cfg")
    out2, _ = run_cli(["-a", "-h", "--estimate", "--estimate-config", cfg2])
    plain2, _ = run_cli(["-a", "-h"], cfg=cfg2)
    assert filter_cmd_lines(out2) == filter_cmd_lines(plain2)
    assert open(cfg2).read() == open(cfg).read()
    assert filter_cmd_lines(out) != filter_cmd_lines(run_cli([])[0])       # (the fixture's own configuration gives another table)


def test_cli_library_statistics_carry_the_restatements_values(estimated):
    from test_estimate import chr21_histograms
    out, _, _ = estimated
    _, names, hists, _ = chr21_histograms()
    lines = [l for l in out.split("\n") if l.startswith("#") and "\tlibrary:" in l]
    assert len(lines) == 2
    for n in names:
        vals, _, _ = ec.run_libraries(ec.restate(hists[n]), 3)
        line = [l for l in lines if "\tlibrary:%s\t" % n in l][0]
        assert "\tmean:%g\tstd:%g\tuppercutoff:%g\tlowercutoff:%g\t" % (vals["mean"], vals["std"], vals["upper"], vals["lower"]) in line, line


def test_cli_estimate_with_the_host_decoder_and_sharded(estimated):
    out, _, _ = estimated
    assert filter_cmd_lines(run_cli(["--estimate"], env=dict(BDX_DECODE="host"))[0]) == filter_cmd_lines(out)
    assert filter_cmd_lines(run_cli(["--estimate"], env=dict(BDX_GPUS="0,0"))[0]) == filter_cmd_lines(out)


def test_cli_ci_window_defaults_to_the_estimated_cutoff(tmp_path):
    vcf = str(tmp_path / "o.vcf")
    run_cli(["--estimate", "--vcf", vcf, "--ci"])
    head = [l for l in open(vcf).read().split("\n") if l.startswith("##")]
    assert "##estimate=1" in head
    assert "##ci_window=509" in head            # the ceiling of the larger estimated upper cutoff, 508.87 (tests/test_estimate.py recomputes it)
    plain = str(tmp_path / "p.vcf")
    run_cli(["--vcf", plain, "--ci"])
    head = [l for l in open(plain).read().split("\n") if l.startswith("##")]
    assert "##estimate=1" not in head and "##ci_window=533" in head


def stripped_configuration(tmp_path):
    """the fixture's configuration with bare readgroup / map / readlen / lib fields: no mean, std or cutoff anywhere"""
    keep = ("readgroup:", "map:", "readlen:", "lib:")
    lines = [l for l in open(os.path.join(CHR21, "inv_del_bam_config")).read().split("\n")]
    path = str(tmp_path / "bare.cfg")
    open(path, "w").write("\n".join("\t".join(f for f in l.split("\t") if f.startswith(keep)) for l in lines))
    assert "mean" not in open(path).read() and "upper" not in open(path).read()
    return path


def test_cli_a_bare_configuration_is_enough(estimated, tmp_path):
    out, _, _ = estimated
    bare, _ = run_cli(["--estimate"], cfg=stripped_configuration(tmp_path))
    assert filter_cmd_lines(bare) == filter_cmd_lines(out)


def test_cli_library_without_a_valid_estimate(tmp_path):
    """-q 255 leaves no observation (no quality byte is greater): with the fixture's configuration both libraries keep its values, with a
    warning each, and the run prints what a plain -q 255 run prints; with the bare configuration the run ends with status 1"""
    out, err = run_cli(["-q", "255", "--estimate"])
    plain, _ = run_cli(["-q", "255"])
    assert filter_cmd_lines(out) == filter_cmd_lines(plain)
    for name in ("H_IJ-NA19238-NA19238-extlibs", "H_IJ-NA19240-NA19240-extlibs"):
        assert "WARNING: --estimate: library %s has no valid estimate (n_kept=0): it keeps the configuration's values" % name in err
    p = subprocess.run([EXE, "-q", "255", "--estimate", stripped_configuration(tmp_path)], cwd=CHR21, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 1 and not p.stdout.decode().strip()
    assert "ERROR: --estimate: library H_IJ-NA19238-NA19238-extlibs has no valid estimate (n_kept=0) and its configuration line gives neither mean nor std" in p.stderr.decode()
