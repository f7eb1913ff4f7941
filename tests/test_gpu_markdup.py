"""GPU tests of --mark-dup: the kernel-level entry point (bdx_mark_duplicates) against the numpy restatement of the rule, a context with
bdx_set_mark_duplicates against the same context without it on columns that carry the marks already, and bin/breakdancer-max --mark-dup on
every route against the run without the option on BAMs rewritten with 0x400 set, and against the oracle's rendering of the marked streams.
Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from exclude_cases import mask_from_table, mask_streams, rewrite_bam_without, table_rows, write_bed, write_case
from fuzzgen import make_case
from helpers import ROOT, OracleRun, filter_cmd_lines, make_opts
from markdup_cases import (cli_name_keys, marked_count, plant_duplicates, rewrite_bam_marked, rule_group_count, rule_marks, stream_marks,
                           with_marks)
from runner import compare, oracle_case, product_options

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
BDX_EINVAL, BDX_ESTATE = 1, 4
PAIRED, REV, MREV, FIRST, SECOND = 0x1, 0x10, 0x20, 0x40, 0x80


# ---- 1. kernel level ----
def fill_records(run_lengths, rng, start_pos=100):
    """columns whose runs have the given lengths (consecutive positions on two sequences): within a run few distinct K -- three mate
    positions, two strands, both mates, two libraries interleaved, one K dominant -- so that groups of every size up to the run's form; name keys from a
    small range, so that equal keys meet and the index decides; and among them records that are no candidates"""
    lens = np.asarray(run_lengths, np.int64)
    n = int(lens.sum())
    run_of = np.repeat(np.arange(len(lens)), lens)
    tid = (run_of >= len(lens) // 2).astype(np.int32) if len(lens) > 1 else np.zeros(n, np.int32)
    pos = (start_pos + 3 * run_of).astype(np.int32)
    # six in ten records take their run's dominant K, so that runs of two already hold duplicates; the others are drawn one by one
    dom = rng.random(n) < 0.6
    per_run = lambda draw: np.where(dom, draw(len(lens))[run_of], draw(n))
    mtid = np.where(rng.random(n) < 0.03, -1, per_run(lambda k: rng.integers(0, 2, k))).astype(np.int32)
    mpos = (pos + per_run(lambda k: rng.choice([200, 201, 350], k))).astype(np.int32)
    flag = (PAIRED | per_run(lambda k: np.where(rng.random(k) < 0.5, REV, 0)) | per_run(lambda k: np.where(rng.random(k) < 0.3, MREV, 0)) |
            per_run(lambda k: np.where(rng.random(k) < 0.5, FIRST, SECOND))).astype(np.uint16)
    u = rng.random(n)
    for bit, lo, hi in ((0x400, 0.0, 0.05), (0x4, 0.05, 0.07), (0x8, 0.07, 0.09), (0x100, 0.09, 0.10), (0x800, 0.10, 0.11)):
        flag[(u >= lo) & (u < hi)] |= bit
    flag[(u >= 0.11) & (u < 0.13)] &= ~np.uint16(PAIRED)
    lib = per_run(lambda k: rng.integers(0, 2, k)).astype(np.uint8)
    key = np.where(rng.random(n) < 0.5, rng.integers(0, 6, n).astype(np.uint64), rng.integers(0, 1 << 62, n).astype(np.uint64) * np.uint64(3))
    return tid, pos, mtid, mpos, flag, lib, key.astype(np.uint64)


def check_kernel(cols, label, want_marks=True):
    from breakdancer_amd.api import mark_duplicates
    want = rule_marks(*cols)
    got, groups = mark_duplicates(*cols)
    assert got.shape == want.shape
    if want_marks:
        assert want.any() and not want.all(), label   # (the reference alone cannot pass an empty comparison)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (label, bad[:10], len(bad))
    assert groups == rule_group_count(*cols), label
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 5000])
def test_kernel_equals_numpy_on_sorted_random_columns(n):
    rng = np.random.default_rng(4000 + n)
    # runs of 1-6 dominate; the lengths are cut to n records
    lens = []
    while sum(lens) < n:
        lens.append(min(int(rng.choice([1, 1, 2, 2, 3, 4, 5, 6, 9])), n - sum(lens)))
    cols = fill_records(lens, rng)
    assert len(cols[0]) == n
    # (no record can be a duplicate among fewer than two)
    check_kernel(cols, "n=%d" % n, want_marks=n >= 63)


def test_kernel_runs_around_the_direct_comparison_limit():
    """runs of exactly T-1, T, T+1, 2T and 2T+1 records for the kernel's T: at index 0, across a wave boundary (64), across a tile
    boundary (256), and ending at n-1"""
    from breakdancer_amd import _lib
    T = _lib.DUP_T
    rng = np.random.default_rng(4100)
    small = lambda k: [int(x) for x in rng.integers(1, 4, k)]
    for L in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
        for lead in (0, 40, 250):
            head = []
            while sum(head) < lead:
                head.append(min(int(rng.integers(1, 4)), lead - sum(head)))
            for tail in (small(30), []):
                lens = head + [L] + tail
                cols = fill_records(lens, rng)
                at = sum(head)
                assert (at < 64 < at + L or lead != 40) and (at < 256 < at + L or lead != 250)
                want = check_kernel(cols, "L=%d lead=%d tail=%d" % (L, lead, len(tail)))
                assert want[at:at + L].any()   # marks inside the run under test
    # all five next to each other, and two long runs back to back
    check_kernel(fill_records([T - 1, T, T + 1, 2 * T, 2 * T + 1, 1, T + 1, T + 1], rng), "side by side")


def test_kernel_one_run_of_twenty_thousand():
    """one position with 20,000 records: 100 groups of 2-500 and the rest singletons, between ordinary runs"""
    rng = np.random.default_rng(4200)
    sizes = np.concatenate([[2, 500], rng.integers(2, 300, 98)])
    n_run = 20000
    assert sizes.sum() < n_run - 1000
    group_of = np.concatenate([np.repeat(np.arange(100), sizes), 100 + np.arange(n_run - sizes.sum())])
    group_of = group_of[rng.permutation(n_run)]
    head = fill_records([1, 2, 3, 1, 2], rng, start_pos=10)
    tail = fill_records([2, 1, 3], rng, start_pos=90000)
    # K of group g: mate position 1000 + g (every group its own), everything else equal; two libraries would split groups, so one
    tid = np.zeros(n_run, np.int32)
    pos = np.full(n_run, 5000, np.int32)
    mid = (tid, pos, np.zeros(n_run, np.int32), (1000 + group_of).astype(np.int32), np.full(n_run, PAIRED | MREV | FIRST, np.uint16),
           np.zeros(n_run, np.uint8), rng.integers(0, 1 << 40, n_run).astype(np.uint64))
    head = (np.zeros_like(head[0]),) + head[1:]   # (one sequence: the store stays sorted)
    tail = (np.zeros_like(tail[0]),) + tail[1:]
    cols = tuple(np.concatenate([h, m, t]) for h, m, t in zip(head, mid, tail))
    want = check_kernel(cols, "20k run")
    o = len(head[0])
    assert int(want[o:o + n_run].sum()) == int(sizes.sum()) - 100


def test_kernel_unsorted_input_forms_separate_runs():
    f = PAIRED | MREV | FIRST
    rows = np.array([(0, 100, 0, 400, f, 0, 5), (0, 200, 0, 500, f, 0, 9), (0, 100, 0, 400, f, 0, 1), (0, 100, 0, 400, f, 0, 3)], np.int64)
    cols = [rows[:, i] for i in range(6)] + [rows[:, 6].astype(np.uint64)]
    want = check_kernel(cols, "unsorted")
    assert want.tolist() == [False, False, False, True]


def test_kernel_long_stretches_at_one_position_that_are_not_adjacent_are_separate_runs():
    """unsorted input: one (tid, pos) in several stretches, each longer than the direct comparison takes, with other records between them --
    every stretch is a run of its own, on the table's path as on the direct one"""
    from breakdancer_amd import _lib
    T = _lib.DUP_T
    f = PAIRED | MREV | FIRST
    rng = np.random.default_rng(4300)

    def stretch(k, pos=100, mpos=400, flag=f):
        return [(0, pos, 0, mpos, flag, 0, int(x)) for x in rng.integers(1, 1 << 40, k)]
    # 65 records of one K, one record elsewhere, 65 more of the same K: 64 + 64 marks in 2 groups
    rows = stretch(T + 1) + [(0, 200, 0, 500, f, 0, 9)] + stretch(T + 1)
    a = np.array(rows, np.int64)
    cols = [a[:, i] for i in range(6)] + [a[:, 6].astype(np.uint64)]
    want = check_kernel(cols, "two stretches")
    assert int(want.sum()) == 2 * T and rule_group_count(*cols) == 2
    assert not want[:T + 1].all() and not want[T + 2:].all()   # a survivor in each
    # three stretches of different lengths (one of them short: the direct path beside the table's), two K in each, a short run between
    rows = (stretch(T + 1) + stretch(T + 5, mpos=401) + [(0, 200, 0, 500, f, 0, 9), (0, 200, 0, 500, f, 0, 3)] + stretch(2 * T + 1) + stretch(3, mpos=401) +
            [(1, 100, 0, 400, f, 0, 5)] + stretch(T - 1) + [(0, 300, 0, 1, f, 0, 1)] + stretch(T + 2, mpos=401))
    a = np.array(rows, np.int64)
    cols = [a[:, i] for i in range(6)] + [a[:, 6].astype(np.uint64)]
    check_kernel(cols, "several stretches")
    # the same with the stretches' records shuffled inside each stretch
    a2 = a.copy()
    lo = 0
    for hi in list(np.nonzero(np.diff(a[:, 1]) | np.diff(a[:, 0]))[0] + 1) + [len(a)]:
        a2[lo:hi] = a[lo:hi][rng.permutation(hi - lo)]
        lo = hi
    cols = [a2[:, i] for i in range(6)] + [a2[:, 6].astype(np.uint64)]
    check_kernel(cols, "several stretches, shuffled")


def test_kernel_one_key_shared_by_thirty_thousand_records():
    """a collapsed repeat: one position, one K, 30,000 candidates -- every one of them meets in one slot of the table; beside it a second
    K with 2,000 and equal name keys among them (the index decides)"""
    rng = np.random.default_rng(4400)
    n1, n2 = 30000, 2000
    n = n1 + n2
    which = rng.permutation(n) < n1
    key = rng.integers(1, 1 << 62, n).astype(np.uint64)
    key[~which] = rng.integers(0, 50, n2).astype(np.uint64)
    cols = (np.zeros(n, np.int32), np.full(n, 777, np.int32), np.zeros(n, np.int32), np.where(which, 1000, 1001).astype(np.int32),
            np.full(n, PAIRED | MREV | FIRST, np.uint16), np.zeros(n, np.uint8), key)
    want = check_kernel(cols, "one K")
    assert int(want.sum()) == n - 2 and rule_group_count(*cols) == 2


def test_kernel_argument_errors():
    from breakdancer_amd import _lib
    lib = _lib.load()
    n = 4
    a32, a16, a8, a64, mask = np.zeros(n, np.int32), np.zeros(n, np.uint16), np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    ptrs = [a32.ctypes.data, a32.ctypes.data, a32.ctypes.data, a32.ctypes.data, a16.ctypes.data, a8.ctypes.data, a64.ctypes.data]
    g = C.c_uint64(7)
    assert lib.bdx_mark_duplicates(0, *ptrs, n, mask.ctypes.data, C.byref(g)) == 0 and g.value == 0
    assert lib.bdx_mark_duplicates(0, *ptrs, n, mask.ctypes.data, None) == 0
    assert lib.bdx_mark_duplicates(0, *([None] * 7), 0, None, None) == 0          # n == 0
    for k in range(7):
        p = list(ptrs)
        p[k] = None
        assert lib.bdx_mark_duplicates(0, *p, n, mask.ctypes.data, None) == BDX_EINVAL, k
    assert lib.bdx_mark_duplicates(0, *ptrs, n, None, None) == BDX_EINVAL


# ---- 2. context level ----
def libs_of(run):
    from breakdancer_amd.api import LibraryConfig
    return [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]),
                          name=run.lib_names[i]) for i in range(run.nlibs)]


@pytest.fixture(scope="module", params=["three-libraries", "one-library"])
def ctx_case(request):
    """a fuzz case with planted duplicates: the oracle on the streams as they are (the merged order), the marks of the merged store, and
    the oracle on the streams with the marks applied in numpy"""
    cfg, streams, targets = make_case(1410)
    streams = plant_duplicates(streams, 1410)
    if request.param == "one-library":   # (a context with one library never copies the library column)
        cfg = "".join(l + "\n" for l in cfg.splitlines() if "map:b.bam" in l)
        streams = streams[1:]
    opts = make_opts(score_threshold=-1)
    plain = oracle_case(cfg, streams, targets, opts)
    soa = plain.merged_soa()
    cols = (soa["tid"], soa["pos"], soa["mtid"], soa["mpos"], soa["flag"], soa["lib"], soa["name_id"])
    marks = rule_marks(*cols)
    groups = rule_group_count(*cols)
    assert marks.sum() > 50 and groups > 30
    per = []
    for b, st in enumerate(streams):
        m = np.zeros(len(st["tid"]), bool)
        sel = plain.m_bam == b
        m[plain.m_src[sel]] = marks[sel]
        per.append(with_marks(st, m))
    marked = oracle_case(cfg, per, targets, opts)
    np.testing.assert_array_equal(marked.m_bam, plain.m_bam)   # (the merged order does not look at 0x400)
    np.testing.assert_array_equal(marked.m_src, plain.m_src)
    assert table_rows(marked.text) and table_rows(marked.text) != table_rows(plain.text)   # the duplicates matter
    return plain, marked, soa, marks, groups


def new_ctx(run, mark):
    import breakdancer_amd as bda
    bd = bda.BreakDancer(product_options(run.opts), libs_of(run), run.nbams, ntids=0, max_read_window_size=run.w0)
    if mark:
        bd.mark_duplicates()
    return bd


def columns(soa):
    from breakdancer_amd.api import BATCH_FIELDS
    out = {}
    for k, dt in BATCH_FIELDS:
        src = soa.get(k)
        if src is None:
            src = soa["bdqual"] if k == "mapq" else soa["name_id"]
        out[k] = np.ascontiguousarray(src, dtype=dt)
    return out


def check_ctx(bd, marked, marks, groups, ref_cls):
    for _ in range(2):   # a second bdx_run gives the same
        bd.run()
        compare(marked, bd)
        np.testing.assert_array_equal(bd.read_class(), ref_cls)
        assert bd.duplicates() == (int(marks.sum()), groups)
    assert bd.lib.bdx_set_mark_duplicates(bd.h, 0) == BDX_ESTATE   # a setter call while reads are held
    assert bd.lib.bdx_set_mark_duplicates(bd.h, 1) == 0            # (no change: nothing to refuse)


def test_context_marks_before_pass_one(ctx_case):
    plain, marked, soa, marks, groups = ctx_case
    cols = columns(soa)
    n = len(marks)
    # the reference: the same context without the option, on columns whose flags carry the marks
    ref = new_ctx(marked, False)
    ref.push_reads(dict(cols, flag=np.where(marks, cols["flag"] | 0x400, cols["flag"]).astype(np.uint16)))
    ref.run()
    compare(marked, ref)
    ref_cls = ref.read_class()
    assert ref.duplicates() == (0, 0)
    # without the option the unmarked columns give the unmarked result
    off = new_ctx(plain, False)
    off.push_reads(cols)
    compare(plain, off.run())
    assert (off.read_class() != ref_cls).any()
    off.close()
    # (a) bdx_push, pageable memory, two batches
    bd = new_ctx(marked, True)
    m, g = C.c_uint64(0), C.c_uint64(0)
    assert bd.lib.bdx_get_duplicates(bd.h, C.byref(m), C.byref(g)) == BDX_ESTATE   # before a run
    cut = n // 3
    bd.push_reads({k: v[:cut] for k, v in cols.items()})
    bd.push_reads({k: v[cut:] for k, v in cols.items()})
    check_ctx(bd, marked, marks, groups, ref_cls)
    bd.close()
    # (b) bdx_acquire_batch / bdx_submit_batch across several batches
    bd = new_ctx(marked, True)
    bd.stream_reads(cols, batch=777)
    check_ctx(bd, marked, marks, groups, ref_cls)
    # the marks are defined per load: nothing is appended behind a run
    with pytest.raises(Exception, match="appended"):
        bd.stream_reads({k: v[:100] for k, v in cols.items()}, batch=100)
    # ... and the next load on the same context starts over
    bd.reset_reads()
    bd.stream_reads(cols, batch=5000)
    check_ctx(bd, marked, marks, groups, ref_cls)
    bd.close()
    ref.close()


def test_context_marks_pinned_batches_and_adopted_reads(ctx_case):
    plain, marked, soa, marks, groups = ctx_case
    cols = columns(soa)
    n = len(marks)
    ref = new_ctx(marked, False)
    ref.push_reads(dict(cols, flag=np.where(marks, cols["flag"] | 0x400, cols["flag"]).astype(np.uint16)))
    ref_cls = ref.run().read_class()
    ref.close()
    hip = C.CDLL("libamdhip64.so")
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipHostFree.argtypes = [C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    # (c) pinned host arrays in two batches and a pageable one between them: the name keys of the pinned ones stay on the host
    pinned, hp = {}, []
    for k, a in cols.items():
        p = C.c_void_p()
        assert hip.hipHostMalloc(C.byref(p), max(a.nbytes, 16), 0) == 0
        hp.append(p)
        v = np.ctypeslib.as_array((C.c_uint8 * a.nbytes).from_address(p.value)).view(a.dtype)
        v[:] = a
        pinned[k] = v
    bd = new_ctx(marked, True)
    c1, c2 = n // 4, n // 2
    bd.push_reads({k: v[:c1] for k, v in pinned.items()})
    bd.push_reads({k: np.array(v[c1:c2]) for k, v in pinned.items()})
    bd.push_reads({k: v[c2:] for k, v in pinned.items()})
    check_ctx(bd, marked, marks, groups, ref_cls)
    bd.close()
    for k, a in cols.items():
        np.testing.assert_array_equal(pinned[k], a)   # the caller's batches are unchanged
    for p in hp:
        hip.hipHostFree(p)
    # (d) bdx_set_device_reads: the caller's arrays in HBM stay as they are, the flag column included
    dev, ptrs = {}, {}
    for k, a in cols.items():
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        dev[k] = p
        ptrs[k] = p.value
    bd = new_ctx(marked, True)
    bd.set_device_reads(ptrs, n)
    check_ctx(bd, marked, marks, groups, ref_cls)
    bd.close()
    for k, a in cols.items():
        back = np.empty_like(a)
        assert hip.hipMemcpy(back.ctypes.data, dev[k], a.nbytes, 2) == 0
        np.testing.assert_array_equal(back, a, err_msg=k)
        hip.hipFree(dev[k])


# ---- 3. the CLI ----
def run_cli(args, cwd, env=None):
    p = subprocess.run([EXE] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, BDX_TIMING="1", **(env or {})))
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def lib_columns(cfg, streams):
    run = OracleRun(cfg, make_opts())
    return [np.array([run.lib_of_rg(g) for g in st["rg"]], dtype=np.int64) for st in streams]


def cli_marks(cfg, streams, only_tid=-1):
    """(marks per stream, D, G) of the store a CLI run holds: every record of the streams, or those of one sequence with -o"""
    libs = lib_columns(cfg, streams)
    keys = [cli_name_keys(st) for st in streams]
    per, groups = stream_marks(streams, libs, keys)
    if only_tid >= 0:
        sub = [{k: ([x for x, s in zip(v, np.asarray(st["tid"]) == only_tid) if s] if isinstance(v, list) else np.asarray(v)[np.asarray(st["tid"]) == only_tid])
                for k, v in st.items()} for st in streams]
        in_t = [np.asarray(st["tid"]) == only_tid for st in streams]
        sub_per, groups = stream_marks(sub, [l[m] for l, m in zip(libs, in_t)], [k[m] for k, m in zip(keys, in_t)])
        for p, sp, m in zip(per, sub_per, in_t):
            np.testing.assert_array_equal(p[m], sp)   # (runs never span sequences: the marks of a sequence are its own)
        return per, sum(int(sp.sum()) for sp in sub_per), groups
    return per, sum(int(p.sum()) for p in per), groups


CLI_ROUTES = [("device", [], dict(), dict()), ("host", [], dict(BDX_DECODE="host"), dict()), ("o-c2", ["-o", "c2"], dict(), dict(chr_tid=1)),
              ("two-ranks", [], dict(BDX_GPUS="0,0"), dict())]


@pytest.mark.parametrize("route", range(len(CLI_ROUTES)), ids=[r[0] for r in CLI_ROUTES])
@pytest.mark.parametrize("seed", [1400, 1401, 1403])
def test_cli_with_mark_dup_equals_the_run_on_marked_files(tmp_path, seed, route):
    label, args, env, kw = CLI_ROUTES[route]
    rng = np.random.default_rng(seed)
    cfg, streams, targets = make_case(seed)
    streams = plant_duplicates(streams, seed)
    indexed = seed != 1401   # (without .bai files -o reads the whole file, and a sharded run is fed by the host reader)
    write_case(str(tmp_path), streams, targets, rng, index=indexed)
    (tmp_path / "cfg").write_text(cfg)
    per, d_want, g_want = cli_marks(cfg, streams, kw.get("chr_tid", -1))
    assert 0 < g_want <= d_want < sum(len(st["tid"]) for st in streams)
    rew = tmp_path / "rewritten"
    rew.mkdir()
    for fn, m in zip(("a.bam", "b.bam"), per):
        assert rewrite_bam_marked(str(tmp_path / fn), str(rew / fn), m) == int(m.sum())
    (rew / "cfg").write_text(cfg)
    opts = make_opts(score_threshold=-1, **kw)
    want = oracle_case(cfg, [with_marks(st, m) for st, m in zip(streams, per)], targets, opts).text
    plain = oracle_case(cfg, streams, targets, opts).text
    # the fixture contains duplicates that matter: the table changes
    assert table_rows(want) and table_rows(want) != table_rows(plain)
    rc, out, err = run_cli(["-y", "-1"] + args + ["--mark-dup", "cfg"], str(tmp_path), env)
    assert rc == 0, (label, err)
    if label == "device":
        assert "on the GPU" in err, err   # (no silent hand-over to the host reader)
    assert filter_cmd_lines(out) == filter_cmd_lines(want), (label, err)
    assert marked_count(err) == (d_want, g_want), label
    rc, ref, err = run_cli(["-y", "-1"] + args + ["cfg"], str(rew), env)
    assert rc == 0 and "duplicate records" not in err, (label, err)
    assert filter_cmd_lines(out) == filter_cmd_lines(ref), label
    if label == "device":   # without the option nothing changes
        rc, out, err = run_cli(["-y", "-1"] + args + ["cfg"], str(tmp_path), env)
        assert rc == 0 and filter_cmd_lines(out) == filter_cmd_lines(plain) and "duplicate records" not in err
        assert table_rows(out) != table_rows(ref)


def test_cli_file_the_device_path_gives_up_is_marked_behind_the_host_reader(tmp_path):
    """one secondary record of 4.5 MB among ordinary ones: the device decode gives the file up and the host reader takes it from the
    start -- the store is marked all the same"""
    from breakdancer_amd.bamwrite import write_bam_records
    seed = 1405
    cfg, streams, targets = make_case(seed)
    streams = plant_duplicates(streams, seed)[:1]
    cfg1 = "".join(l + "\n" for l in cfg.splitlines() if "map:a.bam" in l)
    st = streams[0]
    recs = [dict(tid=st["tid"][i], pos=st["pos"][i], mtid=st["mtid"][i], mpos=st["mpos"][i], isize=st["isize"][i], flag=st["flag"][i], qlen=st["qlen"][i],
                 mapq=int(st["bdqual"][i]), am=None, rg=st["rg"][i], name="read%d" % int(st["name_id"][i])) for i in range(len(st["tid"]))]
    big = dict(recs[2 * len(recs) // 3])
    big["qlen"] = 3_000_000
    big["flag"] = int(big["flag"]) | 0x100   # (secondary: the reader filter drops it)
    recs.insert(2 * len(recs) // 3, big)
    write_bam_records(str(tmp_path / "a.bam"), recs, targets, rgs=("rg1", "rg2", "rg3"), seed=1)
    (tmp_path / "cfg").write_text(cfg1)
    per, d_want, g_want = cli_marks(cfg1, streams)
    want = oracle_case(cfg1, [with_marks(st, per[0])], targets, make_opts(score_threshold=-1)).text
    assert d_want > 0 and table_rows(want)
    rc, out, err = run_cli(["-y", "-1", "--mark-dup", "cfg"], str(tmp_path))
    assert rc == 0, err[-600:]
    assert "host decode threads" in err, err[-600:]
    assert filter_cmd_lines(out) == filter_cmd_lines(want)
    assert marked_count(err) == (d_want, g_want)


@pytest.fixture()
def one_bam_case(tmp_path):
    """one BAM of a fuzz case with planted duplicates, its marks, and the same BAM written again with 0x400 on the marked records"""
    seed = 1404
    rng = np.random.default_rng(seed)
    cfg, streams, targets = make_case(seed)
    streams = plant_duplicates(streams, seed)[:1]
    cfg1 = "".join(l + "\n" for l in cfg.splitlines() if "map:a.bam" in l)
    write_case(str(tmp_path), streams, targets, rng)
    (tmp_path / "cfg").write_text(cfg1)
    per, d_want, g_want = cli_marks(cfg1, streams)
    rew = tmp_path / "rewritten"
    rew.mkdir()
    assert rewrite_bam_marked(str(tmp_path / "a.bam"), str(rew / "a.bam"), per[0]) == d_want > 0
    (rew / "cfg").write_text(cfg1)
    opts = make_opts(score_threshold=-1)
    want = oracle_case(cfg1, [with_marks(streams[0], per[0])], targets, opts).text
    plain = oracle_case(cfg1, streams, targets, opts).text
    assert table_rows(want) and table_rows(want) != table_rows(plain)
    return tmp_path, rew, want, plain, (cfg1, streams, targets, rng), (d_want, g_want)


def test_mark_dup_with_exclude(one_bam_case):
    """excluded records do not exist: they do not compete, and the count is of the records that are left"""
    tmp, rew, _, plain, (cfg1, streams, targets, rng), _ = one_bam_case
    iv = mask_from_table(plain, targets, rng)
    write_bed(str(tmp / "m.bed"), iv, targets, rng)
    masked, removed = mask_streams(streams, iv)
    assert removed[0] > 0
    per, d_want, g_want = cli_marks(cfg1, masked)
    want = oracle_case(cfg1, [with_marks(masked[0], per[0])], targets, make_opts(score_threshold=-1)).text
    assert d_want > 0 and table_rows(want)
    for env in (dict(), dict(BDX_DECODE="host")):
        rc, out, err = run_cli(["-y", "-1", "--exclude", "m.bed", "--mark-dup", "cfg"], str(tmp), env)
        assert rc == 0, err
        assert filter_cmd_lines(out) == filter_cmd_lines(want), env
        assert marked_count(err) == (d_want, g_want), env
    # the file without the excluded records, then with the marks: neither option
    both = tmp / "both"
    both.mkdir()
    rewrite_bam_without(str(tmp / "a.bam"), str(both / "tmp.bam"), iv)
    assert rewrite_bam_marked(str(both / "tmp.bam"), str(both / "a.bam"), per[0]) == d_want
    os.remove(str(both / "tmp.bam"))
    (both / "cfg").write_text(cfg1)
    rc, ref, err = run_cli(["-y", "-1", "cfg"], str(both))
    assert rc == 0 and filter_cmd_lines(ref) == filter_cmd_lines(want), err


def test_mark_dup_with_vcf(one_bam_case):
    tmp, rew, want, plain, _, _ = one_bam_case
    rc, out, err = run_cli(["-y", "-1", "--vcf", "out.vcf", "--mark-dup", "cfg"], str(tmp))
    assert rc == 0 and filter_cmd_lines(out) == filter_cmd_lines(want), err
    rc, out, err = run_cli(["-y", "-1", "--vcf", "out.vcf", "cfg"], str(rew))
    assert rc == 0 and filter_cmd_lines(out) == filter_cmd_lines(want), err
    rc, out, err = run_cli(["-y", "-1", "--vcf", "off.vcf", "cfg"], str(tmp))
    assert rc == 0 and filter_cmd_lines(out) == filter_cmd_lines(plain), err
    got = (tmp / "out.vcf").read_text().splitlines()
    ref = (rew / "out.vcf").read_text().splitlines()
    off = (tmp / "off.vcf").read_text().splitlines()
    assert "##mark_dup=1" in got and not [l for l in ref + off if l.startswith("##mark_dup")]
    body = lambda ls: [l for l in ls if not l.startswith("##")]
    assert body(got) == body(ref) and len(body(got)) > 1   # every record, DR and DV of every sample included
    meta = lambda ls: [l for l in ls if l.startswith("##") and not l.startswith(("##command=", "##mark_dup="))]
    assert meta(got) == meta(ref)
    # DV drops: a call that both runs make (same ends and type) has no more supporting pairs with the option, and some have fewer
    def dv_by_site(ls):
        out = {}
        for l in body(ls)[1:]:
            f = l.split("\t")
            info = dict(x.split("=", 1) for x in f[7].split(";") if "=" in x)
            out[(f[0], f[1], info.get("CHR2"), info.get("POS2"), info.get("SVTYPE"))] = sum(int(s.split(":")[4]) for s in f[9:] if s.split(":")[4] != ".")
        return out
    on, no = dv_by_site(got), dv_by_site(off)
    common = set(on) & set(no)
    assert common and all(on[k] <= no[k] for k in common) and any(on[k] < no[k] for k in common)


def test_mark_dup_with_sites(one_bam_case):
    """--sites counts over the marked store: the run's own calls fed back as sites give, with the option on the planted file, the VCF the
    run without it writes on the file that carries the marks"""
    tmp, rew, want, plain, _, _ = one_bam_case
    rows = [l for l in table_rows(plain) if (l.split("\t")[6] == "CTX") == (l.split("\t")[0] != l.split("\t")[3])]
    assert len(rows) > 5
    for d in (tmp, rew):
        (d / "sites.txt").write_text("".join(l + "\n" for l in rows))
    rc, out, err = run_cli(["-y", "-1", "--sites", "sites.txt", "--sites-vcf", "s.vcf", "--mark-dup", "cfg"], str(tmp))
    assert rc == 0 and filter_cmd_lines(out) == filter_cmd_lines(want), err
    rc, out, err = run_cli(["-y", "-1", "--sites", "sites.txt", "--sites-vcf", "s.vcf", "cfg"], str(rew))
    assert rc == 0 and filter_cmd_lines(out) == filter_cmd_lines(want), err
    rc, out, err = run_cli(["-y", "-1", "--sites", "sites.txt", "--sites-vcf", "off.vcf", "cfg"], str(tmp))
    assert rc == 0, err
    got, ref, off = ((d / f).read_text().splitlines() for d, f in ((tmp, "s.vcf"), (rew, "s.vcf"), (tmp, "off.vcf")))
    assert "##mark_dup=1" in got and not [l for l in ref + off if l.startswith("##mark_dup")]
    body = lambda ls: [l for l in ls if not l.startswith("##")]
    assert body(got) == body(ref) and len(body(got)) == len(rows) + 1
    # the duplicates counted without the option: DV of every site at least as large, of some larger
    dv = lambda ls: [sum(int(s.split(":")[4]) for s in l.split("\t")[9:] if s.split(":")[4] != ".") for l in body(ls)[1:]]
    assert all(a <= b for a, b in zip(dv(got), dv(off))) and sum(dv(got)) < sum(dv(off))


def dump_files(args, cwd, out_dir, env):
    out_dir.mkdir()
    rc, out, err = run_cli(["-y", "-1", "-g", str(out_dir / "out.bed"), "-d", str(out_dir / "fq")] + args + ["cfg"], str(cwd), env)
    assert rc == 0, err
    return filter_cmd_lines(out), {f: open(os.path.join(str(out_dir), f), "rb").read() for f in sorted(os.listdir(str(out_dir)))}


def test_dumps_and_cache_with_mark_dup(one_bam_case):
    tmp, rew, want, _, _, counts = one_bam_case
    dev = dump_files(["--mark-dup"], tmp, tmp / "dev", dict())
    host = dump_files(["--mark-dup"], tmp, tmp / "host", dict(BDX_DECODE="host"))
    ref = dump_files([], rew, tmp / "ref", dict())   # no option, the file with the marks
    assert dev[0] == host[0] == ref[0] == filter_cmd_lines(want)
    assert dev[1] == host[1] == ref[1] and dev[1] and any(len(v) for v in dev[1].values())
    # -C writes the command line into the cache; -R parses --mark-dup from it
    rc, out_c, err = run_cli(["-y", "-1", "-C", "c", "--mark-dup", "cfg"], str(tmp))
    assert rc == 0, err
    rc, out_r, err = run_cli(["-R", "c"], str(tmp))
    assert rc == 0, err
    assert filter_cmd_lines(out_c) == filter_cmd_lines(out_r) == filter_cmd_lines(want)
    assert marked_count(err) == counts
