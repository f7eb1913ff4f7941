"""GPU tests of --depth: the passing read starts inside given intervals (bdx_count_interval_reads, KR) against a numpy restatement of the
rule in include/bdx.h, on both of the kernel's routes, the argument errors, and the CLI's RCI / RCF / RDR on the chr21 golden fixture and
on a sharded run.

The rule pinned here: record i counts for interval (t, [beg, end)) -- 0-based, half-open -- when tid[i] == t, beg <= pos[i] < end and
cls[i] & 0x10 (K1 let it pass); counts are per key, the BAM file or the library.

The restatement is brute force: one mask over all records per interval, no search and no chunks.  Every comparison is exact.  The
intervals are placed by record index around the multiples of the kernel's chunk (_lib.DEPTH_CHUNK), and the tests assert -- with
np.searchsorted, on the store as it came out -- that every class of interval they mean to submit is there."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_sites as T
from helpers import GOLDEN, ROOT, filter_cmd_lines, load_chr21, make_opts
from runner import oracle_case, product_from_oracle, product_options

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CWD = os.path.join(GOLDEN, "chr21")
IMAX = 2**31 - 1
RUN_AT = (2048, 6144, 10240)      # chunk boundaries a run of equal positions straddles; 4096 and 8192 are left clean


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy restatement (brute force)
# ---------------------------------------------------------------------------------------------------------------------------------
def expected_counts(soa, cls, keys, nkeys, intervals):
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    ok = (cls & 0x10) != 0
    k = np.where((keys >= 0) & (keys < nkeys), keys, 0).astype(np.int64) if nkeys > 1 else np.zeros(len(t), np.int64)
    out = np.zeros((len(intervals), nkeys), np.uint32)
    for i, (tid, beg, end) in enumerate(intervals):
        hit = ok & (t == tid) & (s >= beg) & (s < end)
        out[i] = np.bincount(k[hit], minlength=nkeys)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# stores: three of test_gpu_sites.py's, and one laid out by record index for the chunk logic
# ---------------------------------------------------------------------------------------------------------------------------------
def chunk_store(libs, seed):
    """5 C + 777 records on c0 [0, 3000), c1 [3000, 4 C) and c3 [4 C, n): mates are neighbours in the store (a gap of 10: small inserts,
    which pass), every seventh pair fails -q, the last record's mate is absent, and the records [b - 7, b + 9) around b in RUN_AT start at
    one position"""
    from breakdancer_amd import _lib
    C = _lib.DEPTH_CHUNK
    assert C == 2048
    n = 5 * C + 777
    rng = np.random.default_rng(seed)
    tid = np.where(np.arange(n) < 3000, 0, np.where(np.arange(n) < 4 * C, 1, 3))
    pos = 1000 + 10 * np.arange(n) + rng.integers(0, 3, n) * 2           # strictly increasing, gaps of 6 .. 14
    for b in RUN_AT:
        pos[b - 7:b + 9] = pos[b - 7]
    st = T.Store(libs)
    for i in range(0, n - 1, 2):
        assert tid[i] == tid[i + 1]
        st.pair(int(rng.integers(0, len(libs))), int(tid[i]), int(pos[i]), int(tid[i]), int(pos[i + 1]), False, True, mapq=0 if (i // 2) % 7 == 3 else 60)
    st.pair(0, 3, int(pos[n - 1]), 3, int(pos[n - 1]) + 300, False, True, both=False)
    assert st.n_records() == n
    return st


STORES = {}
LABELS = ["one/65", "three/65", "three/big", "one/chunk", "three/chunk"]


def case(label):
    """(oracle run, merged stream) of a labelled store: built and run through the oracle once, shared by the tests"""
    if label not in STORES:
        if label.endswith("/chunk"):
            libs = T.ONE_LIB if label.startswith("one") else T.THREE_LIBS
            run = oracle_case(T.config_text(libs), chunk_store(libs, 5 + len(label)).streams(), T.TARGETS, make_opts())
            STORES[label] = (run, run.merged_soa())
        else:
            run, st, soa = T.store_case(label)
            STORES[label] = (run, soa)
    return STORES[label]


# ---------------------------------------------------------------------------------------------------------------------------------
# intervals, and what they are
# ---------------------------------------------------------------------------------------------------------------------------------
def index_range(soa, intervals):
    """[L, R) of every interval: where its records lie in the (tid, pos)-sorted store"""
    key = (soa["tid"].astype(np.int64) << 32) | soa["pos"].astype(np.int64)
    assert (np.diff(key) >= 0).all()
    iv = np.array(intervals, np.int64).reshape(-1, 3)
    return np.searchsorted(key, (iv[:, 0] << 32) | iv[:, 1], "left"), np.searchsorted(key, (iv[:, 0] << 32) | iv[:, 2], "left")


def make_intervals(soa, rng, C):
    """intervals for a store: around every multiple of C by record index, whole sequences, sequences without reads, empty ones, ones that
    begin or end at a position several records share, random ones; and triples (a, b), (b, c), (a, c) for the additivity test"""
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    n = len(t)
    iv = [(0, 0, 0), (0, 5000, 5000), (2, 0, IMAX), (2, 100, 5000), (4, 0, IMAX), (1000, 0, IMAX), (IMAX, 0, IMAX), (0, IMAX, IMAX),
          (0, 0, 1), (3, int(s[-1]) + 1, IMAX), (int(t[-1]), int(s[-1]), IMAX)]
    iv += [(int(x), 0, IMAX) for x in np.unique(t)]                                     # whole sequences: [0, 2^31 - 1)
    by_index = lambda i, j, end_off=0: (int(t[i]), int(s[i]), int(s[j]) + end_off)        # (records i .. j of one sequence)

    def add(i, j, end_off=0):
        if 0 <= i <= j < n and t[i] == t[j]:
            iv.append(by_index(i, j, end_off))

    for b in range(C, n, C):
        for i, j in ((b - 300, b - 100), (b - 50, b + 50), (b - 1, b), (b, b + 1), (b, b + 40), (b - 40, b), (b - 900, b + C + 700),
                     (b - C - 3, b + C + 3), (b, b + C), (b - C, b), (b + 1, b + C - 1), (b - 7, b + 9), (b - 8, b - 7), (b + 8, b + 9)):
            add(i, j)
            add(i, j, 1)
    for tid in np.unique(t):
        idx = np.nonzero(t == tid)[0]
        add(int(idx[0]), int(idx[-1]))
        add(int(idx[0]), int(idx[-1]), 1)
        for _ in range(12):
            i, j = sorted(int(x) for x in rng.choice(idx, 2))
            add(i, j, int(rng.integers(0, 2)))
        gaps = idx[:-1][np.diff(s[idx]) >= 2]
        for i in gaps[:3]:
            iv.append((int(tid), int(s[i]) + 1, int(s[i + 1])))                          # between two records: not empty, no record
    # runs of equal positions: an interval that begins at the run's position takes all of it, one that ends there none of it
    same = np.nonzero((t[1:] == t[:-1]) & (s[1:] == s[:-1]))[0]
    for i in same[:: max(len(same) // 8, 1)]:
        iv.append((int(t[i]), int(s[i]), int(s[i]) + 1))
        iv.append((int(t[i]), int(s[i]), IMAX))
        iv.append((int(t[i]), max(int(s[i]) - 500, 0), int(s[i])))
    triples = []
    for _ in range(10):
        tid = int(rng.choice(np.unique(t)))
        idx = np.nonzero(t == tid)[0]
        a, b, c = sorted(int(s[x]) for x in rng.choice(idx, 3))
        triples.append((len(iv), len(iv) + 1, len(iv) + 2))
        iv += [(tid, a, b), (tid, b, c), (tid, a, c)]
    return iv, triples


def classes(soa, intervals, C):
    """which of the classes the tests want are among the intervals"""
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    n = len(t)
    iv = np.array(intervals, np.int64).reshape(-1, 3)
    L, R = index_range(soa, intervals)
    c0, c1 = (L + C - 1) // C, R // C
    has = set(np.unique(t).tolist())
    in_run = np.zeros(len(iv), bool)                        # beg is a position that several records of the sequence share
    for k in range(len(iv)):
        in_run[k] = L[k] + 1 < n and R[k] > L[k] + 1 and t[L[k]] == iv[k, 0] and s[L[k]] == iv[k, 1] and s[L[k] + 1] == iv[k, 1]
    return {
        "beg == end": bool((iv[:, 1] == iv[:, 2]).any()),
        "a range with no record": bool(((iv[:, 2] > iv[:, 1]) & (L == R) & np.isin(iv[:, 0], list(has))).any()),
        "inside one chunk": bool(((R > L) & (L // C == (R - 1) // C)).any()),
        "across one boundary, no whole chunk": bool(((R > L) & ((R - 1) // C == L // C + 1) & (c0 >= c1) & (L % C != 0) & (R % C != 0)).any()),
        "a whole chunk, both edges": bool(((c0 < c1) & (L % C != 0) & (R % C != 0)).any()),
        "L on a boundary": bool(((R > L) & (L % C == 0) & (L > 0)).any()),
        "R on a boundary": bool(((R > L) & (R % C == 0)).any()),
        "R == n, n % C != 0": bool(((R == n) & (R > L)).any()) and n % C != 0,
        "a whole sequence": bool(((iv[:, 1] == 0) & (iv[:, 2] == IMAX) & (R > L)).any()),
        "a sequence with no reads": bool(((iv[:, 0] == 2) & (iv[:, 2] > iv[:, 1])).any()) and 2 not in has,
        "a sequence beyond the header": bool((iv[:, 0] >= len(T.TARGETS)).any()),
        "[0, 2^31 - 1)": bool(((iv[:, 1] == 0) & (iv[:, 2] == IMAX)).any()),
        "begins at a run of equal positions": bool(in_run.any()),
        "a run of equal positions across a boundary": bool((in_run & (L % C != 0) & ((L // C) != ((L + 8) // C))).any()),
    }


SMALL_STORE_CLASSES = ("beg == end", "a range with no record", "inside one chunk", "R == n, n % C != 0", "a whole sequence", "a sequence with no reads",
                       "a sequence beyond the header", "[0, 2^31 - 1)")
INPUTS = {}


def inputs(label):
    """(intervals, additivity triples) of a store: made once, shared by the tests, with the classes they must hold asserted"""
    from breakdancer_amd import _lib
    if label not in INPUTS:
        run, soa = case(label)
        C = _lib.DEPTH_CHUNK
        iv, triples = make_intervals(soa, np.random.default_rng(len(label)), C)
        got = classes(soa, iv, C)
        n = len(soa["tid"])
        if label.endswith("/chunk"):
            assert n == 5 * C + 777 and sorted(set(soa["tid"].tolist())) == [0, 1, 3]
            assert all(got.values()), [k for k, v in got.items() if not v]
            assert 0 < int((run.cls & 0x10 == 0).sum()) < n // 4                 # some records do not pass
        else:
            assert all(got[k] for k in SMALL_STORE_CLASSES), (label, [k for k in SMALL_STORE_CLASSES if not got[k]])
        INPUTS[label] = (iv, triples)
    return INPUTS[label]


def key_settings(run, soa):
    return [(False, soa["bam"], run.nbams), (True, soa["lib"], run.nlibs)]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. both routes against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_interval_counts_equal_numpy_restatement_on_both_routes(label):
    from breakdancer_amd import _lib
    run, soa = case(label)
    iv, triples = inputs(label)                             # (the conditions on the inputs: before the GPU is used)
    assert (run.nbams, run.nlibs) == ((1, 1) if label.startswith("one") else (2, 3))
    bd = product_from_oracle(run)
    cls = bd.read_class()
    np.testing.assert_array_equal(cls & 0x3F, run.cls)      # (what K1 wrote is what the restatement reads)
    arr = np.array(iv, dtype=_lib.INTERVAL_DTYPE)
    rng = np.random.default_rng(3)
    total = 0
    for by_library, keys, nkeys in key_settings(run, soa):
        exp = expected_counts(soa, cls, keys, nkeys, iv)
        total += int(exp.sum())
        for plain in (0, 1):
            bd.set_debug("depth_plain", plain)
            got = bd.count_interval_reads(arr, by_library=by_library)
            assert got.shape == (len(iv), nkeys) and got.dtype == np.uint32
            np.testing.assert_array_equal(got, exp, err_msg="%s by_library=%d depth_plain=%d" % (label, by_library, plain))
            order = rng.permutation(len(iv))                # a permutation of the intervals gives the permuted result
            np.testing.assert_array_equal(bd.count_interval_reads(arr[order], by_library=by_library), exp[order])
            for nq in (1, 4, 5):                            # one block with idle waves, a full one, and one wave into the second
                np.testing.assert_array_equal(bd.count_interval_reads(arr[order[:nq]], by_library=by_library), exp[order[:nq]])
            for a, b, c in triples:                         # adjacent intervals add up to their union
                np.testing.assert_array_equal(got[a].astype(np.int64) + got[b], got[c])
        if nkeys > 1:
            assert (exp.sum(axis=0) > 0).all(), label       # (every key has passing reads somewhere)
    assert total > 0
    bd.set_debug("depth_plain", 0)
    first = bd.count_interval_reads(arr, by_library=True)
    bd.run()                                                # a second run, then a second call: the same answer
    np.testing.assert_array_equal(bd.count_interval_reads(arr, by_library=True), first)
    assert bd.count_interval_reads([]).shape == (0, run.nbams)
    one = bd.count_interval_reads([(0, 0, IMAX)])           # (a sequence of tuples is taken as well)
    assert one.shape == (1, run.nbams) and int(one.sum()) == int(((soa["tid"] == 0) & (cls & 0x10 != 0)).sum())
    bd.close()


def test_interval_counts_with_dash_t_and_on_an_empty_store():
    """-t: no same-chromosome read passes, and the call says so; a context that ran with no reads counts 0 everywhere"""
    import breakdancer_amd as bda
    from breakdancer_amd.api import LibraryConfig
    run0, st, _ = T.store_case("three/65")
    run = oracle_case(T.config_text(T.THREE_LIBS), st.streams(), T.TARGETS, make_opts(transchr_rearrange=1))
    soa = run.merged_soa()
    bd = product_from_oracle(run)
    cls = bd.read_class()
    iv = [(0, 0, IMAX), (1, 0, IMAX), (0, 900, 1100), (3, 0, IMAX)]
    for by_library, keys, nkeys in key_settings(run, soa):
        exp = expected_counts(soa, cls, keys, nkeys, iv)
        same = (soa["tid"] == soa["mtid"]) & (cls & 0x10 != 0)
        assert not same.any() and exp.sum() > 0             # (only the CTX pairs' reads pass)
        for plain in (0, 1):
            bd.set_debug("depth_plain", plain)
            np.testing.assert_array_equal(bd.count_interval_reads(iv, by_library=by_library), exp)
    bd.close()
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]))
            for i in range(run.nlibs)]
    empty = bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0)
    empty.run()
    for plain in (0, 1):
        empty.set_debug("depth_plain", plain)
        for by_library in (False, True):
            got = empty.count_interval_reads(iv + [(0, 5, 5), (4, 0, 10)], by_library=by_library)
            assert got.shape == (6, run.nlibs if by_library else run.nbams) and not got.any()
    empty.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. bad calls
# ---------------------------------------------------------------------------------------------------------------------------------
def test_interval_counts_refuse_bad_calls():
    import ctypes as C
    import breakdancer_amd as bda
    from breakdancer_amd import _lib
    from breakdancer_amd.api import LibraryConfig
    run, soa = case("one/65")
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = np.array([(0, 0, 5000)], dtype=_lib.INTERVAL_DTYPE)
    out = np.zeros(4, np.uint32)
    call = lib.bdx_count_interval_reads
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]))
            for i in range(run.nlibs)]
    fresh = bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0)
    assert call(fresh.h, p(good), 1, 0, p(out)) == 4             # BDX_ESTATE: no run yet ...
    assert call(fresh.h, None, 1, 0, None) == 4 and call(fresh.h, None, 0, 0, None) == 4    # ... ahead of every other check
    with pytest.raises(bda.api.BdxError):
        fresh.set_debug("depth_plane", 1)                        # (an unknown switch is still refused)
    fresh.close()
    assert call(None, p(good), 1, 0, p(out)) == 1                # no context
    bd = product_from_oracle(run)
    assert call(bd.h, p(good), 1, 0, p(out)) == 0 and out[0] > 0
    assert call(bd.h, None, 0, 0, None) == 0                     # n == 0, null pointers
    assert call(bd.h, None, 1, 0, p(out)) == 1                   # BDX_EINVAL from here on: a null array
    assert call(bd.h, p(good), 1, 0, None) == 1
    for bad in ((-1, 0, 10), (0, -1, 10), (0, 10, 9), (-2**31, 0, 0), (0, -2**31, -2**31), (0, IMAX, 0)):
        a = np.array([good[0].tolist(), bad], dtype=_lib.INTERVAL_DTYPE)
        assert call(bd.h, p(a), 2, 0, p(out)) == 1, bad
        assert call(bd.h, p(a), 2, 1, p(out)) == 1, bad
    for fine in ((0, 10, 10), (0, IMAX, IMAX), (IMAX, 0, IMAX)):
        assert call(bd.h, p(np.array([fine], dtype=_lib.INTERVAL_DTYPE)), 1, 0, p(out)) == 0, fine
    assert call(bd.h, p(good), 2**31 + 1, 0, p(out)) == 5        # BDX_ELIMIT (checked before any interval is read) ...
    assert call(bd.h, None, 2**31 + 1, 0, p(out)) == 1           # ... and behind the null check
    assert call(bd.h, p(good), 1, 0, p(out)) == 0                # (the context is as good as before)
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the CLI on the chr21 golden fixture
# ---------------------------------------------------------------------------------------------------------------------------------
DEPTH_KEYS = ("RCI", "RCF", "RDR")


def run_cli(args, cwd=CWD, cfg="inv_del_bam_config", env=None):
    p = subprocess.run([EXE] + args + [cfg], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **env) if env else None, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode(), p.stderr.decode()


def strip_depth(text):
    """a VCF minus what --depth adds: the ##depth_flank= line, the three ##FORMAT lines and the three fields of the FORMAT column and of
    every sample (and minus its ##command= line)"""
    out = []
    for l in text.split("\n"):
        if l.startswith(("##depth_flank=", "##command=")) or any(l.startswith("##FORMAT=<ID=%s," % k) for k in DEPTH_KEYS):
            continue
        if l and not l.startswith("#"):
            c = l.split("\t")
            assert c[8] == "GT:GQ:PL:DR:DV:RCI:RCF:RDR" and all(len(f.split(":")) == 8 for f in c[9:]), l
            c[8:] = [":".join(f.split(":")[:5]) for f in c[8:]]
            l = "\t".join(c)
        out.append(l)
    return "\n".join(out)


def check_depth_records(text, prefix, rows, run, by_lib, flank):
    """every record of a --depth VCF against the restatement over the oracle's records; rows: the table rows the records stand for, as
    given (record k is <prefix><k + 1>).  Returns the (RCI, RCF) of the records' samples in table order, None for '.'."""
    lines = text.rstrip("\n").split("\n")
    meta = [l for l in lines if l.startswith("##")]
    assert "##depth_flank=%d" % flank in meta
    assert all(sum(l.startswith("##FORMAT=<ID=%s," % k) for l in meta) == 1 for k in DEPTH_KEYS)
    contigs = [l[len("##contig=<ID="):-1].split(",length=") for l in meta if l.startswith("##contig=")]
    names, length = [c[0] for c in contigs], {c[0]: int(c[1]) for c in contigs}
    by_id = {l.split("\t")[2]: l.split("\t") for l in lines if not l.startswith("#")}
    assert len(by_id) == len(rows) > 0
    soa = run.merged_soa()
    keys, nkeys = (soa["lib"], run.nlibs) if by_lib else (soa["bam"], run.nbams)
    held = set(soa["tid"].tolist()) if run.opts["chr_tid"] >= 0 else None          # -o: the one sequence the run read
    seen = []
    for k, row in enumerate(rows):
        rec = by_id["%s%d" % (prefix, k + 1)]
        fields = [f.split(":")[5:] for f in rec[9:]]
        assert len(fields) == nkeys
        p1, p2 = int(row[1]), int(row[4])
        dotted = row[0] != row[3] or p1 == p2 or (held is not None and names.index(row[0]) not in held)
        if dotted:
            assert all(f == [".", ".", "."] for f in fields), (k, rec)
            seen.append(None)
            continue
        tid, lo, hi, n = names.index(row[0]), min(p1, p2), max(p1, p2), length[row[0]]
        clamp = lambda x: min(max(x, 1), n + 1)
        inside = (tid, clamp(lo) - 1, clamp(hi) - 1)
        left, right = (tid, clamp(lo - flank) - 1, clamp(lo) - 1), (tid, clamp(hi) - 1, clamp(hi + flank) - 1)
        exp = expected_counts(soa, run.cls, keys, nkeys, [inside, left, right]).astype(np.int64)
        len_in, len_flank = inside[2] - inside[1], (left[2] - left[1]) + (right[2] - right[1])
        for j, f in enumerate(fields):
            rci, rcf = int(exp[0, j]), int(exp[1, j] + exp[2, j])
            rdr = "." if rcf == 0 or len_in == 0 or len_flank == 0 else "%.3f" % (rci * len_flank / (len_in * rcf))
            assert f == [str(rci), str(rcf), rdr], (k, j, f, rci, rcf, rdr)
        seen.append([(int(exp[0, j]), int(exp[1, j] + exp[2, j])) for j in range(nkeys)])
    return seen


@pytest.mark.parametrize("args", [[], ["-a"]], ids=["per-bam", "per-library"])
def test_cli_vcf_depth_on_the_golden_fixture(args, tmp_path):
    by_lib = "-a" in args
    run = load_chr21(make_opts(cn_lib=int(by_lib))).run()
    golden, _ = run_cli(args)
    f0, f1, f2 = str(tmp_path / "plain.vcf"), str(tmp_path / "depth.vcf"), str(tmp_path / "depth50.vcf")
    out0, _ = run_cli(["--vcf", f0] + args)
    out1, err1 = run_cli(["--vcf", f1, "--depth"] + args, env=dict(BDX_TIMING="1"))
    assert filter_cmd_lines(out0) == filter_cmd_lines(golden) and filter_cmd_lines(out1) == filter_cmd_lines(golden)
    assert len([l for l in err1.split("\n") if l.startswith("[bdx timing] --depth:")]) == 1
    plain, with_depth = open(f0).read(), open(f1).read()
    assert not any(k in plain for k in DEPTH_KEYS) and "depth_flank" not in plain     # (without --depth nothing of it appears)
    assert strip_depth(with_depth) == T.without_command(plain)
    rows = T.table_rows(out0)
    assert T.vcf_parts(plain)[1] == (run.lib_names if by_lib else [os.path.basename(b) for b in run.bam_names])
    seen = check_depth_records(with_depth, "BDX", rows, run, by_lib, 1000)
    assert len(seen) == 4 and all(s is not None and sum(rcf for _, rcf in s) > 0 for s in seen)
    assert any(rci > 0 for s in seen for rci, _ in s)
    if by_lib:
        return
    # BDX_DECODE=host: the same records are held
    fh = str(tmp_path / "host.vcf")
    outh, _ = run_cli(["--vcf", fh, "--depth"], env=dict(BDX_DECODE="host"))
    assert filter_cmd_lines(outh) == filter_cmd_lines(golden) and T.without_command(open(fh).read()) == T.without_command(with_depth)
    # --depth-flank 50 beside --ci: other flank counts, again the restatement's, and --ci's keys as without --depth
    out2, _ = run_cli(["--vcf", f2, "--depth", "--depth-flank", "50", "--ci"])
    fc = str(tmp_path / "ci.vcf")
    run_cli(["--vcf", fc, "--ci"])
    narrow = open(f2).read()
    assert filter_cmd_lines(out2) == filter_cmd_lines(golden) and strip_depth(narrow) == T.without_command(open(fc).read())
    seen50 = check_depth_records(narrow, "BDX", rows, run, by_lib, 50)
    assert [[rci for rci, _ in s] for s in seen50] == [[rci for rci, _ in s] for s in seen] and seen50 != seen


def test_cli_sites_vcf_depth_dots_and_dash_o(tmp_path):
    """--sites-vcf with -o: a site on a sequence the run did not read, a CTX site and a site with pos1 == pos2 print '.'; the others the
    restatement's counts, an end given in reverse order included"""
    run = load_chr21(make_opts(chr_tid=22)).run()
    from helpers import read_bam
    targets = read_bam(os.path.join(CWD, "NA19238_chr21_del_inv.bam"))[0]
    other = [t for t in targets if t != "21"][0]
    assert targets.index("21") == 22
    sites_file = str(tmp_path / "s.txt")
    lines = ["%s\t100\t1+1-\t%s\t900\t1+1-\tDEL\t800" % (other, other), "21\t29185462\t1+1-\t21\t29186122\t1+1-\tDEL",
             "21\t500\t1+0-\t%s\t700\t0+1-\tCTX\t-1" % other, "21\t29185462\t1+1-\t21\t29185462\t1+1-\tINV\t0",
             "21\t29186122\t1+1-\t21\t29185462\t1+1-\tINV\t660", "21\t300\t1+1-\t21\t46944323\t1+1-\tDEL"]
    open(sites_file, "w").write("".join(l + "\n" for l in lines))
    f0, f1 = str(tmp_path / "plain.vcf"), str(tmp_path / "depth.vcf")
    run_cli(["--sites", sites_file, "--sites-vcf", f0, "-o", "21"])
    run_cli(["--sites", sites_file, "--sites-vcf", f1, "--depth", "-o", "21"])
    assert strip_depth(open(f1).read()) == T.without_command(open(f0).read())
    seen = check_depth_records(open(f1).read(), "SITE", [l.split("\t") for l in lines], run, False, 1000)
    assert [s is None for s in seen] == [True, False, True, True, False, False]
    assert seen[1] == seen[4] and seen[1][0][1] > 0                                  # (the ends in either order: the same counts)
    n_pass = int(((run.cls & 0x10) != 0).sum())
    assert 0 < seen[5][0][0] <= n_pass and seen[5][0][0] > seen[1][0][0]             # (nearly the whole sequence, its flanks clamped at both ends)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. a sharded run
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_depth_sharded_equals_one_gpu(tmp_path):
    from exclude_cases import write_case
    from fuzzgen import make_case
    rng = np.random.default_rng(3)
    cfg, streams, targets = make_case(913, n_pairs=1400)
    write_case(str(tmp_path), streams, targets, rng)
    (tmp_path / "cfg").write_text(cfg)
    d = str(tmp_path)
    args = ["-y", "-1", "-r", "1"]
    table, _ = run_cli(args, cwd=d, cfg="cfg")
    # (as in test_gpu_sites.py: --sites calls a same-chromosome type on two sequences malformed, so the table goes back without such lines)
    kept = [l for l in table.split("\n") if l.startswith("#") or not l or (l.split("\t")[6] == "CTX") == (l.split("\t")[0] != l.split("\t")[3])]
    (tmp_path / "table.txt").write_text("\n".join(kept))
    sargs = ["--sites", "table.txt", "--sites-vcf", "sites.vcf", "--vcf", "calls.vcf", "--depth", "--depth-flank", "300"] + args
    one, _ = run_cli(sargs, cwd=d, cfg="cfg")
    assert filter_cmd_lines(one) == filter_cmd_lines(table)
    ref, ref_calls = open(os.path.join(d, "sites.vcf")).read(), open(os.path.join(d, "calls.vcf")).read()
    for text in (ref, ref_calls):
        recs = [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]
        chroms = {r[0] for r in recs if r[9].split(":")[5] not in (".", "0")}
        assert len(chroms) > 1                                                       # counted records on several sequences: on several ranks
        assert any(r[4] == "<CTX>" and all(f.split(":")[5:] == [".", ".", "."] for f in r[9:]) for r in recs)
        assert "##depth_flank=300" in text
    for gpus in ("0,0", "0,0,0"):
        out, _ = run_cli(sargs, cwd=d, cfg="cfg", env=dict(BDX_GPUS=gpus))
        assert filter_cmd_lines(out) == filter_cmd_lines(one)
        assert open(os.path.join(d, "sites.vcf")).read() == ref, gpus
        assert open(os.path.join(d, "calls.vcf")).read() == ref_calls, gpus
