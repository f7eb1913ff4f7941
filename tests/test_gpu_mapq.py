"""GPU tests of --mapq: the mapping quality at one end of given sites (bdx_site_end_quality, KM) against a numpy restatement of the rule in
include/bdx.h, its consistency with the site counter (KS), the argument errors, and the CLI's SQ* / LQ* keys on the chr21 golden fixture
and on a sharded run.

The rule pinned here: a query is (site, end); (T, P) the asked end, (T', P') the other.  Record i SUPPORTS the end when it passes the
filters, its ReadFlag (class byte) is in flag_mask, it is near P on T and its mate near P' on T' -- no lower-mate condition, each mate
counts at its own end.  It is AROUND the end when tid == T, |pos + 1 - P| <= window and SAM flag 0x4 is clear, and LOW when its quality is
<= its library's minimum (bdx_lib.min_mapping_quality, or -q when that is negative; a library index out of range is library 0).  n, n_all,
n_low count the three; over the supporters' qualities qmin / qmax are the extremes, median the ceil(n / 2)-th smallest, q1 the
ceil(n / 4)-th smallest; n == 0: the four are 0.

The restatement is brute force over all records of the store -- no windows, no search, a sort instead of a histogram -- so it shares no
logic with the kernel.  Every comparison is exact.

The synthetic stores of test_gpu_sites.py carry only the qualities 0, 10 and 60, the same for both mates; here every record's quality is
overwritten before the store is turned into streams: independent per mate, spread over 0 .. 255, about a quarter at or below -q's 35, and
0, 35, 36 and 255 present.  K1 compares quality > minimum, so with -q -1 (the C ABI takes it) a quality of 0 passes: the store 'one/65/neg'
uses that, so that bin 0 of the kernel's histogram is reached."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_sites as T
from helpers import GOLDEN, ROOT, filter_cmd_lines, load_chr21, make_opts, read_bam
from runner import oracle_case, product_from_oracle
from test_mapq import KEYS, restated

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CWD = os.path.join(GOLDEN, "chr21")
WMAX = 1 << 30
FF, CTX = T.FF, T.CTX
WINDOWS = (0, 500, WMAX)


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy restatement (brute force)
# ---------------------------------------------------------------------------------------------------------------------------------
def library_minima(run):
    """every library's minimum mapping quality as K1 resolves it"""
    return np.array([int(run.lib_i[i, 0]) if int(run.lib_i[i, 0]) >= 0 else int(run.opts["min_map_qual"]) for i in range(run.nlibs)], np.int64)


def expected_quality(soa, cls, minima, sites, window):
    """(the summaries [site][end - 1] as _lib.SITE_QUALITY_DTYPE, what was seen on the way)"""
    from breakdancer_amd import _lib
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    mt, ms = soa["mtid"].astype(np.int64), soa["mpos"].astype(np.int64)
    flag = soa["flag"].astype(np.int64)
    qual = soa["bdqual"].astype(np.int64)
    ok = (cls & 0x10) != 0
    f = (cls & 15).astype(np.int64)
    lib = soa["lib"].astype(np.int64)
    least = minima[np.where((lib >= 0) & (lib < len(minima)), lib, 0)]
    mapped = (flag & 0x4) == 0
    w = int(window)
    out = np.zeros((len(sites), 2), dtype=_lib.SITE_QUALITY_DTYPE)
    seen = dict(both_ends=0, split_median=0, ctx_end2=0, same_pairs=[])
    for i, (t1, p1, t2, p2, mask) in enumerate(sites):
        in_mask = ((int(mask) >> f) & 1) != 0
        r1, r2 = (t == t1) & (np.abs(s + 1 - p1) <= w), (t == t2) & (np.abs(s + 1 - p2) <= w)
        m1, m2 = (mt == t1) & (np.abs(ms + 1 - p1) <= w), (mt == t2) & (np.abs(ms + 1 - p2) <= w)
        sup = (ok & in_mask & r1 & m2, ok & in_mask & r2 & m1)
        for e, (near, hit) in enumerate(zip((r1, r2), sup)):
            o = out[i, e]
            around = near & mapped
            o["n_all"], o["n_low"] = int(around.sum()), int((around & (qual <= least)).sum())
            qs = np.sort(qual[hit])
            n = len(qs)
            o["n"] = n
            if n:
                o["qmin"], o["qmax"] = qs[0], qs[-1]
                o["median"], o["q1"] = qs[(n + 1) // 2 - 1], qs[(n + 3) // 4 - 1]
                seen["split_median"] += int(n % 2 == 0 and qs[n // 2 - 1] != qs[n // 2])
        seen["both_ends"] += int((sup[0] & sup[1]).any())
        seen["ctx_end2"] += int(t1 != t2 and bool(sup[1].any()))
        # (for the comparison with KS: the windows do not overlap, and the supporters of the two ends are the two mates of the same pairs)
        apart = t1 != t2 or p2 - p1 > 2 * w
        if apart and sup[0].any() and sorted(soa["name_id"][sup[0]].tolist()) == sorted(soa["name_id"][sup[1]].tolist()):
            seen["same_pairs"].append(i)
    return out, seen


# ---------------------------------------------------------------------------------------------------------------------------------
# stores: those of test_gpu_sites.py with every record's quality drawn anew
# ---------------------------------------------------------------------------------------------------------------------------------
LABELS = ["one/1", "one/63", "one/64", "one/65", "one/big", "three/65", "three/big", "three/big/mixed", "three/big/l", "one/deep", "one/65/neg"]
MIXED = {"lib0": 20, "lib1": None, "lib2": 60}      # 'three/big/mixed': the libraries' own mapqual:, lib1's left to -q
DEEP = (0, 50_000, 0, 58_000)                       # 'one/deep': where its one large FF cluster lies
CASES = {}
EXPECTED = {}


def requalify(st, rng):
    """every record of the store gets a quality of its own: a quarter 0 .. 35, the rest 36 .. 255; 0, 35, 36 and 255 are made to occur"""
    recs = [r for bam in st.recs for r in bam]
    for r in recs:
        r["bdqual"] = int(rng.integers(0, 36)) if rng.random() < 0.25 else int(rng.integers(36, 256))
    if len(recs) >= 8:
        for r, v in zip(rng.choice(len(recs), size=8, replace=False), (0, 35, 36, 255, 255, 36, 37, 254)):
            recs[int(r)]["bdqual"] = v
    else:
        recs[0]["bdqual"] = 255       # (the store of one record: it passes, so that it can support its site)
    return st


def mixed_config(libs):
    return "".join("readgroup:%s\tplatform:illumina\tmap:%s\treadlen:%d.00\tlib:%s\tlower:%.2f\tupper:%.2f\tmean:%.2f\tstd:%.2f%s\n"
                   % (rg, bam, T.RL, lib, mean - 3 * std, mean + 3 * std, mean, std, "" if MIXED[lib] is None else "\tmapqual:%d" % MIXED[lib])
                   for rg, bam, lib, mean, std in libs)


def case(label):
    """(oracle run, store, merged stream) of a labelled store: built and run through the oracle once, shared by the tests"""
    if label not in CASES:
        part = label.split("/")
        libs = T.ONE_LIB if part[0] == "one" else T.THREE_LIBS
        rng = np.random.default_rng(1000 + len(label))
        if part[1] == "big":
            st = T.big_store(libs, 11 + len(label))
        elif part[1] == "deep":
            st = T.small_store(libs, 65, 72)
            st.cluster(rng, "ff", DEEP[0], DEEP[1], DEEP[2], DEEP[3], 200)       # about 150 passing pairs: two full steps of the walk and a tail
        else:
            st = T.small_store(libs, int(part[1]), 7 + int(part[1]))
        requalify(st, rng)
        opts = make_opts(illumina_long_insert=int(part[-1] == "l"), min_map_qual=-1 if part[-1] == "neg" else 35)
        cfg = mixed_config(libs) if part[-1] == "mixed" else T.config_text(libs)
        run = oracle_case(cfg, st.streams(), T.TARGETS, opts)
        CASES[label] = (run, st, run.merged_soa())
    return CASES[label]


def sites_of(label, w):
    run, st, soa = case(label)
    sites = T.make_sites(st, soa, run.cls, np.random.default_rng(len(label) + w % 1000), w)
    if "deep" in label:
        sites.append((DEEP[0], DEEP[1] + 51, DEEP[2], DEEP[3] + 51, 1 << FF))
    return sites


def expected(label, w):
    """(sites, summaries [site][end - 1], what was seen) of a store at window w: computed once, shared by the tests, never changed"""
    if (label, w) not in EXPECTED:
        run, st, soa = case(label)
        sites = sites_of(label, w)
        exp, seen = expected_quality(soa, run.cls, library_minima(run), sites, w)
        exp.setflags(write=False)
        EXPECTED[(label, w)] = (sites, exp, seen)
    return EXPECTED[(label, w)]


def check_inputs(label):
    """the conditions on the inputs, on the restatement alone: no comparison below is empty"""
    run, st, soa = case(label)
    q = soa["bdqual"]
    every = [expected(label, w) for w in WINDOWS]
    exp = np.concatenate([e.reshape(-1) for _, e, _ in every])
    total = lambda key: sum(s[key] for _, _, s in every)
    part = label.split("/")
    if part[1] != "big":
        assert len(soa["tid"]) == (int(part[1]) if part[1] != "deep" else 465) and (exp["n"] > 0).any(), label
    if len(q) >= 63:
        assert {0, 35, 36, 255} <= set(q.tolist()) and 0.15 < (q <= 35).mean() < 0.35 and len(set(q.tolist())) > 40, label
        pairs = {}
        for name, v in zip(soa["name_id"].tolist(), q.tolist()):
            pairs.setdefault(name, []).append(v)
        assert sum(len(set(v)) > 1 for v in pairs.values()) > len(pairs) // 2, label       # (the mates' qualities differ)
    if part[-1] == "neg":
        assert library_minima(run).tolist() == [-1]
        assert ((exp["n"] > 0) & (exp["qmin"] == 0)).any(), label                          # bin 0: a supporter of quality 0
        assert (exp["n_low"] == 0).all() and (exp["n_all"] > 0).any(), label               # (nothing is <= -1)
    if part[-1] == "mixed":
        assert library_minima(run).tolist() == [20, 35, 60], label
        assert ((exp["n"] > 0) & (exp["qmin"] <= 35) & (exp["qmin"] > 20)).any(), label    # a supporter only lib0's own minimum lets pass
    if part[1] == "deep":
        deep = every[1][1][-1]                                                             # window 500, the cluster's own site
        assert deep["n"][0] >= 130 and deep["n"][1] >= 130, deep
    if part[1] != "big":
        return
    at500 = every[1][1]
    assert (at500["n"] > 0).mean() > 0.3, label
    with_n = exp[exp["n"] > 0]
    assert len(set(with_n["median"].tolist())) >= 8, label
    assert total("split_median") > 0, label                                                # even n, the two middle values different
    assert (with_n["q1"] != with_n["median"]).any(), label
    assert (exp["n"] >= 65).any(), label
    assert total("both_ends") > 0, label                                                   # one record supports both ends (overlapping windows)
    assert total("ctx_end2") > 0, label
    assert ((exp["n_low"] > 0) & (exp["n_low"] < exp["n_all"])).any(), label
    assert (with_n["qmax"] == 255).any(), label


def queries_of(sites):
    """every site asked at end 1 and at end 2: the site array twice over and the ends, in the order of exp.reshape(-1)"""
    from breakdancer_amd import _lib
    arr = np.repeat(np.array(sites, dtype=_lib.SITE_DTYPE), 2)
    ends = np.tile(np.array([1, 2], np.uint8), len(sites))
    return arr, ends


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement; 2. against KS
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_site_end_quality_equals_numpy_restatement(label):
    from breakdancer_amd import _lib
    check_inputs(label)                                  # (before the GPU is used)
    run, st, soa = case(label)
    bd = product_from_oracle(run)
    np.testing.assert_array_equal(bd.read_class() & 0x3F, run.cls)   # (what K1 wrote is what the restatement reads)
    rng = np.random.default_rng(len(label))
    for w in WINDOWS:
        sites, exp, seen = expected(label, w)
        exp = exp.reshape(-1)
        arr, ends = queries_of(sites)
        got = bd.site_end_quality(arr, ends, w)
        assert got.shape == (2 * len(sites),) and got.dtype == _lib.SITE_QUALITY_DTYPE
        for k in _lib.SITE_QUALITY_DTYPE.names:
            np.testing.assert_array_equal(got[k], exp[k], err_msg="%s window=%d %s" % (label, w, k))
        for nq in (1, 4, 5):   # one block with idle waves, a full one, and one wave into the second
            order = rng.permutation(len(arr))[:nq]
            np.testing.assert_array_equal(bd.site_end_quality(arr[order], ends[order], w), exp[order])
    assert bd.site_end_quality([], [], 500).shape == (0,)
    one = bd.site_end_quality([(0, 1001, 1, 5001, 1 << CTX)], [2], 500)   # (sequences are taken as well)
    assert one.shape == (1,) and one.dtype == _lib.SITE_QUALITY_DTYPE
    bd.close()


@pytest.mark.parametrize("label", ["one/big", "three/big", "three/big/mixed", "three/big/l"])
def test_site_end_quality_counts_what_the_site_counter_counts(label):
    """where a site's windows do not overlap, a supporter of end 1 is a lower mate: n at end 1 is the site counter's row sum; and where
    the two ends' supporters are the two mates of the same pairs -- both in the store, both passing -- n at end 2 is as well"""
    run, st, soa = case(label)
    bd = product_from_oracle(run)
    checked = 0
    for w in WINDOWS:
        sites, exp, seen = expected(label, w)
        arr, ends = queries_of(sites)
        n = bd.site_end_quality(arr, ends, w)["n"].reshape(-1, 2)
        apart = np.array([t1 != t2 or p2 - p1 > 2 * w for t1, p1, t2, p2, m in sites])
        for by_library in (False, True):
            ks = bd.count_site_pairs(arr[::2], w, by_library=by_library).sum(axis=1)
            np.testing.assert_array_equal(n[apart, 0], ks[apart], err_msg="%s window=%d" % (label, w))
            same = np.array(seen["same_pairs"], dtype=np.int64)
            np.testing.assert_array_equal(n[same, 1], ks[same], err_msg="%s window=%d" % (label, w))
            np.testing.assert_array_equal(n[same, 0], ks[same])
        checked += len(seen["same_pairs"])
        assert len(seen["same_pairs"]) > 0 or w == WMAX, (label, w)      # (at 2^30 every same-chromosome site's windows overlap)
    assert checked > 0
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. bad calls
# ---------------------------------------------------------------------------------------------------------------------------------
def test_site_end_quality_refuses_bad_calls():
    import ctypes as C
    import breakdancer_amd as bda
    from breakdancer_amd import _lib
    from breakdancer_amd.api import LibraryConfig
    from runner import product_options
    run, st, soa = case("one/65")
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = np.array([(0, 1001, 1, 5001, 1 << CTX)], dtype=_lib.SITE_DTYPE)
    e1, e2 = np.array([1, 1], np.uint8), np.array([2, 2], np.uint8)
    mark = np.frombuffer(b"\xA5" * 64, dtype=_lib.SITE_QUALITY_DTYPE).copy()
    out = mark.copy()
    call = lib.bdx_site_end_quality
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]))
            for i in range(run.nlibs)]
    fresh = bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0)
    assert call(fresh.h, p(good), p(e1), 1, 500, p(out)) == 4          # BDX_ESTATE: no run yet
    fresh.close()
    bd = product_from_oracle(run)
    assert call(bd.h, None, None, 0, 500, None) == 0                   # n == 0, null pointers
    assert call(bd.h, None, p(e1), 1, 500, p(out)) == 1                # BDX_EINVAL from here on: a null array
    assert call(bd.h, p(good), None, 1, 500, p(out)) == 1
    assert call(bd.h, p(good), p(e1), 1, 500, None) == 1
    for bad_end in (0, 3, 255):
        for at in (0, 1):
            e = np.array([1, 2], np.uint8)
            e[at] = bad_end
            a = np.array([good[0].tolist(), good[0].tolist()], dtype=_lib.SITE_DTYPE)
            assert call(bd.h, p(a), p(e), 2, 500, p(out)) == 1, (bad_end, at)
    bad_sites = [(-1, 10, 0, 10, 1 << FF), (0, 10, -1, 10, 1 << FF), (0, 0, 0, 10, 1 << FF), (0, 10, 0, 0, 1 << FF), (-2, 10, -1, 10, 1 << FF),
                 (1, 10, 0, 10, 1 << CTX), (0, 11, 0, 10, 1 << FF),                       # not normalised
                 (0, 10, 0, 10, 0), (0, 10, 0, 10, 1 << 0), (0, 10, 0, 10, 1 << 6), (0, 10, 0, 10, 1 << 7), (0, 10, 0, 10, 1 << 9),
                 (0, 10, 0, 10, 1 << 10), (0, 10, 0, 10, (1 << FF) | (1 << 11)), (0, 10, 0, 10, 1 << 31)]
    for s in bad_sites:
        a = np.array([good[0].tolist(), s], dtype=_lib.SITE_DTYPE)
        assert call(bd.h, p(a), p(e2), 2, 500, p(out)) == 1, s
    for w in (-1, WMAX + 1, -2**31):
        assert call(bd.h, p(good), p(e1), 1, w, p(out)) == 1, w
    assert call(bd.h, p(good), p(e1), 2**31 + 1, 500, p(out)) == 5     # BDX_ELIMIT (checked before any site or end is read)
    assert call(bd.h, p(good), p(e1), 2**31 + 1, -1, p(out)) == 1      # (... and behind the window, as in the site counter)
    assert out.tobytes() == mark.tobytes()                             # no refused call wrote a result
    assert call(bd.h, p(good), p(e1), 1, WMAX, p(out)) == 0 and call(bd.h, p(good), p(e2), 1, 0, p(out)) == 0
    assert out[:1].tobytes() != mark[:1].tobytes() and out[1:].tobytes() == mark[1:].tobytes()
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the CLI on the chr21 golden fixture
# ---------------------------------------------------------------------------------------------------------------------------------
def run_cli(args, cwd=CWD, cfg="inv_del_bam_config", env=None):
    p = subprocess.run([EXE] + args + ([cfg] if cfg else []), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **env) if env else None, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode(), p.stderr.decode()


def strip_mapq(text):
    """a VCF minus what --mapq adds: the ##mapq_window= line, the eight ##INFO lines and the records' keys (and minus its ##command= line)"""
    out = []
    for l in text.split("\n"):
        if l.startswith(("##mapq_window=", "##command=")) or any(l.startswith("##INFO=<ID=%s," % k) for k in KEYS):
            continue
        if l and not l.startswith("#"):
            c = l.split("\t")
            c[7] = ";".join(kv for kv in c[7].split(";") if kv.split("=")[0] not in KEYS)
            l = "\t".join(c)
        out.append(l)
    return "\n".join(out)


def records_of(text):
    return [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]


def mapq_keys(text):
    """per record ID the record's --mapq keys, as printed and in their order"""
    return {r[2]: [kv for kv in r[7].split(";") if kv.split("=")[0] in KEYS] for r in records_of(text)}


def check_mapq_records(text, prefix, rows, run, targets, window, held=lambda t: True):
    """every record of a --mapq VCF against the restatement over the oracle's records; rows: the table rows the records stand for, as
    given (record k is <prefix><k + 1>).  Returns the summaries [row][end of the site]."""
    meta = [l for l in text.split("\n") if l.startswith("##")]
    assert "##mapq_window=%d" % window in meta
    for k in KEYS:
        line = [l for l in meta if l.startswith("##INFO=<ID=%s," % k)]
        assert len(line) == 1 and ",Number=2,Type=%s," % ("Float" if k == "LQF" else "Integer") in line[0], k
    got = mapq_keys(text)
    assert len(got) == len(rows) > 0
    ends = [((targets.index(r[0]), int(r[1])), (targets.index(r[3]), int(r[4]))) for r in rows]
    sites = [min(a, b) + max(a, b) + (T.TYPE_MASK[r[6]],) for (a, b), r in zip(ends, rows)]
    exp, seen = expected_quality(run.merged_soa(), run.cls, library_minima(run), sites, window)
    for k, (a, b) in enumerate(ends):
        if not held(a[0]) and not held(b[0]):
            assert got["%s%d" % (prefix, k + 1)] == [], k                 # takes no part: no keys
            continue
        e = [(int(held(sites[k][2 * j])),) + tuple(int(exp[k, j][name]) for name in ("n", "n_all", "n_low", "qmin", "q1", "median", "qmax")) for j in (0, 1)]
        assert ";" + ";".join(got["%s%d" % (prefix, k + 1)]) == restated(e[0], e[1], int(a > b)), (k, got["%s%d" % (prefix, k + 1)], e)
    return exp


@pytest.fixture(scope="module")
def chr21():
    """(the oracle run, the sequence names) of the fixture: made once, left as is"""
    run = load_chr21(make_opts()).run()
    targets = read_bam(os.path.join(CWD, run.bam_names[0]))[0]
    return run, targets


def test_cli_vcf_mapq_on_the_golden_fixture(chr21, tmp_path):
    run, targets = chr21
    golden = filter_cmd_lines(open(os.path.join(CWD, "expected_output")).read())
    f0, f1, f2 = str(tmp_path / "plain.vcf"), str(tmp_path / "mapq.vcf"), str(tmp_path / "mapq100.vcf")
    out0, _ = run_cli(["--vcf", f0])
    out1, err1 = run_cli(["--vcf", f1, "--mapq"], env=dict(BDX_TIMING="1"))
    assert filter_cmd_lines(out0) == golden and filter_cmd_lines(out1) == golden
    assert len([l for l in err1.split("\n") if l.startswith("[bdx timing] --mapq:")]) == 1
    plain, with_mapq = open(f0).read(), open(f1).read()
    assert not any(k + "=" in plain for k in KEYS) and "mapq_window" not in plain     # (without --mapq nothing of it appears)
    assert strip_mapq(plain) == T.without_command(plain)
    assert strip_mapq(with_mapq) == T.without_command(plain)
    T.vcf_parts(with_mapq)                                                           # (every INFO key has its header line; FORMAT is unchanged)
    rows = T.table_rows(out0)
    assert T.default_window(run) == 533
    exp = check_mapq_records(with_mapq, "BDX", rows, run, targets, 533)
    assert (exp["n"] > 0).all() and (exp["n_all"] > exp["n"]).all()                  # (every call of the fixture has supporters at both ends)
    assert (exp["n_low"] > 0).any()
    for keys in mapq_keys(with_mapq).values():
        assert [kv.split("=")[0] for kv in keys] == list(KEYS)                       # all eight, in order
    # the same records are held whatever the route: the host decode, the pass-1 cache (it keeps the command line), --ci and --depth beside
    fh = str(tmp_path / "host.vcf")
    outh, _ = run_cli(["--vcf", fh, "--mapq"], env=dict(BDX_DECODE="host"))
    assert filter_cmd_lines(outh) == golden and T.without_command(open(fh).read()) == T.without_command(with_mapq)
    cache, fc = str(tmp_path / "pass1.cache"), str(tmp_path / "cache.vcf")
    outc, _ = run_cli(["-C", cache, "--vcf", fc, "--mapq"])
    assert filter_cmd_lines(outc) == golden and T.without_command(open(fc).read()) == T.without_command(with_mapq)
    os.remove(fc)
    outr, _ = run_cli(["-R", cache], cfg=None)
    assert filter_cmd_lines(outr) == golden and T.without_command(open(fc).read()) == T.without_command(with_mapq)
    fa, fb = str(tmp_path / "all.vcf"), str(tmp_path / "ci_depth.vcf")
    outa, _ = run_cli(["--vcf", fa, "--ci", "--depth", "--mapq"])
    outb, _ = run_cli(["--vcf", fb, "--ci", "--depth"])
    assert filter_cmd_lines(outa) == golden
    assert strip_mapq(open(fa).read()) == T.without_command(open(fb).read()) and mapq_keys(open(fa).read()) == mapq_keys(with_mapq)
    # --mapq-window 100: other values, again the restatement's
    out2, _ = run_cli(["--vcf", f2, "--mapq", "--mapq-window", "100"])
    narrow = open(f2).read()
    assert filter_cmd_lines(out2) == golden and strip_mapq(narrow) == T.without_command(plain)
    check_mapq_records(narrow, "BDX", rows, run, targets, 100)
    assert mapq_keys(narrow) != mapq_keys(with_mapq)


def test_cli_sites_vcf_mapq_on_the_golden_fixture(chr21, tmp_path):
    run, targets = chr21
    table, _ = run_cli([])
    rows = T.table_rows(table)
    rows[1][0:3], rows[1][3:6] = rows[1][3:6], rows[1][0:3]          # one site's ends given in reverse order
    sites_file = str(tmp_path / "table.txt")
    open(sites_file, "w").write("".join("\t".join(r) + "\n" for r in rows))
    f0, f1 = str(tmp_path / "plain.vcf"), str(tmp_path / "mapq.vcf")
    golden = filter_cmd_lines(open(os.path.join(CWD, "expected_output")).read())
    out0, _ = run_cli(["--sites", sites_file, "--sites-vcf", f0])
    plain = open(f0).read()
    assert not any(k + "=" in plain for k in KEYS) and "mapq_window" not in plain
    calls = None
    for env in (None, dict(BDX_DECODE="host")):
        out1, _ = run_cli(["--sites", sites_file, "--sites-vcf", f1, "--mapq"], env=env)
        assert filter_cmd_lines(out0) == golden and filter_cmd_lines(out1) == golden
        with_mapq = open(f1).read()
        assert strip_mapq(with_mapq) == T.without_command(plain)
        exp = check_mapq_records(with_mapq, "SITE", rows, run, targets, 533)
        keys = mapq_keys(with_mapq)
        assert calls in (None, keys)
        calls = keys
        os.remove(f1)
    # the reversed site prints its ends the other way round: its first entry is the site's second end
    first = lambda kv: kv.split("=")[1].split(",")[0]
    assert first(calls["SITE2"][0]) == str(int(exp[1, 1]["n"])) and first(calls["SITE2"][5]) == str(int(exp[1, 1]["n_all"]))
    assert exp[1, 0]["n_all"] != exp[1, 1]["n_all"]                                  # (... and the two differ, so the order shows)


def test_cli_mapq_of_an_end_on_a_chromosome_the_run_did_not_read_is_a_dot(tmp_path):
    run = load_chr21(make_opts(chr_tid=22)).run()
    targets = read_bam(os.path.join(CWD, "NA19238_chr21_del_inv.bam"))[0]
    other = [t for t in targets if t != "21"][0]
    assert targets.index("21") == 22
    rows = [[other, "100", "1+1-", other, "900", "1+1-", "DEL", "800"], ["21", "29185462", "1+1-", "21", "29186122", "1+1-", "DEL", "660"],
            ["21", "500", "1+0-", other, "700", "0+1-", "CTX", "-1"]]
    sites_file = str(tmp_path / "s.txt")
    open(sites_file, "w").write("".join("\t".join(r) + "\n" for r in rows))
    out = str(tmp_path / "o.vcf")
    run_cli(["--sites", sites_file, "--sites-vcf", out, "--mapq", "-o", "21"])
    text = open(out).read()
    exp = check_mapq_records(text, "SITE", rows, run, targets, 533, held=lambda t: t == 22)
    keys = mapq_keys(text)
    assert keys["SITE1"] == []                                                       # both ends unread: takes no part
    assert exp[1, 0]["n"] > 0 and exp[1, 1]["n"] > 0 and not any("." in kv.split("=")[1].split(",") for kv in keys["SITE2"])
    entries = dict((kv.split("=")[0], kv.split("=")[1].split(",")) for kv in keys["SITE3"])     # the record prints its end on 21 first
    assert list(entries) == list(KEYS) and all(v[1] == "." for v in entries.values())
    assert all(entries[k][0] != "." for k in ("SQN", "LQA", "LQN"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. a sharded run
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_mapq_sharded_equals_one_gpu(tmp_path):
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
    sargs = ["--sites", "table.txt", "--sites-vcf", "sites.vcf", "--vcf", "calls.vcf", "--mapq"] + args
    one, _ = run_cli(sargs, cwd=d, cfg="cfg")
    assert filter_cmd_lines(one) == filter_cmd_lines(table)
    ref, ref_calls = open(os.path.join(d, "sites.vcf")).read(), open(os.path.join(d, "calls.vcf")).read()
    for text in (ref, ref_calls):
        ctx = [r for r in records_of(text) if r[4] == "<CTX>"]
        sqn = [dict(kv.split("=") for kv in mapq_keys(text)[r[2]])["SQN"].split(",") for r in ctx]
        # CTX records with supporters at their second end: those are answered by the rank that holds the SECOND chromosome, and the records
        # lie on several pairs of sequences, so that under either split below one of them has its ends on two ranks
        both = [r for r, n in zip(ctx, sqn) if int(n[0]) > 0 and int(n[1]) > 0]
        assert len({(r[0], dict(kv.split("=") for kv in r[7].split(";") if "=" in kv)["CHR2"]) for r in both}) >= 2, sqn
    for gpus in ("0,0", "0,0,0"):
        out, _ = run_cli(sargs, cwd=d, cfg="cfg", env=dict(BDX_GPUS=gpus))
        assert filter_cmd_lines(out) == filter_cmd_lines(one)
        assert open(os.path.join(d, "sites.vcf")).read() == ref, gpus
        assert open(os.path.join(d, "calls.vcf")).read() == ref_calls, gpus
