"""GPU tests of --ci: the breakpoint bounds of given sites (bdx_site_breakpoint_bounds, KI) against a numpy restatement of the rule in
include/bdx.h, their consistency with the site counter (KS), the argument errors, and the CLI's CIPOS / CIEND / CIN on the chr21 golden
fixture and on a sharded run.

The rule pinned here: the records that count for a site are the site counter's (test_gpu_sites.py), all keys pooled.  Each gives one
observation (x, reverse, U) per end -- by the forward route (record near pos1, mate near pos2) end 1 gets (pos, flag & 0x10) and end 2
(mpos, flag & 0x20), by the reverse route only the other way round; a record matching both routes is taken by the forward one; U is the
record's library's ceil(uppercutoff), 0 when negative, 2^30 when the cutoff is NaN, infinite or above 2^30; -l inverts `reverse`.  With
P = x + 1 a forward read bounds the breakpoint to [P, P + U], a reverse read to [P - U, P]; lo = the largest lower bound, hi = the
smallest upper bound, per end, clamped to [1, 2^31 - 1]; n == 0: all 0.

The restatement is brute force over all records of the store -- no windows, no search -- and writes out the both-routes tie and the
clamps.  Every comparison is exact."""
import math
import os
import subprocess

import numpy as np
import pytest

import test_gpu_sites as T
from helpers import GOLDEN, ROOT, filter_cmd_lines, load_chr21, make_opts, read_bam
from runner import oracle_case, product_from_oracle

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CWD = os.path.join(GOLDEN, "chr21")
WMAX = 1 << 30
IMAX = 2**31 - 1
FF, RF, CTX, INV = T.FF, T.RF, T.CTX, T.INV


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy restatement (brute force)
# ---------------------------------------------------------------------------------------------------------------------------------
def library_bounds(uppercutoffs):
    out = []
    for u in uppercutoffs:
        u = float(np.float32(u))
        if math.isnan(u) or math.isinf(u) or u > 2**30:
            out.append(2**30)
        else:
            out.append(max(int(math.ceil(u)), 0))
    return np.array(out, np.int64)


def expected_bounds(soa, cls, uppercutoffs, long_insert, sites, window):
    """(the bounds as _lib.SITE_BOUNDS_DTYPE, what was seen on the way): the latter counts, over the sites, the bounds set by a forward / a
    reverse read, the clamps that took effect, the contradictory and the consistent sites, and the records matching both routes"""
    from breakdancer_amd import _lib
    t, s = soa["tid"].astype(np.int64), soa["pos"].astype(np.int64)
    mt, ms = soa["mtid"].astype(np.int64), soa["mpos"].astype(np.int64)
    flag = soa["flag"].astype(np.int64)
    first = (flag & 0x40) != 0
    ok = (cls & 0x10) != 0
    f = (cls & 15).astype(np.int64)
    lower = (t < mt) | ((t == mt) & ((s < ms) | ((s == ms) & first)))
    ub = library_bounds(uppercutoffs)
    lib = soa["lib"].astype(np.int64)
    U = ub[np.where((lib >= 0) & (lib < len(ub)), lib, 0)]
    own_rev, mate_rev = ((flag & 0x10) != 0) != bool(long_insert), ((flag & 0x20) != 0) != bool(long_insert)
    w = int(window)
    out = np.zeros(len(sites), dtype=_lib.SITE_BOUNDS_DTYPE)
    seen = dict(set_by={(b, r): 0 for b in ("lo1", "hi1", "lo2", "hi2") for r in ("forward", "reverse")}, clamp_low=0, clamp_high=0,
                contradictory=0, consistent=0, both_routes=0, with_pairs=0)
    for i, (t1, p1, t2, p2, mask) in enumerate(sites):
        in_mask = ((int(mask) >> f) & 1) != 0
        r1, r2 = (t == t1) & (np.abs(s + 1 - p1) <= w), (t == t2) & (np.abs(s + 1 - p2) <= w)
        m1, m2 = (mt == t1) & (np.abs(ms + 1 - p1) <= w), (mt == t2) & (np.abs(ms + 1 - p2) <= w)
        fwd, rev = r1 & m2, r2 & m1
        hit = ok & in_mask & lower & (fwd | rev)
        n = int(hit.sum())
        out[i]["n"] = n
        if n == 0:
            continue
        seen["with_pairs"] += 1
        seen["both_routes"] += int((hit & fwd & rev).sum())
        by_fwd = fwd[hit]                                   # (a record matching both routes is taken by the forward one)
        Uh = U[hit]
        ends = ((np.where(by_fwd, s[hit], ms[hit]), np.where(by_fwd, own_rev[hit], mate_rev[hit])),
                (np.where(by_fwd, ms[hit], s[hit]), np.where(by_fwd, mate_rev[hit], own_rev[hit])))
        vals = []
        for e, (x, rv) in enumerate(ends):
            P = x + 1
            lows, highs = np.where(rv, P - Uh, P), np.where(rv, P, P + Uh)
            lo, hi = int(lows.max()), int(highs.min())
            for name, v, arr in (("lo%d" % (e + 1), lo, lows), ("hi%d" % (e + 1), hi, highs)):
                setters = rv[arr == v]
                seen["set_by"][(name, "reverse")] += int(setters.any())
                seen["set_by"][(name, "forward")] += int((~setters).any())
                seen["clamp_low"] += int(v < 1)
                seen["clamp_high"] += int(v > IMAX)
            lo, hi = min(max(lo, 1), IMAX), min(max(hi, 1), IMAX)
            out[i]["lo%d" % (e + 1)], out[i]["hi%d" % (e + 1)] = lo, hi
            vals.append((lo, hi))
        seen["contradictory"] += int(any(lo > hi for lo, hi in vals))
        seen["consistent"] += int(all(lo <= hi for lo, hi in vals))
    return out, seen


# ---------------------------------------------------------------------------------------------------------------------------------
# stores: those of test_gpu_sites.py, and two whose middle library has no usable cutoff
# ---------------------------------------------------------------------------------------------------------------------------------
LABELS = T.LABELS + ["three/big/inf", "three/big/2^30+5"]
WINDOWS = (0, 500, WMAX)
ODD_CUTOFF = {"inf": "inf", "2^30+5": "%d.00" % (2**30 + 5)}
CASES = {}
EXPECTED = {}


def odd_store(which):
    """big_store with lib1's uppercutoff replaced, a lone FF pair of lib1 beyond the FAR cluster (forward reads whose P + 2^30 passes
    2^31 - 1) and a lone RF pair in front of everything (a reverse read whose P - U lies below 1)"""
    libs = T.THREE_LIBS
    st = T.big_store(libs, 23 + len(which))
    st.pair(1, 3, T.FAR + 50_000, 3, T.FAR + 50_400, False, False)
    st.pair(0, 0, 5, 0, 60, True, False)
    cfg = "".join("readgroup:%s\tplatform:illumina\tmap:%s\treadlen:%d.00\tlib:%s\tlower:%.2f\tupper:%s\tmean:%.2f\tstd:%.2f\n"
                  % (rg, bam, T.RL, lib, mean - 3 * std, ODD_CUTOFF[which] if lib == "lib1" else "%.2f" % (mean + 3 * std), mean, std)
                  for rg, bam, lib, mean, std in libs)
    run = oracle_case(cfg, st.streams(), T.TARGETS, make_opts())
    return run, st, run.merged_soa()


def case(label):
    if label not in CASES:
        which = label.split("/")[-1]
        CASES[label] = odd_store(which) if which in ODD_CUTOFF else T.store_case(label)
    return CASES[label]


def sites_of(label, w):
    run, st, soa = case(label)
    sites = T.make_sites(st, soa, run.cls, np.random.default_rng(len(label) + w % 1000), w)
    if label.split("/")[-1] in ODD_CUTOFF:
        sites += [(3, T.FAR + 50_001, 3, T.FAR + 50_401, 1 << FF), (0, 6, 0, 61, 1 << RF)]
    return sites


def expected(label, w):
    """(sites, bounds, what was seen) of a store at window w: computed once, shared by the tests, never changed"""
    if (label, w) not in EXPECTED:
        run, st, soa = case(label)
        sites = sites_of(label, w)
        exp, seen = expected_bounds(soa, run.cls, run.lib_f[:, 2], run.opts["illumina_long_insert"], sites, w)
        exp.setflags(write=False)
        EXPECTED[(label, w)] = (sites, exp, seen)
    return EXPECTED[(label, w)]


def check_inputs(label):
    """the conditions on the inputs, on the restatement alone: no comparison below is empty"""
    run, st, soa = case(label)
    seen = [expected(label, w)[2] for w in WINDOWS]
    total = lambda key: sum(s[key] for s in seen)
    if "big" not in label:
        assert len(soa["tid"]) == int(label.split("/")[1]) and total("with_pairs") > 0
        return
    sites, exp, at500 = expected(label, 500)
    assert (exp["n"] > 0).mean() > 0.3, label
    assert total("contradictory") > 0 and total("consistent") > 0, label
    for key in seen[0]["set_by"]:
        assert sum(s["set_by"][key] for s in seen) > 0, (label, key)
    assert total("both_routes") > 0, label
    if label.split("/")[-1] in ODD_CUTOFF:
        ub = library_bounds(run.lib_f[:, 2])
        assert ub[1] == 2**30 and ub[0] < 1000 and ub[2] < 1000
        assert total("clamp_high") > 0 and total("clamp_low") > 0, label
    if label.endswith("/l"):
        assert total("clamp_low") > 0, label       # (reads that -l turns round in front of the store's first cluster)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement; 2. against KS
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_site_bounds_equal_numpy_restatement(label):
    from breakdancer_amd import _lib
    check_inputs(label)                                  # (before the GPU is used)
    run, st, soa = case(label)
    bd = product_from_oracle(run)
    np.testing.assert_array_equal(bd.read_class() & 0x3F, run.cls)   # (what K1 wrote is what the restatement reads)
    rng = np.random.default_rng(len(label))
    for w in WINDOWS:
        sites, exp, seen = expected(label, w)
        arr = np.array(sites, dtype=_lib.SITE_DTYPE)
        got = bd.site_breakpoint_bounds(arr, w)
        assert got.shape == (len(sites),) and got.dtype == _lib.SITE_BOUNDS_DTYPE
        for k in ("n", "lo1", "hi1", "lo2", "hi2"):
            np.testing.assert_array_equal(got[k], exp[k], err_msg="%s window=%d %s" % (label, w, k))
        for nq in (1, 4, 5):   # one block with idle waves, a full one, and one wave into the second
            order = rng.permutation(len(sites))[:nq]
            np.testing.assert_array_equal(bd.site_breakpoint_bounds(arr[order], w), exp[order])
    assert bd.site_breakpoint_bounds([], 500).shape == (0,)
    one = bd.site_breakpoint_bounds([(0, 1001, 1, 5001, 1 << CTX)], 500)   # (a sequence of tuples is taken as well)
    assert one.shape == (1,) and one.dtype == _lib.SITE_BOUNDS_DTYPE
    bd.close()


@pytest.mark.parametrize("label", LABELS)
def test_site_bounds_count_what_the_site_counter_counts(label):
    from breakdancer_amd import _lib
    run, st, soa = case(label)
    bd = product_from_oracle(run)
    nonzero = 0
    for w in WINDOWS:
        arr = np.array(sites_of(label, w), dtype=_lib.SITE_DTYPE)
        n = bd.site_breakpoint_bounds(arr, w)["n"]
        for by_library in (False, True):
            np.testing.assert_array_equal(n, bd.count_site_pairs(arr, w, by_library=by_library).sum(axis=1), err_msg="%s window=%d" % (label, w))
        nonzero += int((n > 0).sum())
    assert nonzero > 0
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. bad calls
# ---------------------------------------------------------------------------------------------------------------------------------
def test_site_bounds_refuse_bad_calls():
    import ctypes as C
    import breakdancer_amd as bda
    from breakdancer_amd import _lib
    from breakdancer_amd.api import LibraryConfig
    from runner import product_options
    run, st, soa = T.store_case("one/65")
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = np.array([(0, 1001, 1, 5001, 1 << CTX)], dtype=_lib.SITE_DTYPE)
    out = np.zeros(4, dtype=_lib.SITE_BOUNDS_DTYPE)
    call = lib.bdx_site_breakpoint_bounds
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]))
            for i in range(run.nlibs)]
    fresh = bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0)
    assert call(fresh.h, p(good), 1, 500, p(out)) == 4          # BDX_ESTATE: no run yet
    fresh.close()
    bd = product_from_oracle(run)
    assert call(bd.h, p(good), 1, 500, p(out)) == 0
    assert call(bd.h, None, 0, 500, None) == 0                   # n == 0, null pointers
    assert call(bd.h, None, 1, 500, p(out)) == 1                 # BDX_EINVAL from here on: a null array
    assert call(bd.h, p(good), 1, 500, None) == 1
    bad_sites = [(-1, 10, 0, 10, 1 << FF), (0, 10, -1, 10, 1 << FF), (0, 0, 0, 10, 1 << FF), (0, 10, 0, 0, 1 << FF), (-2, 10, -1, 10, 1 << FF),
                 (1, 10, 0, 10, 1 << CTX), (0, 11, 0, 10, 1 << FF),                       # not normalised
                 (0, 10, 0, 10, 0), (0, 10, 0, 10, 1 << 0), (0, 10, 0, 10, 1 << 6), (0, 10, 0, 10, 1 << 7), (0, 10, 0, 10, 1 << 9),
                 (0, 10, 0, 10, 1 << 10), (0, 10, 0, 10, (1 << FF) | (1 << 11)), (0, 10, 0, 10, 1 << 31)]
    for s in bad_sites:
        a = np.array([good[0].tolist(), s], dtype=_lib.SITE_DTYPE)
        assert call(bd.h, p(a), 2, 500, p(out)) == 1, s
    for w in (-1, WMAX + 1, -2**31):
        assert call(bd.h, p(good), 1, w, p(out)) == 1, w
    assert call(bd.h, p(good), 1, WMAX, p(out)) == 0 and call(bd.h, p(good), 1, 0, p(out)) == 0
    assert call(bd.h, p(good), 2**31 + 1, 500, p(out)) == 5         # BDX_ELIMIT (checked before any site is read)
    assert call(bd.h, p(good), 2**31 + 1, -1, p(out)) == 1          # (... and behind the window, as in the site counter)
    assert lib.bdx_count_site_pairs(bd.h, p(good), 2**31 + 1, -1, 0, p(np.zeros(4, np.uint32))) == 1
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the CLI on the chr21 golden fixture
# ---------------------------------------------------------------------------------------------------------------------------------
CI_KEYS = ("CIPOS", "CIEND", "CIPOS2", "CIN")


def run_cli(args, cwd=CWD, cfg="inv_del_bam_config", env=None):
    p = subprocess.run([EXE] + args + [cfg], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **env) if env else None, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode(), p.stderr.decode()


def strip_ci(text):
    """a VCF minus what --ci adds: the ##ci_window= line, the four ##INFO lines and the records' CI keys (and minus its ##command= line)"""
    out = []
    for l in text.split("\n"):
        if l.startswith(("##ci_window=", "##command=")) or any(l.startswith("##INFO=<ID=%s," % k) for k in CI_KEYS):
            continue
        if l and not l.startswith("#"):
            c = l.split("\t")
            c[7] = ";".join(kv for kv in c[7].split(";") if kv.split("=")[0] not in CI_KEYS)
            l = "\t".join(c)
        out.append(l)
    return "\n".join(out)


def info_of(rec):
    return dict(kv.split("=") if "=" in kv else (kv, None) for kv in rec[7].split(";"))


def check_ci_records(text, prefix, rows, run, targets, window):
    """every record of a --ci VCF against the restatement over the oracle's records; rows: the table rows the records stand for, as given
    (record k is <prefix><k + 1>).  Returns the CINs in table order."""
    meta, samples, recs = T.vcf_parts(text)
    assert "##ci_window=%d" % window in meta
    assert all(any(l.startswith("##INFO=<ID=%s," % k) for l in meta) for k in CI_KEYS)
    by_id = {r[2]: r for r in recs}
    assert len(recs) == len(rows) > 0
    ends = [((targets.index(r[0]), int(r[1])), (targets.index(r[3]), int(r[4]))) for r in rows]
    sites = [min(a, b) + max(a, b) + (T.TYPE_MASK[r[6]],) for (a, b), r in zip(ends, rows)]
    exp, seen = expected_bounds(run.merged_soa(), run.cls, run.lib_f[:, 2], 0, sites, window)
    cins = []
    for k, (row, (a, b)) in enumerate(zip(rows, ends)):
        info = info_of(by_id["%s%d" % (prefix, k + 1)])
        e = exp[k]
        if e["n"] == 0:
            assert not set(info) & set(CI_KEYS), (k, info)
            cins.append(0)
            continue
        second = "CIEND" if "END" in info else "CIPOS2"
        assert ("END" in info) == (a[0] == b[0] and b[1] >= a[1])
        assert set(info) & set(CI_KEYS) == {"CIPOS", second, "CIN"}, (k, info)
        b1, b2 = ((e["lo2"], e["hi2"]), (e["lo1"], e["hi1"])) if a > b else ((e["lo1"], e["hi1"]), (e["lo2"], e["hi2"]))   # (swapped back)
        for key, (lo, hi), P in (("CIPOS", b1, a[1]), (second, b2, b[1])):
            lo, hi = int(lo), int(hi)
            got = [int(x) for x in info[key].split(",")]
            assert got == [min(lo, hi, P) - P, max(lo, hi, P) - P], (k, key, info[key], lo, hi, P)
            assert got[0] <= 0 <= got[1]
        assert int(info["CIN"]) == int(e["n"])
        cins.append(int(info["CIN"]))
    return cins


@pytest.fixture(scope="module")
def chr21():
    """(the oracle run, the sequence names, the plain table, its rows, the --vcf output without --ci) of the fixture: made once, left as is"""
    run = load_chr21(make_opts()).run()
    targets = read_bam(os.path.join(CWD, run.bam_names[0]))[0]
    return run, targets


def test_cli_vcf_ci_on_the_golden_fixture(chr21, tmp_path):
    run, targets = chr21
    golden = filter_cmd_lines(open(os.path.join(CWD, "expected_output")).read())
    f0, f1, f2 = str(tmp_path / "plain.vcf"), str(tmp_path / "ci.vcf"), str(tmp_path / "ci100.vcf")
    out0, _ = run_cli(["--vcf", f0])
    out1, err1 = run_cli(["--vcf", f1, "--ci"], env=dict(BDX_TIMING="1"))
    assert filter_cmd_lines(out0) == golden and filter_cmd_lines(out1) == golden
    assert len([l for l in err1.split("\n") if l.startswith("[bdx timing] --ci:")]) == 1
    plain, with_ci = open(f0).read(), open(f1).read()
    assert not any(k in plain for k in CI_KEYS) and "ci_window" not in plain        # (without --ci nothing of it appears)
    assert strip_ci(plain) == T.without_command(plain)
    assert strip_ci(with_ci) == T.without_command(plain)
    rows = T.table_rows(out0)
    assert T.default_window(run) == 533
    cins = check_ci_records(with_ci, "BDX", rows, run, targets, 533)
    assert cins == [2, 21, 1, 1]                                                    # (the site DVs of this table at window 533)
    for r in T.vcf_parts(with_ci)[2]:
        assert {"CIPOS", "CIEND", "CIN"} <= set(info_of(r))
    # BDX_DECODE=host: the same records are held
    fh = str(tmp_path / "host.vcf")
    outh, _ = run_cli(["--vcf", fh, "--ci"], env=dict(BDX_DECODE="host"))
    assert filter_cmd_lines(outh) == golden and T.without_command(open(fh).read()) == T.without_command(with_ci)
    # --ci-window 100: other values, again the restatement's
    out2, _ = run_cli(["--vcf", f2, "--ci", "--ci-window", "100"])
    narrow = open(f2).read()
    assert filter_cmd_lines(out2) == golden and strip_ci(narrow) == T.without_command(plain)
    cins100 = check_ci_records(narrow, "BDX", rows, run, targets, 100)
    ci_of = lambda text: [[(k, v) for k, v in sorted(info_of(r).items()) if k in CI_KEYS] for r in T.vcf_parts(text)[2]]
    assert cins100 != cins and ci_of(narrow) != ci_of(with_ci)


def test_cli_sites_vcf_ci_on_the_golden_fixture(chr21, tmp_path):
    run, targets = chr21
    table, _ = run_cli([])
    rows = T.table_rows(table)
    rows[1][0:3], rows[1][3:6] = rows[1][3:6], rows[1][0:3]          # one site's ends given in reverse order
    sites_file = str(tmp_path / "table.txt")
    open(sites_file, "w").write("".join("\t".join(r) + "\n" for r in rows))
    f0, f1 = str(tmp_path / "plain.vcf"), str(tmp_path / "ci.vcf")
    golden = filter_cmd_lines(open(os.path.join(CWD, "expected_output")).read())
    out0, _ = run_cli(["--sites", sites_file, "--sites-vcf", f0])
    plain = open(f0).read()
    assert not any(k in plain for k in CI_KEYS) and "ci_window" not in plain
    for env in (None, dict(BDX_DECODE="host")):
        out1, _ = run_cli(["--sites", sites_file, "--sites-vcf", f1, "--ci"], env=env)
        assert filter_cmd_lines(out0) == golden and filter_cmd_lines(out1) == golden
        with_ci = open(f1).read()
        assert strip_ci(with_ci) == T.without_command(plain)
        assert check_ci_records(with_ci, "SITE", rows, run, targets, 533) == [2, 21, 1, 1]
        by_id = {r[2]: info_of(r) for r in T.vcf_parts(with_ci)[2]}
        assert "CIPOS2" in by_id["SITE2"] and "END" not in by_id["SITE2"]             # (the reversed one prints no END)
        assert all({"CIPOS", "CIEND", "CIN"} <= set(by_id["SITE%d" % k]) for k in (1, 3, 4))
        os.remove(f1)
    out2, _ = run_cli(["--sites", sites_file, "--sites-vcf", f1, "--ci", "--ci-window", "100"])
    assert strip_ci(open(f1).read()) == T.without_command(plain)
    assert check_ci_records(open(f1).read(), "SITE", rows, run, targets, 100) != [2, 21, 1, 1]


def test_cli_ci_of_a_site_on_a_chromosome_the_run_did_not_read_is_absent(tmp_path):
    targets = read_bam(os.path.join(CWD, "NA19238_chr21_del_inv.bam"))[0]
    other = [t for t in targets if t != "21"][0]
    sites_file = str(tmp_path / "s.txt")
    open(sites_file, "w").write("%s\t100\t1+1-\t%s\t900\t1+1-\tDEL\t800\n21\t29185462\t1+1-\t21\t29186122\t1+1-\tDEL\n" % (other, other) +
                                "21\t500\t1+0-\t%s\t700\t0+1-\tCTX\t-1\n" % other)
    out = str(tmp_path / "o.vcf")
    run_cli(["--sites", sites_file, "--sites-vcf", out, "--ci", "-o", "21"])
    meta, samples, recs = T.vcf_parts(open(out).read())
    by_id = {r[2]: info_of(r) for r in recs}
    assert not set(by_id["SITE1"]) & set(CI_KEYS) and not set(by_id["SITE3"]) & set(CI_KEYS)
    assert {"CIPOS", "CIEND", "CIN"} <= set(by_id["SITE2"]) and by_id["SITE2"]["CIN"] == "21"


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. a sharded run
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_ci_sharded_equals_one_gpu(tmp_path):
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
    sargs = ["--sites", "table.txt", "--sites-vcf", "sites.vcf", "--vcf", "calls.vcf", "--ci"] + args
    one, _ = run_cli(sargs, cwd=d, cfg="cfg")
    assert filter_cmd_lines(one) == filter_cmd_lines(table)
    ref, ref_calls = open(os.path.join(d, "sites.vcf")).read(), open(os.path.join(d, "calls.vcf")).read()
    for text in (ref, ref_calls):
        recs = T.vcf_parts(text)[2]
        ctx = [info_of(r) for r in recs if r[4] == "<CTX>"]
        assert ctx and any("CIPOS" in i and "CIPOS2" in i and int(i["CIN"]) > 0 for i in ctx)     # a CTX record with its bounds, from tid1's rank
        assert any("CIEND" in info_of(r) for r in recs)
    for gpus in ("0,0", "0,0,0"):
        out, _ = run_cli(sargs, cwd=d, cfg="cfg", env=dict(BDX_GPUS=gpus))
        assert filter_cmd_lines(out) == filter_cmd_lines(one)
        assert open(os.path.join(d, "sites.vcf")).read() == ref, gpus
        assert open(os.path.join(d, "calls.vcf")).read() == ref_calls, gpus
