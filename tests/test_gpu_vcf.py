"""GPU tests of --vcf: the junction counter (bdx_count_junction_pairs, K8) against a numpy restatement, and the CLI's VCF on the chr21
golden fixtures and on sharded runs.

Definitions pinned here: a junction P is the boundary between base P and P + 1; a read counts for it when it is a normal pair's
leftmost mate (pass, ReadFlag NORMAL_FR / NORMAL_RF, pos < mpos) and its fragment [pos + 1, pos + |isize|] covers P and P + 1.  A query's
answer counts the reads that cover at least one of its junctions."""
import math
import os
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, OracleRun, ROOT, filter_cmd_lines, load_chr21, make_opts, read_bam
from runner import product_from_oracle

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CWD = os.path.join(GOLDEN, "chr21")


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def normal_left(soa, cls):
    """the normal-pair bit, derived from the oracle's class bits (pass, ReadFlag) and the record itself"""
    f = cls & 15
    return ((cls & 0x10) != 0) & ((f == 6) | (f == 7)) & (soa["pos"].astype(np.int64) < soa["mpos"].astype(np.int64))


def expected_counts(soa, nl, keys, nkeys, tid, pa, pb):
    t = soa["tid"].astype(np.int64)[nl]
    s = soa["pos"].astype(np.int64)[nl]
    L = np.abs(soa["isize"].astype(np.int64))[nl]
    k = keys.astype(np.int64)[nl] if nkeys > 1 else np.zeros(len(t), np.int64)
    k = np.where(k < nkeys, k, 0)
    maxl = int(L.max()) if len(L) else 0
    out = np.zeros((len(tid), nkeys), np.uint32)
    for c in np.unique(tid):
        m = t == c
        cs, cl, ck = s[m], L[m], k[m]   # (sorted by position within a chromosome)
        for i in np.nonzero(tid == c)[0]:
            a, b = int(pa[i]), int(pb[i])
            lo, hi = np.searchsorted(cs, a + 1 - maxl, "left"), np.searchsorted(cs, b - 1, "right")
            ss, ll = cs[lo:hi], cl[lo:hi]
            cov = ((ss + 1 <= a) & (a + 1 <= ss + ll)) | ((ss + 1 <= b) & (b + 1 <= ss + ll))
            out[i] = np.bincount(ck[lo:hi][cov], minlength=nkeys)[:nkeys]
    return out


def genotype(dr, dv):
    """the documented model: alt-read probability 0.01 / 0.5 / 0.99, PL rounded half away from zero, GQ = second-smallest PL capped at 99"""
    if dr is None or dr + dv == 0:
        return None
    lk = [dv * math.log10(p) + dr * math.log10(1.0 - p) for p in (0.01, 0.5, 0.99)]
    best = max(lk)
    pl = []
    for x in lk:
        v = -10.0 * (x - best)
        f = math.floor(v)
        pl.append(int(f + 1 if v - f >= 0.5 else f))
    gt = min(range(3), key=lambda g: (pl[g], g))
    return ("0/0", "0/1", "1/1")[gt], min(99, sorted(pl)[1]), pl


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def cfg_line(rg, bam, lib, mean, std):
    return "readgroup:%s\tplatform:illumina\tmap:%s\treadlen:100.00\tlib:%s\tlower:%.2f\tupper:%.2f\tmean:%.2f\tstd:%.2f\n" % (
        rg, bam, lib, mean - 3 * std, mean + 3 * std, mean, std)


def synthetic_run(libs, lib_bam, bams, lengths, opts, only_tids):
    from breakdancer_amd.synth import make_genome
    d = make_genome(lengths, coverage=30.0, seed=5, libs=libs, lib_bam=lib_bam, n_translocations=40, only_tids=only_tids)
    cfg = "".join(cfg_line("rg%d" % i, bams[lib_bam[i]], "lib%d" % i, m, s) for i, (m, s) in enumerate(libs))
    run = OracleRun(cfg, opts)
    run.set_targets(["c%d" % i for i in range(len(lengths))])
    for b in range(len(bams)):
        m = d["bam"] == b
        st = {k: d[k][m] for k in ("tid", "pos", "mtid", "mpos", "isize", "flag")}
        st["qlen"] = d["qlen"][m].astype(np.int32)
        st["bdqual"] = d["mapq"][m]
        st["lib"] = d["lib"][m].astype(np.int32)
        st["name_id"] = d["name_key"][m]
        run.set_stream(b, st)
    return run.run()


def make_queries(rng, lengths, soa, lmax, n=3000):
    tid = rng.integers(0, len(lengths) + 1, n)                       # (the last one is beyond the header: no reads)
    L = np.array(list(lengths) + [100000])
    pa = rng.integers(1, L[tid] + 1000)
    kind = rng.integers(0, 4, n)
    span = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(1, lmax - 1, n), np.where(kind == 2, rng.integers(lmax - 3, lmax + 3, n),
                                                                                          rng.integers(lmax, 20 * lmax, n))))
    pb = pa + span
    edges = []
    for t in range(len(lengths)):
        m = soa["tid"] == t
        if m.any():
            first, last = int(soa["pos"][m].min()), int(soa["pos"][m].max())
            edges += [(t, 1, 1), (t, 1, max(first, 1)), (t, max(first - 5, 1), first + 3), (t, last, last), (t, last + 2, last + 500),
                      (t, last + 1000, last + 1000)]
        else:
            edges += [(t, 1, 1), (t, 500, 5000)]
        c = int(rng.integers(10000, lengths[t] - 10000))
        edges += [(t, c, c + 1), (t, c, c + lmax - 2), (t, c, c + lmax - 1), (t, c, c + lmax), (t, c, c + 2 * lmax), (t, c + 10, c + 12)]
    e = np.array(edges, np.int64)
    return (np.concatenate([tid, e[:, 0]]).astype(np.int32), np.concatenate([pa, e[:, 1]]).astype(np.int32),
            np.concatenate([pb, e[:, 2]]).astype(np.int32))


CASES = [("three libraries in two files", ((400.0, 30.0), (350.0, 40.0), (500.0, 50.0)), (0, 0, 1), ["a.bam", "b.bam"], {}),
         ("three libraries in two files, -l", ((400.0, 30.0), (350.0, 40.0), (500.0, 50.0)), (0, 0, 1), ["a.bam", "b.bam"],
          dict(illumina_long_insert=1)),
         ("one library, one file", ((420.0, 35.0),), (0,), ["a.bam"], {})]


@pytest.mark.parametrize("label,libs,lib_bam,bams,kw", CASES, ids=[c[0] for c in CASES])
def test_junction_counts_equal_numpy_restatement(label, libs, lib_bam, bams, kw):
    lengths = (1_500_000, 1_200_000, 400_000, 900_000)
    run = synthetic_run(libs, lib_bam, bams, lengths, make_opts(**kw), only_tids=(0, 1, 3))   # chromosome 2 has no reads
    bd = product_from_oracle(run)
    soa = run.merged_soa()
    assert len(soa["tid"]) > 500_000 and not (soa["tid"] == 2).any()
    nl = normal_left(soa, run.cls)
    assert nl.sum() > 100_000
    np.testing.assert_array_equal((bd.read_class() & 0x40) != 0, nl)   # (what K1 marked is what the restatement derives)
    lmax = int(max(math.floor(l[0] + 3 * l[1]) for l in libs))
    tid, pa, pb = make_queries(np.random.default_rng(len(libs) + len(kw)), lengths, soa, lmax)
    for by_library, keys, nkeys in ((False, soa["bam"], len(bams)), (True, soa["lib"], len(libs))):
        got = bd.count_junction_pairs(tid, pa, pb, by_library=by_library)
        assert got.shape == (len(tid), nkeys) and got.dtype == np.uint32
        exp = expected_counts(soa, nl, keys, nkeys, tid, pa, pb)
        np.testing.assert_array_equal(got, exp, err_msg="%s by_library=%s" % (label, by_library))
        assert (exp.sum(axis=1) > 0).mean() > 0.3
    assert bd.count_junction_pairs([], [], []).shape == (0, len(bams))
    bd.close()


def test_junction_counts_refuse_bad_calls():
    import ctypes as C
    from breakdancer_amd import _lib
    run = load_chr21(make_opts()).run()
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    t, a, b = np.array([22], np.int32), np.array([29185056], np.int32), np.array([29185377], np.int32)
    out = np.zeros(4, np.uint32)
    import breakdancer_amd as bda
    from runner import product_options
    from breakdancer_amd.api import LibraryConfig
    libs = [LibraryConfig(*[float(x) for x in run.lib_f[i]], min_mapping_quality=int(run.lib_i[i, 0]), bam_file_index=int(run.lib_i[i, 1]))
            for i in range(run.nlibs)]
    fresh = bda.BreakDancer(product_options(run.opts), libs, run.nbams, ntids=0, max_read_window_size=run.w0)
    assert lib.bdx_count_junction_pairs(fresh.h, p(t), p(a), p(b), 1, 0, p(out)) == 4   # BDX_ESTATE: no run yet
    fresh.close()
    bd = product_from_oracle(run)
    assert lib.bdx_count_junction_pairs(bd.h, p(t), p(a), p(b), 1, 0, p(out)) == 0
    assert lib.bdx_count_junction_pairs(bd.h, None, None, None, 0, 0, None) == 0            # n == 0
    for args in ((None, p(a), p(b), p(out)), (p(t), None, p(b), p(out)), (p(t), p(a), None, p(out)), (p(t), p(a), p(b), None)):
        assert lib.bdx_count_junction_pairs(bd.h, *args[:3], 1, 0, args[3]) == 1            # BDX_EINVAL: null array
    for tt, aa, bb in ((-1, 10, 10), (22, 0, 10), (22, 11, 10)):
        q = [np.array([v], np.int32) for v in (tt, aa, bb)]
        assert lib.bdx_count_junction_pairs(bd.h, p(q[0]), p(q[1]), p(q[2]), 1, 0, p(out)) == 1, (tt, aa, bb)
    bd.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the CLI on the chr21 golden fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
GOLDEN_CASES = [("expected_output.cn_per_lib", ["-a", "-o", "21"]), ("expected_output.cn_per_lib.af", ["-a", "-h", "-o", "21"]),
                ("expected_output.af", ["-h", "-o", "21"]), ("expected_output", ["-o", "21"]), ("expected_output", []),
                ("expected_output.af", ["-h"])]


def run_cli(args, cwd=CWD, cfg="inv_del_bam_config", env=None):
    p = subprocess.run([EXE] + args + [cfg], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **env) if env else None, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode()


def parse_vcf(text):
    lines = text.rstrip("\n").split("\n")
    meta = [l for l in lines if l.startswith("##")]
    head = [l for l in lines if l.startswith("#CHROM")]
    recs = [l.split("\t") for l in lines if not l.startswith("#")]
    assert lines[0] == "##fileformat=VCFv4.2" and len(head) == 1
    cols = head[0].split("\t")
    assert cols[:9] == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"]
    info_ids = {l.split("ID=")[1].split(",")[0] for l in meta if l.startswith("##INFO=")}
    fmt_ids = {l.split("ID=")[1].split(",")[0] for l in meta if l.startswith("##FORMAT=")}
    contigs = [l.split("ID=")[1].split(",")[0] for l in meta if l.startswith("##contig=")]
    for r in recs:
        assert len(r) == len(cols), r                                   # (tab count)
        for kv in r[7].split(";"):
            assert kv.split("=")[0] in info_ids, kv
        assert r[8] == "GT:GQ:PL:DR:DV" and set(r[8].split(":")) <= fmt_ids
    order = [(contigs.index(r[0]), int(r[1])) for r in recs]
    assert order == sorted(order)
    return cols[9:], contigs, recs


def check_vcf_against_table(table, vcf_text, samples_exp, dr_exp, by_lib, dr_unknown=False, af_col=False):
    samples, contigs, recs = parse_vcf(vcf_text)
    assert samples == samples_exp
    rows = [l.split("\t") for l in table.split("\n") if l and not l.startswith("#")]
    assert len(recs) == len(rows)
    by_id = {r[2]: r for r in recs}
    for k, row in enumerate(rows):
        r = by_id["BDX%d" % (k + 1)]
        assert r[0] == row[0] and r[1] == row[1] and r[3] == "N" and r[4] == "<%s>" % row[6] and r[5] == row[8] and r[6] == "PASS"
        info = dict(kv.split("=") if "=" in kv else (kv, None) for kv in r[7].split(";"))
        assert "IMPRECISE" in info and info["SVTYPE"] == row[6] and info["CHR2"] == row[3] and info["POS2"] == row[4]
        assert ("END" in info) == (row[0] == row[3] and int(row[4]) >= int(row[1]))
        if "END" in info:
            assert info["END"] == row[4]
        assert ("SVLEN" in info) == (row[6] in ("DEL", "INS")) and (row[6] not in ("DEL", "INS") or int(info["SVLEN"]) == -int(row[7]))
        assert info["ORI1"] == row[2] and info["ORI2"] == row[5] and info["NREADS"] == row[9]
        if af_col:   # (the table prints a NaN frequency as "-nan"; the VCF as missing)
            af = float(row[11])
            assert info["BDAF"] == "." if math.isnan(af) else abs(float(info["BDAF"]) - af) <= 1e-4 * max(1.0, abs(af)), (info["BDAF"], af)
        dv_exp = [0] * len(samples)
        if row[10] != "NA":
            for ent in row[10].split(":"):
                name, cnt = ent.split("|")
                dv_exp[samples.index(os.path.basename(name))] += int(cnt.split(",")[0])
        for j, f in enumerate(r[9:]):
            gt, gq, pl, dr, dv = f.split(":")
            assert int(dv) == dv_exp[j]
            if dr_unknown:
                assert (gt, gq, pl, dr) == ("./.", ".", ".", ".")
                continue
            assert int(dr) == dr_exp[k][j], (k, j, f)
            g = genotype(int(dr), int(dv))
            if g is None:
                assert (gt, gq, pl) == ("./.", ".", ".")
            else:
                assert (gt, int(gq), [int(x) for x in pl.split(",")]) == g, f


def chr21_expected_dr(table, kw, by_lib):
    run = load_chr21(make_opts(**kw)).run()
    targets = read_bam(os.path.join(CWD, run.bam_names[0]))[0]
    soa = run.merged_soa()
    nl = normal_left(soa, run.cls)
    rows = [l.split("\t") for l in table.split("\n") if l and not l.startswith("#")]
    tid, pa, pb, owner = [], [], [], []
    for k, row in enumerate(rows):
        c1, c2, p1, p2 = targets.index(row[0]), targets.index(row[3]), int(row[1]), int(row[4])
        if c1 == c2:
            tid.append(c1); pa.append(min(p1, p2)); pb.append(max(p1, p2)); owner.append(k)
        else:
            for c, q in ((c1, p1), (c2, p2)):
                tid.append(c); pa.append(q); pb.append(q); owner.append(k)
    keys, nkeys = (soa["lib"], run.nlibs) if by_lib else (soa["bam"], run.nbams)
    cnt = expected_counts(soa, nl, keys, nkeys, np.array(tid), np.array(pa), np.array(pb))
    dr = np.zeros((len(rows), nkeys), np.int64)
    for i, k in enumerate(owner):
        dr[k] += cnt[i]
    return dr, run


@pytest.mark.parametrize("fn,args", GOLDEN_CASES)
def test_cli_vcf_on_golden_cases(fn, args, tmp_path):
    vcf = str(tmp_path / "out.vcf")
    plain = run_cli(args)
    with_vcf = run_cli(["--vcf", vcf] + args)
    assert filter_cmd_lines(with_vcf) == filter_cmd_lines(plain) == filter_cmd_lines(open(os.path.join(CWD, fn)).read())
    by_lib = "-a" in args
    kw = dict(cn_lib=int(by_lib), print_af=int("-h" in args), chr_tid=22 if "-o" in args else -1)
    dr, run = chr21_expected_dr(plain, kw, by_lib)
    samples = run.lib_names if by_lib else [os.path.basename(b) for b in run.bam_names]
    text = open(vcf).read()
    assert "##command=" + " ".join([EXE, "--vcf", vcf] + args + ["inv_del_bam_config"]) in text
    check_vcf_against_table(plain, text, samples, dr, by_lib, af_col="-h" in args)
    assert any("0/" in l or "1/1" in l for l in text.split("\n") if not l.startswith("#"))


def test_cli_vcf_with_dash_t_has_no_reference_counts(tmp_path):
    vcf = str(tmp_path / "t.vcf")
    table = run_cli(["--vcf", vcf, "-t", "-y", "-1"])
    assert filter_cmd_lines(table) == filter_cmd_lines(run_cli(["-t", "-y", "-1"]))
    run = load_chr21(make_opts(transchr_rearrange=1)).run()
    check_vcf_against_table(table, open(vcf).read(), [os.path.basename(b) for b in run.bam_names], None, False, dr_unknown=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. sharded runs and -o with CTX calls
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_vcf_sharded_equals_one_gpu_and_dash_o_ctx(tmp_path):
    from fuzzgen import make_case
    from test_gpu_cli_fuzz import write_case
    rng = np.random.default_rng(3)
    cfg, streams, targets = make_case(913, n_pairs=1400)
    write_case(str(tmp_path), streams, targets, rng)
    (tmp_path / "cfg").write_text(cfg)
    d = str(tmp_path)
    args = ["-y", "-1", "-r", "1"]
    one = run_cli(["--vcf", "one.vcf"] + args, cwd=d, cfg="cfg")
    assert filter_cmd_lines(one) == filter_cmd_lines(run_cli(args, cwd=d, cfg="cfg"))
    ref = open(os.path.join(d, "one.vcf")).read()
    assert "<CTX>" in ref
    recs = [l.split("\t") for l in ref.split("\n") if l and not l.startswith("#")]
    assert any(int(f.split(":")[3]) > 0 for r in recs for f in r[9:])
    for gpus in ("0,0", "0,0,0"):
        out = run_cli(["--vcf", "one.vcf"] + args, cwd=d, cfg="cfg", env=dict(BDX_GPUS=gpus))
        assert filter_cmd_lines(out) == filter_cmd_lines(one)
        assert open(os.path.join(d, "one.vcf")).read() == ref, gpus
    # -o: the run reads one chromosome.  Its calls' junctions lie there and have their counts; a junction elsewhere would be unknown ('.'),
    # but a CTX call needs both mates of its pairs, so an -o run does not make one.
    for chrom in targets:
        o = run_cli(["--vcf", "o.vcf", "-o", chrom] + args, cwd=d, cfg="cfg")
        orecs = [l.split("\t") for l in open(os.path.join(d, "o.vcf")).read().split("\n") if l and not l.startswith("#")]
        rows = [l.split("\t") for l in o.split("\n") if l and not l.startswith("#")]
        assert len(orecs) == len(rows)
        for r in orecs:
            assert r[0] == chrom or r[4] == "<CTX>", r
            drs = [f.split(":")[3] for f in r[9:]]
            if r[4] == "<CTX>":
                assert all(x == "." for x in drs) and all(f.startswith("./.:.:.:") for f in r[9:]), r
            else:
                assert all(x != "." for x in drs), r
