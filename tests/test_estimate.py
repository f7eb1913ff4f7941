"""CPU tests of --estimate: bdx_estimate_insert_size against a plain-Python restatement with the same sums in the same order
(estimate_cases.py), the host half of the CLI through the stand-alone bdx-estimate-check (the run's libraries, the rewritten
configuration), the usage errors through bin/breakdancer-max -- each ends the run with status 1 before the GPU is touched -- and the
figures of the chr21 fixture.

Counts and `valid` must be exact.  Doubles get a relative tolerance of 1e-10: every sum has at most 32768 terms, each rounded once to
2^-53 relative, which bounds the accumulated error by 32768 * 2^-53 = 3.6e-12; 1e-10 leaves margin for the division and the square root.
This is derived, not measured."""
import os
import subprocess

import numpy as np
import pytest

import estimate_cases as ec
from helpers import GOLDEN, ROOT, read_bam

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHECK = os.path.join(ROOT, "bin", "bdx-estimate-check")
CHR21 = os.path.join(GOLDEN, "chr21")
RTOL = 1e-10
DOUBLES = ("mean_all", "sd_all", "mean", "sd", "sd_minus", "sd_plus")
COUNTS = ("n", "n_kept", "n_minus", "n_plus", "valid")


def run_tool(exe, args, cwd=None, env=None):
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)


def assert_estimate(got, want, label):
    for k in COUNTS:
        assert int(got[k]) == int(want[k]), (label, k, got[k], want[k])
    for k in DOUBLES:
        assert abs(got[k] - want[k]) <= RTOL * abs(want[k]), (label, k, got[k], want[k])


HAND = ec.hand_cases()
GENERATED = ec.generated_cases()


@pytest.mark.parametrize("label", sorted(HAND))
def test_estimate_equals_restatement_on_hand_cases(label):
    from breakdancer_amd.api import estimate_insert_size
    want = ec.restate(HAND[label])
    assert_estimate(estimate_insert_size(HAND[label]), want, label)


def test_hand_cases_are_what_their_names_say():
    r = {k: ec.restate(h) for k, h in HAND.items()}
    assert r["empty"]["n"] == 0 and not r["empty"]["valid"] and r["empty"]["mean"] == 0.0
    assert r["one"]["n_kept"] == 1 and r["one"]["sd_all"] == 0.0 and not r["one"]["valid"]
    e = r["all_equal"]
    assert e["sd_all"] == 0.0 and e["n_kept"] == e["n"] == 500 and e["n_plus"] == 0 and not e["valid"]
    assert r["kept_99"]["n_kept"] == 99 and not r["kept_99"]["valid"]
    assert r["kept_100"]["n_kept"] == 100 and r["kept_100"]["valid"]
    assert r["n_plus_1"]["n_plus"] == 1 and r["n_plus_1"]["sd_plus"] == 0.0 and not r["n_plus_1"]["valid"]
    o = r["outlier_trimmed"]
    assert o["n_kept"] == o["n"] - 1 and o["mean_all"] - o["mean"] > 10 and o["valid"]
    b = r["bin_edges"]
    assert (b["n_minus"], b["n_plus"]) == (120, 130) and b["valid"]
    assert r["bimodal"]["valid"] and r["bimodal"]["n_kept"] == 4500


def test_estimate_equals_restatement_on_generated_libraries():
    from breakdancer_amd.api import estimate_insert_size
    assert len(GENERATED) >= 20
    some_trimmed = False
    for label, h in GENERATED.items():
        want = ec.restate(h)
        assert ec.preconditions_hold(want), label
        some_trimmed |= want["n_kept"] < want["n"]
        assert_estimate(estimate_insert_size(h), want, label)
    assert some_trimmed


def test_estimate_refuses_null_pointers():
    import ctypes as C
    from breakdancer_amd import _lib as L
    lib = L.load()
    h = np.zeros(ec.BINS, dtype=np.uint64)
    out = L.bdx_insert_estimate()
    assert lib.bdx_estimate_insert_size(None, C.byref(out)) == 1
    assert lib.bdx_estimate_insert_size(h.ctypes.data_as(C.c_void_p), None) == 1
    assert L.ISIZE_BINS == ec.BINS
    assert "#define BDX_ISIZE_BINS %d" % ec.BINS in open(os.path.join(ROOT, "include", "bdx.h")).read()


# ---------------------------------------------------------------------------------------------------------------------------------
# the host half of the CLI: bdx-estimate-check

def parse_config(text, c=3):
    """the configuration parser's view of the insert-size fields, per library name: (mean, std, upper, lower) as float32 -- the keys
    the tests write are the plain ones (mean: std: upper: lower: lib:)"""
    libs = {}
    for line in text.split("\n"):
        if not line:
            break
        d = {}
        for f in line.split("\t"):
            if ":" in f:
                k, v = f.split(":", 1)
                d[k] = v
        mean, std = np.float32(d.get("mean", 0)), np.float32(d.get("std", 0))
        upper, lower = np.float32(d.get("upper", 0)), np.float32(d.get("lower", 0))
        if "mean" in d and "std" in d and ("upper" not in d or "lower" not in d):
            upper = np.float32(mean + std * np.float32(c))
            lower = max(np.float32(mean - std * np.float32(c)), np.float32(0))
        libs[d["lib"]] = (mean, std, upper, lower)
    return libs


def write_hist(path, hists, over=()):
    with open(path, "w") as f:
        for lib, h in enumerate(hists):
            for x in np.nonzero(h)[0]:
                f.write("%d %d %d\n" % (lib, x, h[x]))
        for lib, x, c in over:
            f.write("%d %d %d\n" % (lib, x, c))


def check_tool(tmp_path, hists, config, c=None, over=()):
    hp, cp, op = str(tmp_path / "hist.txt"), str(tmp_path / "in.cfg"), str(tmp_path / "out.cfg")
    write_hist(hp, hists, over)
    open(cp, "w").write(config)
    p = run_tool(CHECK, [hp, cp] + (["-c", str(c)] if c is not None else []) + ["--out", op])
    rows = [l.split("\t") for l in p.stdout.decode().splitlines()]
    out = dict(rc=p.returncode, err=p.stderr.decode(), est={}, lib={}, warnings=[r[1] for r in rows if r[0] == "warning"],
               window=[int(r[1]) for r in rows if r[0] == "window"], config=open(op).read() if os.path.exists(op) else None)
    for r in rows:
        if r[0] == "estimate":
            out["est"][r[2]] = dict(n=int(r[3]), n_over=int(r[4]), n_kept=int(r[5]), n_minus=int(r[6]), n_plus=int(r[7]), valid=int(r[8]),
                                    **{k: float(v) for k, v in zip(DOUBLES, r[9:15])})
        if r[0] == "library":
            out["lib"][r[2]] = tuple(np.float32(v) for v in r[3:7])
    return out


CONFIG = ("readgroup:rg1\tplatform:illumina\tmap:a.bam\treadlen:90.00\tlib:libA\tnum:10001\tlower:277.03\tupper:525.50\tmean:467.59\tstd:31.91\texe:samtools view\n"
          "readgroup:rg2\tplatform:illumina\tmap:a.bam\treadlen:90.00\tlib:libA\tnum:10001\tlower:277.03\tupper:525.50\tmean:467.59\tstd:31.91\texe:samtools view\n"
          "readgroup:rg3\tmap:b.bam\treadlen:100.00\tlib:libB\tnum:77\tmean:300.00\tstd:20.00\n"
          "readgroup:rg4\tmap:c.bam\treadlen:100.00\tlib:libC\n")


def three_libraries():
    hs = [GENERATED[k] for k in sorted(GENERATED)[:2]]
    return [hs[0], ec.hist_of([300] * 10 + [310] * 5), hs[1]]      # libB: 15 observations, not valid


@pytest.mark.parametrize("c", [None, 2, 5])
def test_rewritten_configuration_parses_to_the_runs_libraries(tmp_path, c):
    hists = three_libraries()
    r = check_tool(tmp_path, hists, CONFIG, c=c, over=[(0, ec.BINS, 3), (0, 2**31 - 1, 4)])
    cc = 3 if c is None else c
    assert r["rc"] == 0, r["err"]
    assert r["est"]["libA"]["n_over"] == 7 and r["est"]["libC"]["n_over"] == 0
    for name, h in zip(("libA", "libB", "libC"), hists):
        want = ec.restate(h)
        assert_estimate(r["est"][name], want, name)
    # the run's libraries: the restatement's values through %.2f and float32 -- -c is honoured also where the line had its own cutoffs (libA)
    for name, h in (("libA", hists[0]), ("libC", hists[2])):
        want = ec.restate(h)
        assert want["valid"] and ec.preconditions_hold(want, cc)
        vals, _, _ = ec.run_libraries(want, cc)
        assert r["lib"][name] == (vals["mean"], vals["std"], vals["upper"], vals["lower"]), name
    assert r["lib"]["libB"] == (np.float32(300), np.float32(20), np.float32(300 + 20 * cc), np.float32(300 - 20 * cc))
    assert len(r["warnings"]) == 1 and "libB" in r["warnings"][0] and "n_kept=15" in r["warnings"][0]
    # parsed again, the rewritten configuration yields exactly the run's libraries
    again = parse_config(r["config"], cc)
    assert again == r["lib"]
    t = min(int(np.float32(m) - np.float32(rl) * np.float32(2)) for m, rl in ((r["lib"]["libA"][0], 90), (r["lib"]["libB"][0], 100), (r["lib"]["libC"][0], 100)))
    assert r["window"] == [max(50, t)]
    lines_in, lines_out = CONFIG.split("\n"), r["config"].split("\n")
    assert len(lines_in) == len(lines_out)
    assert lines_out[2] == lines_in[2]                                   # a library that is not valid: its line is left unchanged
    a = lines_out[0].split("\t")
    _, text, _ = ec.run_libraries(ec.restate(hists[0]), cc)
    assert a == ["readgroup:rg1", "platform:illumina", "map:a.bam", "readlen:90.00", "lib:libA", "num:%d" % ec.restate(hists[0])["n_kept"],
                 "exe:samtools view", "lower:" + text["lower"], "upper:" + text["upper"], "mean:" + text["mean"], "std:" + text["std"]]
    assert lines_out[1].split("\t")[1:] == a[1:] and lines_out[1].startswith("readgroup:rg2\t")
    assert lines_out[3].startswith("readgroup:rg4\tmap:c.bam\treadlen:100.00\tlib:libC\tlower:")


def test_library_without_estimate_and_without_mean_or_std_ends_the_run(tmp_path):
    hists = three_libraries()
    hists[2] = ec.hist_of([500] * 40)
    r = check_tool(tmp_path, hists, CONFIG)
    assert r["rc"] == 1 and "libC" in r["err"] and "neither mean nor std" in r["err"] and r["config"] is None


# ---------------------------------------------------------------------------------------------------------------------------------
# usage errors through the CLI: status 1, the message, nothing on stdout, before the GPU is touched

def test_usage_text_names_the_two_options():
    p = run_tool(EXE, [], CHR21)
    err = p.stderr.decode()
    assert p.returncode == 1 and "--estimate " in err and "--estimate-config FILE" in err


def test_usage_errors_exit_1_before_the_gpu_is_touched(tmp_path):
    out, cache = str(tmp_path / "o.cfg"), str(tmp_path / "cache")
    with_cache = "--estimate does not go with -C or -R: the cache's pass-1 statistics belong to the cutoffs of the run that wrote it."
    cases = [(["--estimate-config", out], ["inv_del_bam_config"], "--estimate-config FILE goes with --estimate."),
             (["--estimate", "-C", cache], ["inv_del_bam_config"], with_cache),
             (["-C", cache, "--estimate", "--estimate-config", out], ["inv_del_bam_config"], with_cache),
             (["--estimate", "-R", cache], [], with_cache),
             (["-R", cache, "--estimate"], [], with_cache)]
    for args, cfg, message in cases:
        p = run_tool(EXE, args + cfg, CHR21, env=dict(HIP_VISIBLE_DEVICES="-1"))
        err = p.stderr.decode()
        assert p.returncode == 1 and err.strip() == message, (args, err)
        assert not p.stdout.decode().strip(), (args, err)
    assert not os.path.exists(out) and not os.path.exists(cache)


def test_unwritable_estimate_config_fails_before_the_gpu_is_touched(tmp_path):
    p = run_tool(EXE, ["--estimate", "--estimate-config", str(tmp_path / "no" / "such" / "dir" / "o.cfg"), "inv_del_bam_config"], CHR21,
                 env=dict(HIP_VISIBLE_DEVICES="-1"))
    assert p.returncode == 1 and "--estimate-config" in p.stderr.decode() and not p.stdout.decode().strip()


# ---------------------------------------------------------------------------------------------------------------------------------
# the chr21 fixture: the figures are recomputed here; the table of the issue is only a sanity anchor

def chr21_histograms(min_q=35):
    cfg = open(os.path.join(CHR21, "inv_del_bam_config")).read()
    rg_lib, bam_lib = {}, {}
    for line in cfg.split("\n"):
        if line:
            d = dict(f.split(":", 1) for f in line.split("\t") if ":" in f)
            rg_lib[d["readgroup"]] = d["lib"]
            bam_lib[d["map"]] = d["lib"]
    names = sorted(set(rg_lib.values()))
    fallback = bam_lib[sorted(bam_lib)[0]]
    hists = {n: np.zeros(ec.BINS, dtype=np.uint64) for n in names}
    over = {n: 0 for n in names}
    for bam in sorted(bam_lib):
        _, r = read_bam(os.path.join(CHR21, bam))
        lib = np.array([names.index(rg_lib.get(g, fallback)) for g in r["rg"]], dtype=np.uint8)
        soa = dict(flag=r["flag"], isize=r["isize"], tid=r["tid"], mtid=r["mtid"], mapq=r["bdqual"], lib=lib)
        h, o = ec.observations(soa, len(names), [min_q] * len(names))
        for i, n in enumerate(names):
            hists[n] += h[i]
            over[n] += int(o[i])
    return cfg, names, hists, over


def test_chr21_reference_point(tmp_path):
    cfg, names, hists, over = chr21_histograms()
    assert names == ["H_IJ-NA19238-NA19238-extlibs", "H_IJ-NA19240-NA19240-extlibs"] and all(v == 0 for v in over.values())
    r = check_tool(tmp_path, [hists[n] for n in names], cfg)
    assert r["rc"] == 0 and not r["warnings"], r["err"]
    anchor = {names[0]: (1279, "473.46", "23.61", "375.25", "508.87"), names[1]: (1160, "466.86", "22.53", "371.88", "501.50")}
    for n in names:
        want = ec.restate(hists[n])
        assert_estimate(r["est"][n], want, n)
        vals, text, _ = ec.run_libraries(want, 3)
        assert r["lib"][n] == (vals["mean"], vals["std"], vals["upper"], vals["lower"])
        assert (want["n"], text["mean"], text["std"], text["lower"], text["upper"]) == anchor[n] and want["n_kept"] == want["n"]
    assert parse_config(r["config"]) == r["lib"]
