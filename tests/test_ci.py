"""CPU tests of --ci: its usage errors through bin/breakdancer-max -- every one ends the run with status 1 before the GPU is touched -- and
the interval arithmetic of the VCF writer (host/vcf.cpp, ci_offsets) through the stand-alone bdx-ci-check, built here a second time with
the address and undefined-behaviour sanitizers.

The arithmetic pinned here: an end printed at P whose supporting pairs bound the breakpoint below by lo and above by hi gets
a = min(lo, hi, P) - P and b = max(lo, hi, P) - P, so a <= 0 <= b always."""
import os
import subprocess

import pytest

from helpers import GOLDEN, ROOT

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHR21 = os.path.join(GOLDEN, "chr21")
HOST = os.path.join(ROOT, "breakdancer_amd", "host")
IMAX = 2**31 - 1


def run_tool(exe, args, cwd):
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_usage_text_names_the_two_options():
    p = run_tool(EXE, [], CHR21)
    err = p.stderr.decode()
    assert p.returncode == 1 and "--ci " in err and "--ci-window INT" in err


def test_usage_errors_exit_1_before_the_gpu_is_touched(tmp_path):
    out = str(tmp_path / "o.vcf")
    for args in (["--ci"], ["--vcf", out, "--ci-window", "300"], ["--ci-window", "300"],
                 ["--vcf", out, "--ci", "--ci-window", "-1"], ["--vcf", out, "--ci", "--ci-window", "x"],
                 ["--vcf", out, "--ci", "--ci-window", "1073741825"]):
        p = run_tool(EXE, args + ["inv_del_bam_config"], CHR21)
        err = p.stderr.decode()
        assert p.returncode == 1 and "--ci" in err and "bdx_create" not in err and not p.stdout.decode().strip(), (args, err)
    assert not os.path.exists(out)     # (a usage error: nothing was opened)


def test_no_finite_cutoff_asks_for_the_window(tmp_path):
    cfg = tmp_path / "cfg"
    lines = open(os.path.join(CHR21, "inv_del_bam_config")).read().split("\n")
    cfg.write_text("\n".join("\t".join("upper:inf" if f.startswith("upper:") else f for f in l.split("\t")) for l in lines))
    p = run_tool(EXE, ["--vcf", str(tmp_path / "o.vcf"), "--ci", str(cfg)], CHR21)
    err = p.stderr.decode()
    assert p.returncode == 1 and "--ci-window" in err and "bdx_create" not in err and not p.stdout.decode().strip(), err


# ---------------------------------------------------------------------------------------------------------------------------------
# the interval arithmetic on its own: bdx-ci-check, plain and under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
# (lo, hi, P) -> (a, b)
CASES = [((90, 130, 100), (-10, 30)),                   # lo < P < hi
         ((100, 100, 100), (0, 0)),
         ((100, 130, 100), (0, 30)), ((90, 100, 100), (-10, 0)),
         ((110, 130, 100), (0, 30)),                    # P below the interval ...
         ((60, 80, 100), (-40, 0)),                     # ... and above it
         ((130, 90, 100), (-10, 30)),                   # lo > hi: the span of the contradiction, P inside it ...
         ((130, 110, 100), (0, 30)), ((80, 60, 100), (-40, 0)),   # ... and outside, on either side
         ((1, 1, 1), (0, 0)), ((1, IMAX, 1), (0, IMAX - 1)), ((1, IMAX, IMAX), (1 - IMAX, 0)),   # values at 1 and at 2^31 - 1
         ((IMAX, 1, 1000), (1 - 1000, IMAX - 1000)), ((IMAX, IMAX, IMAX), (0, 0)), ((IMAX, IMAX, 1), (0, IMAX - 1)),
         ((1, 1, IMAX), (1 - IMAX, 0))]


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """(bin/bdx-ci-check, the same two sources built with -fsanitize=address,undefined)"""
    plain = os.path.join(ROOT, "bin", "bdx-ci-check")
    if not os.path.exists(plain):
        subprocess.check_call(["make", "-C", ROOT, "bin/bdx-ci-check"], stdout=subprocess.DEVNULL)
    san = str(tmp_path_factory.mktemp("san") / "bdx-ci-check-san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", san, os.path.join(HOST, "ci_check_main.cpp"), os.path.join(HOST, "vcf.cpp")])
    return plain, san


def test_interval_arithmetic_on_a_table_of_cases(checkers):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    args = [str(v) for c, _ in CASES for v in c]
    for exe in checkers:
        p = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        err = p.stderr.decode()
        assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (exe, err)
        got = [tuple(int(x) for x in l.split()) for l in p.stdout.decode().splitlines()]
        assert got == [e for _, e in CASES], exe
        assert all(a <= 0 <= b for a, b in got)
        for bad in ([], ["1", "2"], ["1", "2", "x"], ["1", "2", "3", "4"]):
            p = subprocess.run([exe] + bad, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            assert p.returncode == 2 and "Sanitizer" not in p.stderr.decode(), (exe, bad)
