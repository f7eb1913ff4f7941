"""CPU tests of --depth: its usage errors through bin/breakdancer-max -- every one ends the run with status 1 before the GPU is touched -- and
the arithmetic of the VCF writer (host/vcf.cpp, depth_spans and depth_ratio) through the stand-alone bdx-depth-check, built here a second
time with the address and undefined-behaviour sanitizers.

The arithmetic pinned here: a record printed at pos1 / pos2 (1-based) with lo = min, hi = max and flank F is counted over the read starts
P with lo <= P < hi (inside), lo - F <= P < lo and hi <= P < hi + F (flanks), every bound clamped to [1, contig length + 1] first;
RDR = (RCI / len_in) / (RCF / len_flank) with the clamped lengths, three decimals as printf rounds the double (an exact binary tie goes to
the even digit), '.' when RCF == 0 or a length is 0."""
import os
import subprocess

import pytest

from helpers import GOLDEN, ROOT

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHR21 = os.path.join(GOLDEN, "chr21")
HOST = os.path.join(ROOT, "breakdancer_amd", "host")


def run_tool(exe, args, cwd):
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_usage_text_names_the_two_options():
    p = run_tool(EXE, [], CHR21)
    err = p.stderr.decode()
    assert p.returncode == 1 and "--depth " in err and "--depth-flank INT" in err and "[1000]" in err


def test_usage_errors_exit_1_before_the_gpu_is_touched(tmp_path):
    out = str(tmp_path / "o.vcf")
    cases = [(["--depth"], "--depth"),                                               # nothing to write to
             (["--depth", "--depth-flank", "500"], "--depth"),
             (["--vcf", out, "--depth-flank", "500"], "--depth"),                   # the flank without --depth
             (["--depth-flank", "500"], "--depth"),
             (["--vcf", out, "--depth", "--depth-flank", "0"], "--depth-flank"),    # outside 1 .. 2^30
             (["--vcf", out, "--depth", "--depth-flank", "-5"], "--depth-flank"),
             (["--vcf", out, "--depth", "--depth-flank", "1073741825"], "--depth-flank"),
             (["--vcf", out, "--depth", "--depth-flank", "x"], "--depth-flank"),
             (["--vcf", out, "--depth", "--depth-flank", "12x"], "--depth-flank")]
    for args, named in cases:
        p = run_tool(EXE, args + ["inv_del_bam_config"], CHR21)
        err = p.stderr.decode()
        assert p.returncode == 1 and named in err and "Unrecognized" not in err and "unrecognized" not in err, (args, err)
        assert "bdx_create" not in err and not p.stdout.decode().strip(), (args, err)
    assert not os.path.exists(out)     # (a usage error: nothing was opened)


# ---------------------------------------------------------------------------------------------------------------------------------
# the arithmetic on its own: bdx-depth-check, plain and under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
# (RCI, RCF, pos1, pos2, flank, contig length) -> (len_in, len_flank, RDR), worked out by hand
CASES = [((50, 100, 1001, 2001, 1000, 100000), (1000, 2000, "1.000")),       # plain: 0.05 per base inside, 0.05 beside
         ((10, 200, 1001, 2001, 1000, 100000), (1000, 2000, "0.100")),       # a deletion: 0.01 against 0.1
         ((300, 100, 1001, 2001, 1000, 100000), (1000, 2000, "6.000")),      # a duplication
         ((10, 200, 2001, 1001, 1000, 100000), (1000, 2000, "0.100")),       # the ends in reverse order
         ((50, 0, 1001, 2001, 1000, 100000), (1000, 2000, ".")),             # RCF == 0
         ((0, 0, 1001, 2001, 1000, 100000), (1000, 2000, ".")),
         ((5, 7, 5000, 5000, 1000, 100000), (0, 2000, ".")),                 # len_in == 0
         ((5, 7, 200001, 200500, 1000, 100000), (0, 0, ".")),                # both ends behind the contig: every length 0
         ((100, 1010, 11, 111, 1000, 100000), (100, 1010, "1.000")),         # left flank clamped at 1: starts 1 .. 10
         ((100, 1000, 1, 101, 1000, 100000), (100, 1000, "1.000")),          # ... no left flank at all
         ((400, 2202, 1500, 1900, 1000, 2000), (400, 1101, "0.500")),        # right flank clamped at the contig's end: starts 1900 .. 2000
         ((400, 1000, 1000, 2001, 1000, 2000), (1001, 999, "0.399")),        # ... hi behind the last base: no right flank; 400 * 999 / (1001 * 1000) = 0.3992...
         ((1, 3, 1001, 3001, 1000, 100000), (2000, 2000, "0.333")),          # rounding at the third decimal: down ...
         ((2, 3, 1001, 3001, 1000, 100000), (2000, 2000, "0.667")),          # ... up
         ((1, 16, 1001, 3001, 1000, 100000), (2000, 2000, "0.062")),         # 0.0625 and 0.1875 are exact in binary: ties to the even digit
         ((3, 16, 1001, 3001, 1000, 100000), (2000, 2000, "0.188")),
         ((0, 100, 1001, 2001, 1000, 100000), (1000, 2000, "0.000")),        # RCI == 0
         ((7, 1, 1, 2, 1, 2), (1, 1, "7.000")),                              # the smallest record: inside start 1, flank start 2
         ((2**31, 1, 1, 2**31 - 1, 2**30, 2**31 - 1), (2**31 - 2, 1, "1.000"))]   # the largest: 2^31 * 1 / ((2^31 - 2) * 1) = 1.00000000093


def test_the_tie_cases_are_what_python_prints_too():
    """the expectations above that depend on how a double prints, against Python's own correctly rounded formatting"""
    assert "%.3f" % (1 / 16) == "0.062" and "%.3f" % (3 / 16) == "0.188"
    assert "%.3f" % (400 * 999 / (1001 * 1000)) == "0.399"


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """(bin/bdx-depth-check, the same two sources built with -fsanitize=address,undefined)"""
    plain = os.path.join(ROOT, "bin", "bdx-depth-check")
    if not os.path.exists(plain):
        subprocess.check_call(["make", "-C", ROOT, "bin/bdx-depth-check"], stdout=subprocess.DEVNULL)
    san = str(tmp_path_factory.mktemp("san") / "bdx-depth-check-san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", san, os.path.join(HOST, "depth_check_main.cpp"), os.path.join(HOST, "vcf.cpp")])
    return plain, san


def test_depth_arithmetic_on_a_table_of_cases(checkers):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    args = [str(v) for c, _ in CASES for v in c]
    for exe in checkers:
        p = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        err = p.stderr.decode()
        assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (exe, err)
        got = [(int(l.split()[0]), int(l.split()[1]), l.split()[2]) for l in p.stdout.decode().splitlines()]
        for (c, e), g in zip(CASES, got):
            assert g == e, (exe, c, g, e)
        assert len(got) == len(CASES)
        for bad in ([], ["1", "2", "3", "4", "5"], ["1", "2", "3", "4", "5", "x"], ["1", "2", "3", "4", "5", "6", "7"]):
            p = subprocess.run([exe] + bad, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            assert p.returncode == 2 and "Sanitizer" not in p.stderr.decode(), (exe, bad)
