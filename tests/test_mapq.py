"""CPU tests of --mapq: its usage errors through bin/breakdancer-max -- every one ends the run with status 1 before the GPU is touched -- and
the INFO keys of the VCF writer (host/vcf.cpp, mapq_info) through the stand-alone bdx-mapq-check, built here a second time with the address
and undefined-behaviour sanitizers.

The formatting pinned here: eight keys in the order SQN, SQMIN, SQQ1, SQMED, SQMAX, LQA, LQN, LQF, each with one entry for the first printed
end and one for the second.  The two ends arrive in the order of the site the record was counted as and are swapped back when the record
prints them the other way round.  An entry is '.' for an end on a chromosome the run did not read (every key), with n == 0 (SQMIN, SQQ1,
SQMED, SQMAX; SQN prints 0) and with n_all == 0 (LQF); LQF = n_low / n_all with three decimals as printf rounds the double."""
import os
import subprocess

import pytest

from helpers import GOLDEN, ROOT

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHR21 = os.path.join(GOLDEN, "chr21")
HOST = os.path.join(ROOT, "breakdancer_amd", "host")
KEYS = ("SQN", "SQMIN", "SQQ1", "SQMED", "SQMAX", "LQA", "LQN", "LQF")


def run_tool(exe, args, cwd):
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_usage_text_names_the_two_options():
    p = run_tool(EXE, [], CHR21)
    err = p.stderr.decode()
    assert p.returncode == 1 and "--mapq " in err and "--mapq-window INT" in err
    lines = err.split("\n")
    at = lambda opt: [i for i, l in enumerate(lines) if l.strip().startswith(opt + " ")][0]
    assert at("--ci-window") < at("--mapq") < at("--mapq-window")         # (beside those of --ci)


def test_usage_errors_exit_1_before_the_gpu_is_touched(tmp_path):
    out = str(tmp_path / "o.vcf")
    needs = "--mapq needs --vcf FILE or --sites-vcf FILE to write to (and --mapq-window goes with --mapq)."
    takes = "--mapq-window takes an integer from 0 to 2^30, not '%s'."
    cases = [(["--mapq"], needs),                                                      # 1. nothing to write to
             (["--mapq", "--mapq-window", "500"], needs),
             (["--vcf", out, "--mapq-window", "500"], needs),                          # 2. the window without --mapq
             (["--mapq-window", "500"], needs),
             (["--vcf", out, "--ci", "--mapq-window", "500"], needs),                  # (--ci's window is not --mapq's)
             (["--vcf", out, "--mapq", "--mapq-window", "-1"], takes % "-1"),          # 3. below 0
             (["--vcf", out, "--mapq", "--mapq-window", "1073741825"], takes % "1073741825"),   # 4. above 2^30
             (["--vcf", out, "--mapq", "--mapq-window", "x"], takes % "x"),            # (... and no integer at all)
             (["--vcf", out, "--mapq", "--mapq-window", "12x"], takes % "12x"),
             (["--vcf", out, "--mapq", "--mapq-window", ""], takes % "")]
    for args, message in cases:
        p = run_tool(EXE, args + ["inv_del_bam_config"], CHR21)
        err = p.stderr.decode()
        assert p.returncode == 1 and err.strip() == message, (args, err)
        assert not p.stdout.decode().strip(), (args, err)
    assert not os.path.exists(out)     # (a usage error: nothing was opened)


# ---------------------------------------------------------------------------------------------------------------------------------
# the formatting on its own: bdx-mapq-check, plain and under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
def end(held=1, n=0, n_all=0, n_low=0, qmin=0, q1=0, median=0, qmax=0):
    return (held, n, n_all, n_low, qmin, q1, median, qmax)


def restated(e1, e2, swapped):
    """the writer's rules, written out: what the INFO fragment of a record has to be"""
    first, second = (e2, e1) if swapped else (e1, e2)

    def entry(key, e):
        held, n, n_all, n_low, qmin, q1, median, qmax = e
        if not held:
            return "."
        if key == "SQN":
            return str(n)
        if key in ("SQMIN", "SQQ1", "SQMED", "SQMAX"):
            return str(dict(SQMIN=qmin, SQQ1=q1, SQMED=median, SQMAX=qmax)[key]) if n else "."
        if key == "LQA":
            return str(n_all)
        if key == "LQN":
            return str(n_low)
        return "%.3f" % (n_low / n_all) if n_all else "."

    return "".join(";%s=%s,%s" % (k, entry(k, first), entry(k, second)) for k in KEYS)


FULL = end(n=7, n_all=40, n_low=10, qmin=36, q1=37, median=60, qmax=255)
CASES = [(FULL, end(n=2, n_all=3, n_low=1, qmin=40, q1=40, median=40, qmax=41), 0),
         (FULL, end(n=2, n_all=3, n_low=1, qmin=40, q1=40, median=40, qmax=41), 1),      # swapped: the second site end prints first
         (FULL, end(n=0, n_all=3, n_low=2), 0),                                          # n == 0: SQN=0, the four qualities '.'; 2/3
         (end(n=0, n_all=3, n_low=1), FULL, 1),                                          # 1/3
         (end(n=0, n_all=0, n_low=0), end(n=0, n_all=0, n_low=0), 0),                    # 0/0: LQF '.', LQA and LQN 0
         (FULL, end(held=0), 0),                                                         # one end not held: '.' in every key ...
         (FULL, end(held=0), 1),                                                         # ... in the first place when swapped
         (end(held=0, n=5, n_all=9, n_low=9, qmin=1, q1=2, median=3, qmax=4), FULL, 0),  # (whatever the summary of such an end holds)
         (end(n=1, n_all=16, n_low=1, qmin=0, q1=0, median=0, qmax=0), end(n=3, n_all=16, n_low=3, qmin=255, q1=255, median=255, qmax=255), 0),  # quality 0 prints 0; 0.0625, 0.1875: ties
         (end(n=2**32 - 1, n_all=2**32 - 1, n_low=2**32 - 1, qmin=1, q1=2, median=3, qmax=4), end(n=1, n_all=2**32 - 1, n_low=1, qmin=9, q1=9, median=9, qmax=9), 0),
         (end(n=1, n_all=8, n_low=8, qmin=5, q1=5, median=5, qmax=5), end(n=1, n_all=2000, n_low=1, qmin=5, q1=5, median=5, qmax=5), 0)]   # 1.000, 0.001 (0.0005 rounds as the double does)


def test_the_restatement_on_cases_worked_out_by_hand():
    assert restated(*CASES[0]) == ";SQN=7,2;SQMIN=36,40;SQQ1=37,40;SQMED=60,40;SQMAX=255,41;LQA=40,3;LQN=10,1;LQF=0.250,0.333"
    assert restated(*CASES[1]) == ";SQN=2,7;SQMIN=40,36;SQQ1=40,37;SQMED=40,60;SQMAX=41,255;LQA=3,40;LQN=1,10;LQF=0.333,0.250"
    assert restated(*CASES[2]) == ";SQN=7,0;SQMIN=36,.;SQQ1=37,.;SQMED=60,.;SQMAX=255,.;LQA=40,3;LQN=10,2;LQF=0.250,0.667"
    assert restated(*CASES[4]) == ";SQN=0,0;SQMIN=.,.;SQQ1=.,.;SQMED=.,.;SQMAX=.,.;LQA=0,0;LQN=0,0;LQF=.,."
    assert restated(*CASES[6]) == ";SQN=.,7;SQMIN=.,36;SQQ1=.,37;SQMED=.,60;SQMAX=.,255;LQA=.,40;LQN=.,10;LQF=.,0.250"
    assert "%.3f" % (1 / 16) == "0.062" and "%.3f" % (3 / 16) == "0.188"


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """(bin/bdx-mapq-check, the same two sources built with -fsanitize=address,undefined)"""
    plain = os.path.join(ROOT, "bin", "bdx-mapq-check")
    if not os.path.exists(plain):
        subprocess.check_call(["make", "-C", ROOT, "bin/bdx-mapq-check"], stdout=subprocess.DEVNULL)
    san = str(tmp_path_factory.mktemp("san") / "bdx-mapq-check-san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", san, os.path.join(HOST, "mapq_check_main.cpp"), os.path.join(HOST, "vcf.cpp")])
    return plain, san


def test_mapq_info_on_a_table_of_cases(checkers):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    text = "".join(" ".join(str(v) for v in e1 + e2 + (sw,)) + "\n" for e1, e2, sw in CASES)
    for exe in checkers:
        p = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        err = p.stderr.decode()
        assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (exe, err)
        got = p.stdout.decode().splitlines()
        assert len(got) == len(CASES)
        for c, g in zip(CASES, got):
            assert g == restated(*c), (exe, c, g)
        for bad in ("1 2 3\n", " ".join(["1"] * 16) + " x\n", " ".join(["1"] * 18) + "\n", " ".join(["1"] * 16) + " -1\n"):
            p = subprocess.run([exe], input=bad.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            assert p.returncode == 2 and "Sanitizer" not in p.stderr.decode(), (exe, bad)
