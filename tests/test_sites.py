"""CPU tests of --sites: the table parser (host/sites.cpp) and its errors through bin/breakdancer-max -- every one ends the run with
status 1 before the GPU is touched -- and through the stand-alone bdx-sites-check, built here a second time with the address and
undefined-behaviour sanitizers; and, on the CPU oracle alone, that the hand-built stores of test_gpu_sites.py leave no comparison empty."""
import os
import subprocess

import pytest

from helpers import GOLDEN, ROOT, read_bam

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHR21 = os.path.join(GOLDEN, "chr21")
HOST = os.path.join(ROOT, "breakdancer_amd", "host")
MASKS = "DEL=4,INS=8,INV=34,ITX=16,CTX=256"          # Options::sv_flag_mask without -l
MASKS_L = "DEL=16,INS=8,INV=34,ITX=0,CTX=256"        # ... and with -l: no read class prints as ITX

GOOD = "21\t100\t3+0-\t21\t900\t0+3-\tDEL\t800\t99\t3\tx|3\n"
# (label, line, extra options): line 2 of a file whose lines 1 and 3 are good
MALFORMED = [("too-few-fields", "21\t100\t3+0-\t21\t900\t0+3-\n", []),
             ("one-field", "21\n", []),
             ("spaces-are-not-separators", "21 100 3+0- 21 900 0+3- DEL 800\n", []),
             ("position-not-an-integer", "21\t1e3\t3+0-\t21\t900\t0+3-\tDEL\t800\n", []),
             ("position-empty", "21\t\t3+0-\t21\t900\t0+3-\tDEL\t800\n", []),
             ("position-zero", "21\t0\t3+0-\t21\t900\t0+3-\tDEL\t800\n", []),
             ("position-negative", "21\t100\t3+0-\t21\t-900\t0+3-\tDEL\t800\n", []),
             ("position-beyond-int32", "21\t100\t3+0-\t21\t2147483648\t0+3-\tDEL\t800\n", []),
             ("unknown-type", "21\t100\t3+0-\t21\t900\t0+3-\tDUP\t800\n", []),
             ("empty-type", "21\t100\t3+0-\t21\t900\t0+3-\t\t800\n", []),
             ("itx-with-dash-l", "21\t100\t3+0-\t21\t900\t0+3-\tITX\t800\n", ["-l"]),
             ("ctx-on-one-chromosome", "21\t100\t3+0-\t21\t900\t0+3-\tCTX\t-1\n", []),
             ("del-on-two-chromosomes", "21\t100\t3+0-\t20\t900\t0+3-\tDEL\t800\n", []),
             ("malformed-line-on-an-unknown-sequence", "chrUn_x\t100\t3+0-\tchrUn_x\tnine\t0+3-\tDEL\t800\n", [])]


def run_tool(exe, args, cwd):
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("label,line,extra", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_lines_exit_1_with_file_and_line(tmp_path, label, line, extra):
    f = tmp_path / "sites.txt"
    f.write_text(GOOD + line + GOOD)
    out = tmp_path / "o.vcf"
    p = run_tool(EXE, ["--sites", str(f), "--sites-vcf", str(out)] + extra + ["inv_del_bam_config"], CHR21)
    assert p.returncode == 1, (p.stdout.decode()[-300:], p.stderr.decode())
    assert ("%s:2:" % f) in p.stderr.decode(), p.stderr.decode()
    assert not p.stdout.decode().strip()   # (nothing was printed: the file is read before any work is done, and before the GPU is touched)


def test_itx_is_a_type_without_dash_l(tmp_path):
    """the same ITX line that -l refuses gets past the parser without it (the run then fails later, on this machine for want of a GPU, or
    succeeds): stderr does not name the file and line"""
    f = tmp_path / "sites.txt"
    f.write_text(GOOD + "21\t100\t3+0-\t21\t900\t0+3-\tITX\t800\n")
    p = run_tool(EXE, ["--sites", str(f), "--sites-vcf", str(tmp_path / "o.vcf"), "-o", "21", "inv_del_bam_config"], CHR21)
    assert ("%s:2" % f) not in p.stderr.decode(), p.stderr.decode()


def test_sites_needs_sites_vcf_and_the_reverse(tmp_path):
    f = tmp_path / "sites.txt"
    f.write_text(GOOD)
    for args in (["--sites", str(f)], ["--sites-vcf", str(tmp_path / "o.vcf")], ["--sites-window", "300"],
                 ["--sites", str(f), "--sites-vcf", str(tmp_path / "o.vcf"), "--sites-window", "x"],
                 ["--sites", str(f), "--sites-vcf", str(tmp_path / "o.vcf"), "--sites-window", "-1"],
                 ["--sites", str(f), "--sites-vcf", str(tmp_path / "o.vcf"), "--sites-window", "1073741825"]):
        p = run_tool(EXE, args + ["inv_del_bam_config"], CHR21)
        assert p.returncode == 1 and "--sites" in p.stderr.decode() and not p.stdout.decode().strip(), (args, p.stderr.decode())
    assert not os.path.exists(str(tmp_path / "o.vcf"))     # (a usage error: nothing was opened)


def test_unreadable_sites_file_exits_1_naming_the_file(tmp_path):
    missing = str(tmp_path / "no_such.txt")
    p = run_tool(EXE, ["--sites", missing, "--sites-vcf", str(tmp_path / "o.vcf"), "inv_del_bam_config"], CHR21)
    assert p.returncode == 1 and missing in p.stderr.decode(), p.stderr.decode()
    assert not p.stdout.decode().strip()
    p = run_tool(EXE, ["--sites", str(tmp_path), "--sites-vcf", str(tmp_path / "o.vcf"), "inv_del_bam_config"], CHR21)   # a directory
    assert p.returncode == 1 and str(tmp_path) in p.stderr.decode() and not p.stdout.decode().strip(), p.stderr.decode()


def test_unwritable_sites_vcf_exits_1(tmp_path):
    f = tmp_path / "sites.txt"
    f.write_text(GOOD)
    p = run_tool(EXE, ["--sites", str(f), "--sites-vcf", str(tmp_path / "no_such_dir" / "o.vcf"), "inv_del_bam_config"], CHR21)
    assert p.returncode == 1 and "o.vcf" in p.stderr.decode() and not p.stdout.decode().strip(), p.stderr.decode()


def test_usage_text_names_the_three_options():
    p = run_tool(EXE, [], CHR21)
    err = p.stderr.decode()
    assert p.returncode == 1 and "--sites FILE" in err and "--sites-vcf FILE" in err and "--sites-window INT" in err
    assert "--vcf FILE" in err and "--exclude FILE" in err


# ---------------------------------------------------------------------------------------------------------------------------------
# the parser on its own: bdx-sites-check, plain and under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """(bin/bdx-sites-check, the same two sources built with -fsanitize=address,undefined)"""
    plain = os.path.join(ROOT, "bin", "bdx-sites-check")
    if not os.path.exists(plain):
        subprocess.check_call(["make", "-C", ROOT, "bin/bdx-sites-check"], stdout=subprocess.DEVNULL)
    san = str(tmp_path_factory.mktemp("san") / "bdx-sites-check-san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", san, os.path.join(HOST, "sites_check_main.cpp"), os.path.join(HOST, "sites.cpp")])
    return plain, san


def check(exe, path, masks, names):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, str(path), masks] + names, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def test_parser_errors_under_the_sanitizers(tmp_path, checkers):
    names = ["20", "21", "22"]
    for exe in checkers:
        for label, line, extra in MALFORMED:
            f = tmp_path / ("%s.txt" % label)
            f.write_text(GOOD + line + GOOD)
            p = check(exe, f, MASKS_L if extra else MASKS, names)
            err = p.stderr.decode()
            assert p.returncode == 1 and ("%s:2:" % f) in err and "Sanitizer" not in err and "runtime error" not in err, (exe, label, err)
        p = check(exe, tmp_path / "no_such.txt", MASKS, names)
        assert p.returncode == 1 and "no_such.txt" in p.stderr.decode() and "Sanitizer" not in p.stderr.decode()
        odd = tmp_path / "odd.txt"     # no newline at the end, a lone carriage return, a NUL byte, a very long line, tabs only
        odd.write_bytes(b"\r\n\t\t\t\n" + GOOD.encode() + b"21\t5\t.\t21\t6\t.\tINV\t\x00\t\n" + b"#" + b"x" * 100000 + b"\n" + b"21\t7\t.\t21\t8\t.\tINS\t" + b"9" * 400)
        p = check(exe, odd, MASKS, names)
        assert p.returncode == 0 and "Sanitizer" not in p.stderr.decode() and "runtime error" not in p.stderr.decode(), p.stderr.decode()
        assert p.stdout.decode().splitlines()[-1] == "unknown 0" and len(p.stdout.decode().splitlines()) == 4


def test_parser_keeps_normalises_and_counts(tmp_path, checkers):
    """comments and blank lines are skipped, lines on unknown sequences ignored and counted, the ends swapped into order (the line as given is
    kept beside them), a numeric Size kept and anything else there not, further fields ignored, \\r\\n taken; the masks are the ones handed in"""
    names = ["20", "21", "22"]
    f = tmp_path / "sites.txt"
    f.write_text("#Software: x\n#Chr1\tPos1\n\n" +
                 "21\t900\t3+0-\t21\t100\t0+3-\tDEL\t800\t99\n" +           # ends out of order
                 "22\t5\t.\t20\t7\t.\tCTX\t-1\r\n" +                         # ... across chromosomes; \r\n
                 "chrUn\t5\t.\t21\t7\t.\tCTX\t-1\n" +                        # unknown: ignored, counted
                 "21\t5\t.\t21\t5\t.\tINV\tn/a\n" +                          # Size is not a number: none kept
                 "21\t+6\t.\t21\t7\t.\tITX\n" +                              # seven fields
                 "21\t6\t.\tchrUn2\t7\t.\tCTX\t3\n")
    for exe in checkers:
        p = check(exe, f, MASKS, names)
        assert p.returncode == 0, p.stderr.decode()
        assert p.stdout.decode().splitlines() == ["1 1 900 1 100 DEL 800 1 100 1 900 4", "2 2 5 0 7 CTX -1 0 7 2 5 256", "3 1 5 1 5 INV . 1 5 1 5 34",
                                                  "4 1 6 1 7 ITX . 1 6 1 7 16", "unknown 2"]
    only = tmp_path / "only.txt"
    only.write_text("# nothing but comments\n\nchrUn\t5\t.\tchrUn\t7\t.\tDEL\t2\n#\n")
    for exe in checkers:
        p = check(exe, only, MASKS, names)
        assert p.returncode == 0 and p.stdout.decode().splitlines() == ["unknown 1"], (p.stdout.decode(), p.stderr.decode())


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU test's stores, on the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["one/big", "three/big", "three/big/l"])
def test_the_big_stores_leave_no_comparison_empty(label):
    import test_gpu_sites as T
    run, st, soa = T.store_case(label)
    share, flags, rr_counts = T.coverage(run, st, soa)
    assert 4500 < len(soa["tid"]) < 6500
    assert share > 0.3 and rr_counts, (share, rr_counts)
    assert flags >= {T.FF, T.LARGE, T.SMALL, T.RF, T.CTX}, flags
    assert T.RR not in flags      # (the pass-2 remap leaves no passing record with ARP_RR: test_gpu_sites.py's docstring)
