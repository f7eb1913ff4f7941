"""CPU tests of --clip: the clip word (include/bdx.h bdx_clip_word; csrc/bdx_clip.h, the one function of every reader) on a table of CIGARs
worked out by hand, the words the host reader gives every record of the chr21 BAMs against a plain Python parse, the INFO keys of the VCF
writer (host/vcf.cpp clip_info) and their winner rule through the stand-alone bdx-clip-check -- built here a second time with the address
and undefined-behaviour sanitizers --, and the command line's usage errors.  No GPU: test_gpu_clip.py has the kernel and the routes."""
import os
import subprocess

import numpy as np
import pytest

from clip_cases import TABLE, cigar_of, parse_bam_cigars, synthetic_bam, table_word, word_of, words_of_bam
from helpers import GOLDEN, ROOT

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
HOST = os.path.join(ROOT, "breakdancer_amd", "host")
CHR21 = os.path.join(GOLDEN, "chr21")
BAMS = ("NA19238_chr21_del_inv.bam", "NA19240_chr21_del_inv.bam")
KEYS = ("CLN", "CLPOS", "CLSUP", "CLSIDE")


def run_tool(exe, args, cwd):
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    return subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """(bin/bdx-clip-check, the same sources built with -fsanitize=address,undefined)"""
    plain = os.path.join(ROOT, "bin", "bdx-clip-check")
    if not os.path.exists(plain):
        subprocess.check_call(["make", "-C", ROOT, "bin/bdx-clip-check"], stdout=subprocess.DEVNULL)
    san = str(tmp_path_factory.mktemp("san") / "bdx-clip-check-san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", san, os.path.join(HOST, "clip_check_main.cpp"), os.path.join(HOST, "vcf.cpp"),
                           os.path.join(HOST, "bam_reader.cpp"), "-lz"])
    return plain, san


SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def clean(p, exe):
    err = p.stderr.decode()
    assert "Sanitizer" not in err and "runtime error" not in err, (exe, err)
    return err


# ---------------------------------------------------------------------------------------------------------------------------------
# the clip word
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_restatement_agrees_with_the_table_worked_out_by_hand():
    for row in TABLE:
        assert word_of(cigar_of(row[0]), row[1], row[2]) == table_word(row), row
    texts = [r[0] for r in TABLE]
    for needed in ("", "90M", "5S85M", "85M5S", "3H2S80M5S", "300S90M", "90S", "40M5I45M", "40M10D40M2N8M", "90S4000N"):
        assert needed in texts
    assert [r[5] for r in TABLE if r[0].startswith("5S6553")] == [65534, 65535, 65535]
    assert [r[4] for r in TABLE if r[0].startswith("5S6553")] == [7, 7, 0]                   # the right clip goes when the span is capped
    assert any(r[2] & 0x4 for r in TABLE) and any("=" in r[0] and "X" in r[0] for r in TABLE) and any("P" in r[0] for r in TABLE)


def test_bdx_clip_word_on_the_table():
    import ctypes as C
    from breakdancer_amd import _lib
    from breakdancer_amd.api import clip_word
    for row in TABLE:
        assert clip_word(cigar_of(row[0]), row[1], row[2]) == table_word(row), row
    lib = _lib.load()
    assert lib.bdx_clip_word(None, 0, 90, 0) == 0 and lib.bdx_clip_word(None, 3, 90, 0) == 0    # no CIGAR; a null pointer is no CIGAR either
    # an unmapped record's word is 0 whatever its CIGAR, and no other flag bit matters
    for row in TABLE:
        c = cigar_of(row[0])
        assert clip_word(c, row[1], row[2] | 0x4) == 0
        assert clip_word(c, row[1], (row[2] | 0xFFFB) & ~0x4 if not row[2] & 0x4 else row[2]) == table_word(row)
    # the word is read byte by byte: a CIGAR at an odd address gives the same
    w = np.array([(5 << 4) | 4, (85 << 4) | 0], dtype="<u4").tobytes()
    buf = (C.c_uint8 * 16).from_buffer_copy(b"\0" + w + b"\0" * 7)
    assert lib.bdx_clip_word(C.c_void_p(C.addressof(buf) + 1), 2, 90, 0) == 5 | (85 << 16)


def test_the_checker_prints_the_tables_words(checkers):
    text = "".join("%s %d %d\n" % (r[0] or "*", r[1], r[2]) for r in TABLE)
    for exe in checkers:
        p = subprocess.run([exe, "words"], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=SAN_ENV)
        clean(p, exe)
        assert p.returncode == 0
        got = [tuple(int(v) for v in l.split()) for l in p.stdout.decode().splitlines()]
        assert got == [(r[3], r[4], r[5], table_word(r)) for r in TABLE], exe
        for bad in ("5S85 90 0\n", "S85M 90 0\n", "5Q85M 90 0\n", "5S85M 90\n", "5S85M 90 0 1\n", "5S85M -1 0\n", "268435456M 90 0\n"):
            p = subprocess.run([exe, "words"], input=bad.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=SAN_ENV)
            clean(p, exe)
            assert p.returncode == 2, (exe, bad)


def test_the_host_reader_gives_every_record_of_the_chr21_bams_the_parsed_word(checkers):
    n_soft = 0
    piled = 0
    for bam in BAMS:
        recs = parse_bam_cigars(os.path.join(CHR21, bam))
        exp = words_of_bam(recs)
        n_soft += sum(1 for c in recs["cigar"] for _, op in c if op == "S")
        piled += int(((recs["pos"] + 1 == 29185119) & ((exp & 255) >= 5)).sum())
        for exe in checkers:
            p = subprocess.run([exe, "bam", os.path.join(CHR21, bam)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=SAN_ENV)
            clean(p, exe)
            assert p.returncode == 0
            got = np.array([[int(v) for v in l.split()] for l in p.stdout.decode().splitlines()], dtype=np.int64)
            assert got.shape == (len(exp), 4)
            np.testing.assert_array_equal(got[:, 0], recs["tid"])
            np.testing.assert_array_equal(got[:, 1], recs["pos"])
            np.testing.assert_array_equal(got[:, 2], recs["flag"])
            np.testing.assert_array_equal(got[:, 3], exp.astype(np.int64), err_msg=bam)
    assert n_soft == 689            # (the fixture's soft clips: the comparison above is not one of zeros)
    assert piled == 20              # the pile of left clips at 21:29185119


def test_the_writers_cigars_are_what_a_plain_parse_reads_back(tmp_path):
    for index in (False, True):
        path = str(tmp_path / ("syn%d.bam" % index))
        soa, cigars, words = synthetic_bam(path, n=600, index=index)
        back = parse_bam_cigars(path)
        assert back["cigar"] == [cigar_of(c) for c in cigars]
        np.testing.assert_array_equal(back["pos"], soa["pos"])
        np.testing.assert_array_equal(words_of_bam(back), words)
        assert os.path.exists(path + ".bai") == index
    assert len(set(words.tolist())) > 25 and (words == 0).any() and ((words >> 16) == 65535).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the INFO keys and the winner
# ---------------------------------------------------------------------------------------------------------------------------------
def end(held=1, pos=1000, n_left=0, n_right=0, pos_left=0, pos_right=0, peak_left=0, peak_right=0):
    return (held, pos, n_left, n_right, pos_left, pos_right, peak_left, peak_right)


def restated(e1, e2, swapped, support):
    """the writer's rules, written out"""
    first, second = (e2, e1) if swapped else (e1, e2)

    def entry(key, e):
        held, pos, n_left, n_right, pos_left, pos_right, peak_left, peak_right = e
        if not held:
            return "."
        if key == "CLN":
            return str(n_left + n_right)
        piles = [(-peak_left, abs(pos_left - pos), 0, pos_left, "L"), (-peak_right, abs(pos_right - pos), 1, pos_right, "R")]
        peak, _, _, x, side = sorted(p for p in piles if p[0] < 0)[0] if (peak_left or peak_right) else (0, 0, 0, 0, "")
        if -peak < support or not side:
            return "."
        return dict(CLPOS=str(x), CLSUP=str(-peak), CLSIDE=side)[key]

    return "".join(";%s=%s,%s" % (k, entry(k, first), entry(k, second)) for k in KEYS)


BOTH = end(n_left=9, n_right=4, pos_left=990, pos_right=1003, peak_left=5, peak_right=3)
CASES = [(BOTH, end(pos=2000, n_right=6, pos_right=2001, peak_right=6), 0, 2),                       # the larger peak wins, either side
         (BOTH, end(pos=2000, n_right=6, pos_right=2001, peak_right=6), 1, 2),                       # swapped: the second site end prints first
         (end(n_left=4, n_right=4, pos_left=990, pos_right=1003, peak_left=4, peak_right=4), BOTH, 0, 2),    # equal peaks: the nearer (R at 3 against L at 10)
         (end(n_left=4, n_right=4, pos_left=997, pos_right=1004, peak_left=4, peak_right=4), BOTH, 0, 2),    # ... the nearer is L
         (end(n_left=4, n_right=4, pos_left=997, pos_right=1003, peak_left=4, peak_right=4), BOTH, 0, 2),    # equal peaks, equal distance: L
         (end(n_left=4, n_right=4, pos_left=1000, pos_right=1000, peak_left=4, peak_right=4), BOTH, 0, 2),   # ... both on P itself: L
         (end(n_left=3, n_right=1, pos_left=990, pos_right=1001, peak_left=1, peak_right=1), BOTH, 0, 2),    # the winner below the support: three dots, CLN stays
         (end(n_left=3, n_right=1, pos_left=990, pos_right=1001, peak_left=1, peak_right=1), BOTH, 0, 1),    # ... support 1: printed
         (BOTH, BOTH, 0, 5), (BOTH, BOTH, 0, 6),                                                      # the peak at the support, and one below
         (end(), end(pos=1), 0, 1),                                                                   # no observation: CLN=0 and dots, at any support
         (BOTH, end(held=0), 0, 2), (BOTH, end(held=0), 1, 2),                                        # an end that is not held: '.' in every key
         (end(held=0, n_left=5, pos_left=7, peak_left=5), BOTH, 0, 2),
         (end(pos=2**31 - 1, n_left=2**32 - 1, n_right=2**32 - 1, pos_left=2**31 - 1, pos_right=1, peak_left=2**32 - 1, peak_right=2**32 - 1), BOTH, 0, 2**30)]


def test_the_restatement_on_cases_worked_out_by_hand():
    assert restated(*CASES[0]) == ";CLN=13,6;CLPOS=990,2001;CLSUP=5,6;CLSIDE=L,R"
    assert restated(*CASES[1]) == ";CLN=6,13;CLPOS=2001,990;CLSUP=6,5;CLSIDE=R,L"
    assert restated(*CASES[2]).startswith(";CLN=8,13;CLPOS=1003,990;CLSUP=4,5;CLSIDE=R,L")
    assert restated(*CASES[3]).startswith(";CLN=8,13;CLPOS=997,")
    assert restated(*CASES[4]) == ";CLN=8,13;CLPOS=997,990;CLSUP=4,5;CLSIDE=L,L"
    assert restated(*CASES[6]) == ";CLN=4,13;CLPOS=.,990;CLSUP=.,5;CLSIDE=.,L"
    assert restated(*CASES[7]) == ";CLN=4,13;CLPOS=1001,990;CLSUP=1,5;CLSIDE=R,L"
    assert restated(*CASES[9]) == ";CLN=13,13;CLPOS=.,.;CLSUP=.,.;CLSIDE=.,."
    assert restated(*CASES[10]) == ";CLN=0,0;CLPOS=.,.;CLSUP=.,.;CLSIDE=.,."
    assert restated(*CASES[12]) == ";CLN=.,13;CLPOS=.,990;CLSUP=.,5;CLSIDE=.,L"
    assert restated(*CASES[14]) == ";CLN=8589934590,13;CLPOS=2147483647,.;CLSUP=4294967295,.;CLSIDE=L,."


def test_clip_info_on_a_table_of_cases(checkers):
    for exe in checkers:
        for c in CASES:
            e1, e2, sw, support = c
            line = " ".join(str(v) for v in e1 + e2 + (sw,)) + "\n"
            p = subprocess.run([exe, "keys", str(support)], input=line.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=SAN_ENV)
            clean(p, exe)
            assert p.returncode == 0 and p.stdout.decode().splitlines() == [restated(*c)], (exe, c, p.stdout)
        for bad in ("1 2 3\n", " ".join(["1"] * 16) + " x\n", " ".join(["1"] * 18) + "\n", " ".join(["1"] * 16) + " -1\n"):
            p = subprocess.run([exe, "keys", "2"], input=bad.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=SAN_ENV)
            clean(p, exe)
            assert p.returncode == 2, (exe, bad)
        for bad_args in (["keys", "0"], ["keys", "x"], ["keys", str(2**30 + 1)], ["keys"], ["bam"], ["words", "1"], []):
            p = subprocess.run([exe] + bad_args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=SAN_ENV)
            clean(p, exe)
            assert p.returncode == 2, (exe, bad_args)


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def test_usage_text_names_the_options():
    p = run_tool(EXE, [], CHR21)
    err = p.stderr.decode()
    assert p.returncode == 1
    for opt in ("--clip ", "--clip-window INT", "--clip-min INT", "--clip-support INT"):
        assert opt in err, opt


def test_usage_errors_exit_1_before_the_gpu_is_touched(tmp_path):
    out = str(tmp_path / "o.vcf")
    needs = "--clip needs --vcf FILE or --sites-vcf FILE to write to (and --clip-window, --clip-min and --clip-support go with --clip)."
    takes = "--clip-%s takes an integer from %d to %d, not '%s'."
    cases = [(["--clip"], needs),                                                           # 1. nothing to write to
             (["--clip", "--clip-window", "100"], needs),
             (["--vcf", out, "--clip-window", "100"], needs),                               # 2. a --clip-* option without --clip
             (["--vcf", out, "--clip-min", "10"], needs),
             (["--vcf", out, "--clip-support", "2"], needs),
             (["--vcf", out, "--mapq", "--clip-window", "100"], needs),                     # (--mapq is not --clip)
             (["--clip-support", "2"], needs)]
    for name, lo, hi in (("window", 0, 1023), ("min", 1, 255), ("support", 1, 2**30)):      # 3. - 5. a value outside its range, or no integer
        for bad in (str(lo - 1), str(hi + 1), "x", "12x", ""):
            cases.append((["--vcf", out, "--clip", "--clip-" + name, bad], takes % (name, lo, hi, bad)))
    for args, message in cases:
        p = run_tool(EXE, args + ["inv_del_bam_config"], CHR21)
        err = p.stderr.decode()
        assert p.returncode == 1 and err.strip() == message, (args, err)
        assert not p.stdout.decode().strip(), (args, err)
    assert not os.path.exists(out)     # (a usage error: nothing was opened)
    # the other tools do not take the option
    for tool in ("bam2cfg", "bdx-dump-reads"):
        p = run_tool(os.path.join(ROOT, "bin", tool), ["--clip", "inv_del_bam_config"], CHR21)
        assert p.returncode != 0, tool
