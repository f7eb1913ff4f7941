"""CPU tests of --anchor: the CLI's call, merge and table (host/anchor.cpp through bin/bdx-anchor-check) against the Python restatement of
tests/anchor_cases.py on hand-written rows; the default window and step; the restatement's own rows on hand-made windows; the layout
of bdx_anchor_split against the header; and the option errors of the command.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import anchor_cases as A
from helpers import GOLDEN, ROOT

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHECK = os.path.join(ROOT, "bin", "bdx-anchor-check")
NAMES = ["chrA", "chrB", "chrC"]


def build():
    if not os.path.exists(CHECK) or not os.path.exists(EXE):
        import __graft_entry__ as g
        g.build()


def row(last_left, first_right, u_left=3, u_right=3, n_left=None, n_right=None, n_low=0, split=None):
    """a row as the kernel would write it for a call: split = last_left + 1"""
    n_left, n_right = u_left if n_left is None else n_left, u_right if n_right is None else n_right
    return dict(n_fwd=n_left + 1, n_rev=n_right + 2, n_low=n_low, n_left=n_left, n_right=n_right, u_left=u_left, u_right=u_right,
                split=last_left + 1 if split is None else split, last_left=last_left, first_right=first_right)


# (name, --min, [(seq, row)] in grid order, the rows of the table that must come out: (chrom, Pos1, Pos2, Windows) or None: not stated)
LEN_B = 5000
HAND = [
    ("an empty table", 3, [(0, row(100, 120, u_left=2)), (0, row(100, 120, u_right=0)), (1, row(-1, 50, u_left=0, n_left=0, split=0))], []),
    ("no rows at all", 3, [], []),
    ("one call, seen by two windows", 3, [(0, row(1000, 1010)), (0, row(1000, 1010))], [("chrA", 1001, 1011, 2)]),
    ("a chain: a-b and b-c intersect, a-c do not", 1, [(0, row(100, 200)), (0, row(200, 300, u_left=4)), (0, row(300, 400))], [("chrA", 201, 301, 3)]),
    ("a chain closed by a long member", 1, [(0, row(100, 1000, u_left=1, u_right=1)), (0, row(300, 320)), (0, row(900, 950)), (0, row(1001, 1002))],
     None),
    ("touching ends merge, one apart does not", 1, [(0, row(100, 200)), (0, row(200, 250, u_left=5)), (0, row(251, 300))],
     [("chrA", 201, 251, 2), ("chrA", 252, 301, 1)]),
    ("the same positions on two sequences stay apart", 2, [(0, row(100, 200)), (1, row(100, 200)), (2, row(150, 160))],
     [("chrA", 101, 201, 1), ("chrB", 101, 201, 1), ("chrC", 151, 161, 1)]),
    ("tie on distinct starts: the more anchors", 1, [(0, row(100, 200, n_left=3, n_right=3)), (0, row(150, 180, n_left=9, n_right=3))], [("chrA", 151, 181, 2)]),
    ("tie on both: the smaller split", 1, [(0, row(150, 180)), (0, row(100, 200))], [("chrA", 101, 201, 2)]),
    ("tie on all three: the first in grid order", 1, [(0, row(100, 200, n_low=7)), (0, row(100, 190, n_low=1))], [("chrA", 101, 201, 2)]),
    ("rows out of position order come out in order", 1, [(1, row(900, 910)), (0, row(500, 510)), (1, row(100, 110)), (0, row(10, 20))],
     [("chrA", 11, 21, 1), ("chrA", 501, 511, 1), ("chrB", 101, 111, 1), ("chrB", 901, 911, 1)]),
    ("a contig's first and last window", 3, [(1, row(0, 1)), (1, row(0, 1)), (1, row(LEN_B - 2, LEN_B - 1)), (0, row(0, 1)), (0, row(2**31 - 3, 2**31 - 2))],
     [("chrA", 1, 2, 1), ("chrA", 2**31 - 2, 2**31 - 1, 1), ("chrB", 1, 2, 2), ("chrB", LEN_B - 1, LEN_B, 1)]),
    ("--anchor-min at its edges", 4, [(0, row(100, 110, u_left=4, u_right=4)), (0, row(300, 310, u_left=3, u_right=9)), (0, row(500, 510, u_left=9, u_right=3))],
     [("chrA", 101, 111, 1)]),
]


def run_check(tmp_path, seq_rows, minimum):
    build()
    f = tmp_path / "rows.txt"
    f.write_text(A.rows_text(seq_rows))
    args = [CHECK, str(f), "--min", str(minimum)]
    for n in NAMES:
        args += ["--contig", n]
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    text = p.stdout.decode()
    return int(text.split("\n")[0].split("\t")[1]), text[text.index("#Chr"):]


@pytest.mark.parametrize("name", [h[0] for h in HAND])
def test_merge_and_table_equal_the_restatement(name, tmp_path):
    _, minimum, seq_rows, stated = [h for h in HAND if h[0] == name][0]
    want = A.table_of_rows(seq_rows, minimum, NAMES)
    if stated is not None:         # the restatement itself gives what the case was written to give
        got = [l.split("\t") for l in want.rstrip("\n").split("\n")[1:]]
        assert [(g[0], int(g[1]), int(g[2]), int(g[9])) for g in got] == stated, got
        assert all(g[3] == "INS" for g in got)
    ncalls, body = run_check(tmp_path, seq_rows, minimum)
    assert ncalls == sum(A.calls(r, minimum) for _, r in seq_rows)
    assert body == want


def test_merge_on_random_rows_equals_the_restatement(tmp_path):
    rng = np.random.default_rng(7)
    for trial in range(6):
        seq_rows = []
        for _ in range(120):
            ll = int(rng.integers(0, 4000))
            seq_rows.append((int(rng.integers(0, 3)), row(ll, ll + int(rng.integers(0, 60)), u_left=int(rng.integers(0, 6)), u_right=int(rng.integers(0, 6)),
                                                          n_left=int(rng.integers(6, 9)), n_right=int(rng.integers(6, 9)), n_low=int(rng.integers(0, 3)))))
        minimum = 1 + trial % 3
        want = A.table_of_rows(seq_rows, minimum, NAMES)
        lines = want.count("\n") - 1
        assert 3 < lines < sum(A.calls(r, minimum) for _, r in seq_rows)        # some rows merge, some stay alone
        assert run_check(tmp_path, seq_rows, minimum)[1] == want, trial


def test_check_tool_refuses_malformed_input(tmp_path):
    build()
    good = "0 1 1 0 1 1 1 1 11 10 12\n"
    for text in ("0 1 1 0 1 1 1 1 11 10\n", good.replace("\n", " 5\n"), "3" + good[1:], "0 1 1 0 1 1 1 1 -1 10 12\n", "0 x 1 0 1 1 1 1 11 10 12\n"):
        f = tmp_path / "bad.txt"
        f.write_text(text)
        p = subprocess.run([CHECK, str(f), "--min", "1", "--contig", "a"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 2, text
    for bad in ([], ["--min", "1"], [str(tmp_path / "bad.txt"), "--min", "0", "--contig", "a"], [str(tmp_path / "bad.txt"), "--min", "1"],
                ["--cutoffs", "x"], ["--cutoffs", "400", "--bogus"]):
        assert subprocess.run([CHECK] + bad, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60).returncode == 2, bad


@pytest.mark.parametrize("cutoffs,window,step", [
    ([490.0], None, None), ([490.5], None, None), ([489.99, 300.0, 610.25], None, None), ([float("inf"), 375.0], None, None),
    ([float("nan"), 375.0, float("-inf")], None, None), ([0.4], None, None), ([0.5, -3.0], None, None), ([2.0**31], None, None),
    ([536870912.0], None, None), ([536870912.5], None, None), ([490.0], 1, None), ([490.0], 7, None), ([490.0], 2, None), ([490.0], 1 << 30, None),
    ([490.0], 1000, 1), ([490.0], 1000, 333), ([490.0], None, 100), ([float("inf")], 50, None)])
def test_default_window_and_step(cutoffs, window, step):
    build()
    w = window if window is not None else A.default_window(cutoffs)
    assert w is not None
    s = step if step is not None else A.default_step(w)
    args = [CHECK, "--cutoffs", ",".join(repr(float(c)) for c in cutoffs), "--length", "1000001"]
    args += (["--window", str(window)] if window is not None else []) + (["--step", str(step)] if step is not None else [])
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode() == "window\t%d\tstep\t%d\twindows\t%d\n" % (w, s, A.grid(1000001, s))
    assert 1 <= s and 1 <= w <= 1 << 30
    if window is None and step is None and w > 1:
        # with the defaults every junction position lies in the middle half of some window (or in the first window's first quarter)
        for x in (0, s - 1, s, w - 1, w, 999_999, 1_000_000):
            assert any(j * s + w // 4 <= x < j * s + w - w // 4 or (j == 0 and x < w // 4) for j in range(max(x // s - 2, 0), x // s + 1)), x


def test_default_window_needs_a_finite_positive_cutoff():
    build()
    for cutoffs in ([float("inf")], [float("nan"), float("inf")], [0.0], [-5.0, 0.0], [-0.5]):
        assert A.default_window(cutoffs) is None
        p = subprocess.run([CHECK, "--cutoffs", ",".join(repr(c) for c in cutoffs)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 1 and p.stdout.decode().startswith("error\t") and "--anchor-window" in p.stdout.decode(), cutoffs


def test_restatement_on_hand_made_windows(tmp_path):
    """the rule itself, on windows small enough to check by eye (and, inside split_row, at every S of the window); the rows then go
    through the check tool as one sequence's, so that the two halves are held together once"""
    cases = [
        # (R, L, beg, end) -> (split, n_left, n_right, u_left, u_right, last_left, first_right)
        (([], [], 10, 50), (10, 0, 0, 0, 0, -1, -1)),
        (([12, 12, 15], [], 10, 50), (16, 3, 0, 2, 0, 15, -1)),
        (([], [12, 30], 10, 50), (10, 0, 2, 0, 2, -1, 12)),
        (([12, 14, 16], [20, 22, 22], 10, 50), (17, 3, 3, 3, 2, 16, 20)),
        (([20], [12], 10, 50), (10, 0, 1, 0, 1, -1, 12)),                    # the wrong way round: 1 either way, the smallest S
        (([12], [12], 10, 50), (10, 0, 1, 0, 1, -1, 12)),                    # both at one position: S = 10 .. 12 give 1, S = 13 gives 1: the smallest
        (([12, 12], [12], 10, 50), (13, 2, 0, 1, 0, 12, -1)),
        (([12, 14, 16], [11, 13, 15], 10, 50), (10, 0, 3, 0, 3, -1, 11)),    # alternating, a left-pointing one first: 3 at S = 10, 13, 15, 17: the smallest
        (([11, 13, 15], [12, 14, 16], 10, 50), (12, 1, 3, 1, 3, 11, 12)),    # alternating, a right-pointing one first: 4 at S = 12, 14, 16
        (([12, 14, 16], [13, 15, 17], 10, 50), (13, 1, 3, 1, 3, 12, 13)),
        (([12, 13, 30, 31, 32], [14, 15, 33, 34, 35], 10, 50), (33, 5, 3, 5, 3, 32, 33)),     # two clusters: the better split
        (([10], [49], 10, 50), (11, 1, 1, 1, 1, 10, 49)),                    # the window's first and last position
        (([2**31 - 3], [2**31 - 2], 2**31 - 10, 2**31 - 1), (2**31 - 2, 1, 1, 1, 1, 2**31 - 3, 2**31 - 2)),
        (([5], [6], 7, 7), (7, 0, 0, 0, 0, -1, -1)),
    ]
    rows = []
    for (R, L, beg, end), want in cases:
        r = A.split_row(R, L, 0, beg, end)
        assert (r["split"], r["n_left"], r["n_right"], r["u_left"], r["u_right"], r["last_left"], r["first_right"]) == want, ((R, L, beg, end), r)
        assert r["split"] == (r["last_left"] + 1 if r["n_left"] else beg)
        rows.append((0, r))
    assert sum(A.calls(r, 1) for _, r in rows) >= 5
    assert run_check(tmp_path, rows, 1)[1] == A.table_of_rows(rows, 1, NAMES)


def test_struct_layout_equals_the_header():
    from breakdancer_amd import _lib
    text = open(os.path.join(ROOT, "include", "bdx.h")).read()
    body = re.search(r"typedef struct bdx_anchor_split \{(.*?)\} bdx_anchor_split;", text, re.S).group(1)
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"uint32_t": "<u4", "int32_t": "<i4"}[ctype]) for n in names.split(",")]
    dt = _lib.ANCHOR_SPLIT_DTYPE
    assert [(n, dt.fields[n][0].str) for n in dt.names] == fields and tuple(dt.names) == A.FIELDS
    assert dt.itemsize == 40 and [dt.fields[n][1] for n in dt.names] == list(range(0, 40, 4))
    assert "bdx_window_anchor_split" in _lib.EXPORTS
    assert re.search(r"int bdx_window_anchor_split\(bdx_ctx\* ctx, const bdx_interval\* iv, size_t n, int32_t min_qual, bdx_anchor_split\* out", text)


def run_cli(args, env=None, cwd=None):
    build()
    return subprocess.run([EXE] + args, cwd=cwd, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("env", [{}, {"BDX_FOREGROUND": "1"}])
def test_cli_usage_errors(env, tmp_path):
    cwd = os.path.join(GOLDEN, "chr21")
    out = str(tmp_path / "anchor.txt")
    bad = [["--anchor-window", "100"], ["--anchor-step", "5"], ["--anchor-min", "3"], ["--anchor-mapq", "0"]]
    for name, lo, hi in (("window", 1, 2**30), ("step", 1, 2**30), ("min", 1, 2**30), ("mapq", 0, 255)):
        bad += [["--anchor", out, "--anchor-" + name, v] for v in (str(lo - 1), str(hi + 1), "x", "3.5", "")]
    for args in bad:
        p = run_cli(args + ["inv_del_bam_config"], env, cwd)
        assert p.returncode == 1 and b"--anchor" in p.stderr and p.stdout == b"", (args, p.stderr)
    p = run_cli(["--anchor"], env, cwd)
    assert p.returncode == 1
    # no finite positive cutoff and no --anchor-window: before the GPU is touched (the BAM it names does not even exist)
    cfg = tmp_path / "bare.cfg"
    cfg.write_text("readgroup:rg0\tplatform:illumina\tmap:none.bam\treadlen:50.00\tlib:lib0\tnum:10\tlower:0.00\tupper:0.00\tmean:0.00\tstd:0.00\n")
    p = run_cli(["--anchor", out, str(cfg)], env, str(tmp_path))
    assert p.returncode == 1 and b"--anchor-window" in p.stderr and b"bdx_create" not in p.stderr and p.stdout == b""
    # an unwritable FILE
    p = run_cli(["--anchor", str(tmp_path / "no" / "dir" / "f"), "inv_del_bam_config"], env, cwd)
    assert p.returncode == 1 and b"--anchor file" in p.stderr and p.stdout == b""
