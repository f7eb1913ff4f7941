"""CPU tests of --mini: the score of a row (bdx_insert_shift_score, csrc/bdx_mini.h) and the CLI's window call, threshold, merge and table
(host/mini.cpp through bin/bdx-mini-check) against the Python restatement of tests/mini_cases.py; the restatement's own D against the
definition of the Kolmogorov-Smirnov distance, exactly; and the option errors of the command.  No GPU."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mini_cases as M
from helpers import GOLDEN, ROOT

EXE = os.path.join(ROOT, "bin", "breakdancer-max")
CHECK = os.path.join(ROOT, "bin", "bdx-mini-check")

# The tolerance of the score, 1e-12 relative.  Derivation: a score is computed for lambda >= 0.4 only.  There term j of the series is
# exp(-2 (j^2 - 1) lambda^2) <= exp(-0.32 (j^2 - 1)): 1, 0.38, 0.077, 0.008, ... -- the terms fall at least that fast, the sum is reached
# within 12 terms, and since the series alternates with falling terms the sum lies between 1 - 0.38 and 1: the additions cancel by less than
# a factor of 3.  exp and log are good to an ulp or two (2e-16), their arguments -- products of a few doubles -- likewise, so the relative
# error of ln p = ln 2 - 2 lambda^2 + ln S stays within some tens of ulps: several orders below 1e-12, whichever libm evaluates it.
RTOL = 1e-12


def build():
    if not os.path.exists(CHECK) or not os.path.exists(EXE):
        import __graft_entry__ as g
        g.build()


def close(a, b):
    return abs(a - b) <= RTOL * max(abs(a), abs(b))


def row(n, t_plus=0, t_minus=0, saturated=0, total=0, n_over=0):
    return (n, n_over, saturated, 0, total, t_plus, t_minus)


def score_rows():
    """(row, N) pairs: n = 1, 2, 20, 4096; D = 0, tiny, 0.05 .. 1; lambda on both sides of 0.4; lambda = 30; N = 0; saturated rows"""
    out = []
    N = 1_000_003
    for n in (1, 2, 20, 4096):
        for D in (0.0, 1e-9, 0.05, 0.1, 0.2, 0.35, 0.5, 0.75, 0.999, 1.0):
            t = int(round(D * n * N))
            out.append((row(n, t_plus=t, t_minus=t // 3), N))
            out.append((row(n, t_plus=t // 2, t_minus=t), N))
        c = math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)
        edge = int(0.4 / c * n * N)
        for t in (edge - 1, edge, edge + 1, edge + 2):
            if 0 <= t <= n * N:
                out.append((row(n, t_plus=t), N))
        out.append((row(n, t_plus=n * N), 0))                          # N == 0
        out.append((row(n, t_plus=n * N, saturated=1), N))             # a saturated row (the kernel writes t = 0 there; the score ignores t anyway)
    c = math.sqrt(4096) + 0.12 + 0.11 / 64.0
    out.append((row(4096, t_minus=int(30.0 / c * 4096 * N)), N))       # lambda = 30: exp(-2 lambda^2) underflows
    out.append((row(0), N))
    out.append((row(20, t_plus=20 * (2**51 - 1)), 2**51 - 1))          # the largest null
    return out


def test_score_rows_cover_what_they_should():
    lams = [M.lam_of(r[0], M.score(r, N)[1]) for r, N in score_rows() if r[0] and N and not r[2]]
    assert any(0.399 < l < 0.4 for l in lams) and any(0.4 <= l < 0.401 for l in lams)
    assert any(29.9 < l < 30.1 for l in lams) and math.exp(-2 * 30.0 ** 2) == 0.0      # (where a naive exp underflows)
    assert {r[0] for r, _ in score_rows()} >= {0, 1, 2, 20, 4096}
    big = [M.score(r, N)[0] for r, N in score_rows()]
    assert max(big) > 7000 and all(math.isfinite(s) and s >= 0 for s in big)


def test_library_score_equals_the_restatement():
    build()
    from breakdancer_amd import _lib, api
    assert _lib.INSERT_SHIFT_DTYPE.itemsize == 40 and _lib.MINI_CAP == M.MINI_CAP and _lib.ISIZE_BINS == M.ISIZE_BINS
    assert [_lib.INSERT_SHIFT_DTYPE.fields[k][1] for k in ("n", "n_over", "saturated", "pad", "sum", "t_plus", "t_minus")] == [0, 4, 8, 12, 16, 24, 32]
    for r, N in score_rows():
        sc, D = api.insert_shift_score(r, N)
        esc, eD = M.score(r, N)
        assert D == eD, (r, N, D, eD)                                   # (one division of two doubles)
        assert close(sc, esc) and (sc == 0) == (esc == 0), (r, N, sc, esc)
    import ctypes as C
    lib = _lib.load()
    assert lib.bdx_insert_shift_score(None, 5, None, None) == 1          # BDX_EINVAL: no row
    one = np.zeros(1, dtype=_lib.INSERT_SHIFT_DTYPE)
    assert lib.bdx_insert_shift_score(one.ctypes.data_as(C.c_void_p), 5, None, None) == 0   # either result may be left out


def run_check(tmp_path, rows_by_window, N, mu, window, step, contigs, min_pairs=None, score=None):
    build()
    f = tmp_path / "rows.txt"
    f.write_text(M.rows_text(rows_by_window))
    args = [CHECK, str(f), "--n", ",".join(str(x) for x in N), "--mu", ",".join(repr(float(x)) for x in mu), "--window", str(window), "--step", str(step)]
    if min_pairs is not None:
        args += ["--min-pairs", str(min_pairs)]
    if score is not None:
        args += ["--score", str(score)]
    for name, length in contigs:
        args += ["--contig", "%s:%d" % (name, length)]
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    scored = [l.split("\t")[1:] for l in lines if l.startswith("row\t")]
    thr = [l.split("\t") for l in lines if l.startswith("threshold\t")]
    assert len(thr) == 1
    table = p.stdout.decode()[p.stdout.decode().index("#Chr"):]
    return scored, dict(threshold=int(thr[0][1]), scoring=int(thr[0][3]), saturated=int(thr[0][5])), table


def expected_table(rows_by_window, N, mu, window, step, contigs, min_pairs=20, score=None):
    lengths = [l for _, l in contigs]
    first = np.concatenate([[0], np.cumsum([M.grid(l, step) for l in lengths])])
    calls = {}
    for w, rows in rows_by_window.items():
        seq = int(np.searchsorted(first, w, "right")) - 1
        calls[(seq, int(w - first[seq]))] = M.window_call(rows, N, mu, min_pairs)
    W = sum(c is not None for c in calls.values())
    thr = score if score is not None else M.default_threshold(W)
    return M.table_text(M.merge(calls, thr, window, step, lengths), [n for n, _ in contigs]), thr, W


def test_check_tool_scores_equal_the_restatement(tmp_path):
    cases = [c for c in score_rows() if c[1] == 1_000_003]
    rows_by_window = {w: [r] for w, (r, _) in enumerate(cases)}
    scored, _, _ = run_check(tmp_path, rows_by_window, [1_000_003], [300.0], 100, 50, [("c", 100 * len(cases))])
    kept = [(w, r) for w, (r, _) in enumerate(cases) if any(r)]
    assert len(scored) == len(kept) > 80
    for (w, r), (sw, sl, ssc, sd) in zip(kept, scored):
        esc, eD = M.score(r, 1_000_003)
        assert (int(sw), int(sl)) == (w, 0) and float(sd) == eD and close(float(ssc), esc), (r, ssc, esc)


def strong(n, N, del_=True, frac=0.9, mu=300.0, size=40):
    """a row that scores high: D = frac, shifted by `size` to the DEL or the INS side"""
    t = int(frac * n * N)
    total = int(n * (mu + (size if del_ else -size)))
    return row(n, t_plus=0 if del_ else t, t_minus=t if del_ else 0, total=total)


def test_merge_and_table_equal_the_restatement(tmp_path):
    N, mu = [50_000, 80_000, 999], [300.0, 412.5, 200.0]           # (library 2 is not usable: its rows never score)
    contigs = [("chrA", 1000), ("chrB", 1030), ("chrC", 77)]
    window, step = 100, 50
    first = [0, M.grid(1000, step), M.grid(1000, step) + M.grid(1030, step)]
    assert first == [0, 20, 41] and M.grid(77, step) == 2
    z = row(0)
    weak = row(25, t_plus=int(0.2 * 25 * 50_000), total=25 * 305)
    rw = {
        2: [strong(40, N[0]), z, z], 3: [strong(60, N[0], frac=0.95), strong(30, N[1], frac=0.5, mu=412.5), z], 4: [strong(40, N[0]), z, z],   # a run of three; the best in the middle
        5: [weak, z, z],                                                                                  # broken by a sub-threshold window
        6: [strong(40, N[0]), z, z],
        7: [strong(40, N[0], del_=False), z, z],                                                          # broken by a Type change
        9: [strong(50, N[0], del_=False), z, z],                                                          # a single window (8 is missing: all zeros)
        10: [z, z, strong(500, N[2])],                                                                    # only an unusable library: no scoring row
        11: [row(19, t_plus=19 * N[0], total=19 * 400), z, z],                                            # below min-pairs
        12: [row(5000, saturated=1, total=5000 * 300), row(30, saturated=1, total=30 * 400), z],          # saturated
        19: [strong(40, N[0]), z, z],                                                                     # the last window of chrA ...
        20: [strong(40, N[0]), z, z],                                                                     # ... and the first of chrB: a sequence change
        first[1] + 20: [z, strong(45, N[1], mu=412.5), z],                                                 # chrB's last window [1000, 1100): End clamped to 1030
        first[2] + 1: [strong(40, N[0]), z, z],                                                           # chrC's window [50, 150) on a contig of 77
    }
    for min_pairs, score in ((None, None), (20, 35), (30, None), (2, 0), (20, 99999)):
        scored, info, table = run_check(tmp_path, rw, N, mu, window, step, contigs, min_pairs, score)
        exp, thr, W = expected_table(rw, N, mu, window, step, contigs, min_pairs or 20, score)
        assert info["threshold"] == thr and info["scoring"] == W and info["saturated"] == 1
        assert table == exp, (min_pairs, score, table, exp)
    _, info, table = run_check(tmp_path, rw, N, mu, window, step, contigs)
    rows = [l.split("\t") for l in table.rstrip("\n").split("\n")[1:]]
    assert info["threshold"] == 20 + 10 + 1                         # (W = 11 .. 12: 10 < W <= 12)
    assert [(r[0], r[1], r[2], r[3], r[8]) for r in rows] == [
        ("chrA", "101", "300", "DEL", "3"), ("chrA", "301", "400", "DEL", "1"), ("chrA", "351", "450", "INS", "1"), ("chrA", "451", "550", "INS", "1"),
        ("chrA", "951", "1000", "DEL", "1"), ("chrB", "1", "100", "DEL", "1"), ("chrB", "1001", "1030", "DEL", "1"), ("chrC", "51", "77", "DEL", "1")]
    assert rows[0][6] == "90" and rows[0][4] == "40.0" and rows[0][7] == "0.950"   # the best window of the run of three: both libraries' pairs, the better D
    assert rows[2][4] == "-40.0"
    # a score above the cap prints as 99999 (one row reaches 35,710 at most: n = BDX_MINI_CAP, D = 1; three libraries together pass the cap)
    full = row(4096, t_plus=4096 * 50_000, total=4096 * 400)
    _, _, table = run_check(tmp_path, {0: [full, full, full]}, [50_000] * 3, [300.0] * 3, window, step, contigs)
    assert table.split("\n")[1].split("\t")[5] == "99999" and 99999 < 3 * M.score(full, 50_000)[0] < 3 * 35711


def test_default_threshold(tmp_path):
    assert [M.default_threshold(W) for W in (0, 1, 10, 11, 100, 101, 10**7, 10**7 + 1)] == [20, 20, 30, 31, 40, 41, 90, 91]
    N, mu = [50_000], [300.0]
    for W, thr in ((1, 20), (10, 30), (11, 31)):
        rw = {w: [strong(40, N[0])] for w in range(0, 2 * W, 2)}
        _, info, _ = run_check(tmp_path, rw, N, mu, 100, 50, [("c", 100_000)])
        assert (info["scoring"], info["threshold"]) == (W, thr)
    for W in (10**4, 10**4 + 1):
        rw = {w: [row(20, t_plus=1, total=6000)] for w in range(W)}
        _, info, table = run_check(tmp_path, rw, N, mu, 100, 50, [("c", 50 * W)])
        assert (info["scoring"], info["threshold"]) == (W, M.default_threshold(W)) and table.count("\n") == 1
    # W = 10^7 and the other counts no rows file should hold: mini_default_threshold itself, through the tool.  Every power of ten is a
    # point where 10 log10 W is an integer, so that one ulp in a pow or a log10 would move the result by one; the counts beside them, and
    # the integers nearest to the irrational steps 10^(r / 10) between two decades, frame every change of the result
    Ws = [0, 1, 2, 10, 11, 10**7 - 1, 10**7, 10**7 + 1, 2**64 - 1]
    Ws += [10**d + e for d in range(2, 20) for e in (-1, 0, 1)]
    Ws += [int(10 ** (d + r / 10.0)) + e for d in (0, 3, 6, 7, 12) for r in range(1, 10) for e in (0, 1)]
    p = subprocess.run([CHECK] + [a for W in Ws for a in ("--scoring-windows", str(W))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    got = [l.split("\t") for l in p.stdout.decode().rstrip("\n").split("\n")]
    assert [(g[0], int(g[1])) for g in got] == [("default-threshold", W) for W in Ws]
    by_w = {int(g[1]): int(g[2]) for g in got}
    assert (by_w[1], by_w[10], by_w[11], by_w[10**7], by_w[10**7 + 1], by_w[10**7 - 1]) == (20, 30, 31, 90, 91, 90)
    for W in Ws:
        assert by_w[W] == M.default_threshold(W), W
    for bad in (["--scoring-windows"], ["--scoring-windows", "x"], ["--scoring-windows", "5", "--n", "3"], ["--scoring-windows", "-5"]):
        assert subprocess.run([CHECK] + bad, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60).returncode == 2, bad


def test_d_formula_equals_the_definition_of_the_ks_distance():
    """sup over every integer x of |F_n(x) - F(x)|, in exact fractions, against max(t_plus, t_minus) / (n N) of the restatement"""
    rng = np.random.default_rng(12)
    for k in range(12):
        n = int(rng.integers(1, 40))
        centre, width = int(rng.integers(0, M.ISIZE_BINS)), int(rng.integers(1, 400))
        hist = np.zeros(M.ISIZE_BINS, np.int64)
        vals = np.clip(rng.normal(centre, width, 5000).astype(np.int64), 0, M.ISIZE_BINS - 1)
        np.add.at(hist, vals, 1)
        if k % 3 == 0:
            xs = rng.choice(vals, n)                                          # from the null itself
        elif k % 3 == 1:
            xs = np.clip(rng.choice(vals, n) + int(rng.integers(-300, 300)), 0, M.ISIZE_BINS - 1)   # shifted
        else:
            xs = rng.integers(0, M.ISIZE_BINS, n)                             # anywhere, 0 and the last bin within reach
        if k == 5:
            xs = np.concatenate([xs, [0, 0, M.ISIZE_BINS - 1]])
        xs = np.asarray(xs, np.int64)
        n = len(xs)
        cum = np.cumsum(hist)
        N = int(cum[-1])
        r = M.row_of(xs, 0, cum)
        ecdf = np.cumsum(np.bincount(xs, minlength=M.ISIZE_BINS))            # n F_n(x) at every integer
        diff = ecdf.astype(object) * N - cum.astype(object) * n              # n N (F_n - F), Python integers
        sup = max(Fraction(int(abs(d)), n * N) for d in diff)
        assert sup == Fraction(max(r[5], r[6]), n * N), k
        assert Fraction(r[5], n * N) == max(Fraction(0), max(Fraction(int(d), n * N) for d in diff))   # D+ is attained at an integer x_i
        assert r[0] == n and r[4] == int(xs.sum())


def run_cli(args, env=None, cwd=None):
    build()
    return subprocess.run([EXE] + args, cwd=cwd, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("env", [{}, {"BDX_FOREGROUND": "1"}])
def test_cli_usage_errors(env, tmp_path):
    cwd = os.path.join(GOLDEN, "chr21")
    out = str(tmp_path / "mini.txt")
    bad = [["--mini-window", "100"], ["--mini-step", "5"], ["--mini-min-pairs", "20"], ["--mini-score", "30"],
           ["--mini", out, "--mini-window", "0"], ["--mini", out, "--mini-window", str(2**30 + 1)], ["--mini", out, "--mini-window", "x"],
           ["--mini", out, "--mini-step", "0"], ["--mini", out, "--mini-step", str(2**30 + 1)], ["--mini", out, "--mini-step", "-3"],
           ["--mini", out, "--mini-min-pairs", "1"], ["--mini", out, "--mini-min-pairs", str(M.MINI_CAP + 1)],
           ["--mini", out, "--mini-score", "-1"], ["--mini", out, "--mini-score", "100000"], ["--mini", out, "--mini-score", "3.5"]]
    for args in bad:
        p = run_cli(args + ["inv_del_bam_config"], env, cwd)
        assert p.returncode == 1 and b"--mini" in p.stderr and p.stdout == b"", (args, p.stderr)
    p = run_cli(["--mini"], env, cwd)
    assert p.returncode == 1
    # no finite positive mean and no --mini-window: before the GPU is touched (the BAM it names does not even exist)
    cfg = tmp_path / "bare.cfg"
    cfg.write_text("readgroup:rg0\tplatform:illumina\tmap:none.bam\treadlen:50.00\tlib:lib0\tnum:10\tlower:0.00\tupper:0.00\tmean:0.00\tstd:0.00\n")
    p = run_cli(["--mini", out, str(cfg)], env, str(tmp_path))
    assert p.returncode == 1 and b"--mini-window" in p.stderr and b"bdx_create" not in p.stderr and p.stdout == b""
    # an unwritable FILE
    p = run_cli(["--mini", str(tmp_path / "no" / "dir" / "f"), "inv_del_bam_config"], env, cwd)
    assert p.returncode == 1 and b"--mini file" in p.stderr and p.stdout == b""
