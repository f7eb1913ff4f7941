"""Generates tests/golden/poisson_edge_vectors.json with mpmath (60 digits): log P(X > k; lambda) of a Poisson variable at the
points where K5 (csrc/bdx_poisson.h) changes behaviour -- the series switch at lambda = k + 2, the lane / wave switch at 4096,
k = 0, lambda <= 0, the 1e-10 floor of lambda, the underflow of p -- plus the 168 points of poisson_vectors.json, a seeded
random sample and points beyond the domain for which 1e-10 is asserted.  Run here once; the vectors are committed.

Every lambda is stored as float.hex() of the double the kernel receives and the reference is evaluated at exactly that double.
reference: the pmf summed directly above k; every row is cross-checked (1e-30 relative on p) by a second evaluation and a row
without an agreeing one stops the generator.  Where p > 1/2, log p is log1p(-sum of the pmf up to k), so that a log p of
-1e-300 is recorded as that and not as the rounding of the direct sum; that sum has a cross-check of its own (check_head).
The two groups of 600 seeded random draws give 1,160 rows: 40 draws of the second group are clamped to lambda = 1e-10 with
a k that an earlier one has, and a (family, lambda, k) is kept once.  No test imports mpmath."""
import json
import math
import os
import random
import sys

import mpmath as mp

mp.mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))
LOG_MIN_NORMAL = mp.mpf(-1022) * mp.log(2)  # p >= 2^-1022: a normal double
LOG_HALF_DENORMAL = mp.mpf(-1075) * mp.log(2)  # p < 2^-1075 rounds to zero


def up(x):
    return math.nextafter(x, math.inf)


def down(x):
    return math.nextafter(x, -math.inf)


def pmf(lam, j):
    return mp.exp(-lam + j * mp.log(lam) - mp.loggamma(j + 1))


@mp.workdps(75)  # guard digits: up to 1e6 rounded additions
def tail_direct(lam, k):
    """sum of the pmf above k: first term, then t * lambda / j, until j > lambda and the term is below 1e-70 of the sum"""
    j = k + 1
    t = pmf(lam, j)
    s = t
    eps = mp.mpf("1e-70")
    while True:
        j += 1
        t = t * lam / j
        s += t
        if j > lam and t < eps * s:
            return s


def head(lam, k):
    """sum of the pmf up to k, summed downwards from k"""
    t = pmf(lam, k)
    s = t
    for j in range(k, 0, -1):
        t = t * j / lam
        s += t
        if j < lam and t < mp.mpf("1e-90") * s:
            break
    return s


def second_evaluation(lam, k, p):
    """(name, value) of the cross-check: the regularised lower incomplete gamma function where mpmath's series converges,
    else the complement of the head where p > 1e-20"""
    try:
        return "gammainc", mp.gammainc(k + 1, 0, lam, regularized=True)
    except mp.libmp.NoConvergence:
        pass
    if p > mp.mpf("1e-20"):
        with mp.workdps(90):
            return "complement", 1 - head(lam, k)
    return None, None


def check_head(lam, k, x, h, p, stats):
    """the head has a second evaluation of its own (1e-30 relative): the regularised upper incomplete gamma function where
    mpmath's evaluation converges, else 1 - the direct sum -- which says no more than `below 1e-65` of a head that small"""
    try:
        how, q = "head: gammainc", mp.gammainc(k + 1, x, mp.inf, regularized=True)
        ok = abs(q - h) <= mp.mpf("1e-30") * h
    except mp.libmp.NoConvergence:
        how, q = "head: 1 - direct sum", 1 - p
        ok = abs(q - h) <= mp.mpf("1e-30") * h + mp.mpf("1e-65")
    if not ok:
        sys.exit("no agreeing second evaluation of the head for lambda=%r k=%d (%s): %s vs %s" % (lam, k, how, mp.nstr(h, 40), mp.nstr(q, 40)))
    stats[how] = stats.get(how, 0) + 1


def make_row(family, lam, k, stats):
    lam = float(lam)
    k = int(k)
    row = {"family": family, "lambda_hex": lam.hex(), "k": k}
    if not lam > 0.0:  # cdf complement of a zero-mean Poisson is 0 (poisson_close's first line)
        row.update(logp="-inf", band="zero")
        return row
    x = mp.mpf(lam)  # exactly the double
    p = tail_direct(x, k)
    how, q = second_evaluation(x, k, p)
    if how is None or abs(q - p) > mp.mpf("1e-30") * p:
        sys.exit("no agreeing second evaluation for lambda=%r k=%d (%s): %s vs %s" % (lam, k, how, mp.nstr(p, 40), q and mp.nstr(q, 40)))
    stats[how] = stats.get(how, 0) + 1
    lg = mp.log(p)
    if p > 0.5:  # 1 - p may be far below the 1e-70 the direct sum stops at: log p from the head, which keeps its relative precision
        with mp.workdps(90):
            h = head(x, k)
            lg = mp.log1p(-h)
        check_head(lam, k, x, h, p, stats)
    band = "normal" if lg >= LOG_MIN_NORMAL else "denormal" if lg >= LOG_HALF_DENORMAL else "zero"
    row.update(logp=mp.nstr(lg, 25), band=band)
    return row


def log_tail_estimate(lam, k):
    """log of the first term above k: within a fraction of a nat of log p for lambda << k, enough to find the band edges"""
    return float(mp.log(pmf(mp.mpf(lam), k + 1)))


def underflow_points():
    """k walked across the edges of the denormal band of each lambda (three normal rows, the whole band, three zero rows),
    and two terms of the wave series that underflow"""
    out = []
    for lam in [0.05, 1.0, 47.3]:
        k = int(lam) + 1
        while log_tail_estimate(lam, k) > float(LOG_MIN_NORMAL) + 1.0:
            k += 1
        first = k - 4
        while log_tail_estimate(lam, k) > float(LOG_HALF_DENORMAL) - 1.0:
            k += 1
        for kk in range(first, k + 4):
            out.append(("underflow", lam, kk))
    out += [("underflow", 0.05, 5000), ("underflow", 1.0, 4500)]
    return out


def points():
    """(family, lambda, k) of every row, in file order"""
    out = []
    # the series switch lambda < (k + 1) + 1, either side of it and around the mode
    for k in [1, 2, 3, 5, 8, 21, 63, 64, 65, 127, 128, 255, 256, 1000, 2047, 4095, 4096, 4097, 6000, 8190, 8191, 8192]:
        r = math.sqrt(k)
        for lam in [down(k + 2.0), k + 2.0, up(k + 2.0), k + 1.0, float(k), k - r, k + 3 + r, k + 3 + 4 * r, max(0.3, k - 4 * r),
                    0.5 * k + 0.1, min(8192.0, 2.0 * k + 3)]:
            out.append(("switch", lam, k))
    # the lane / wave switch k > 4096 || lambda > 4096
    for k in [4095, 4096, 4097]:
        for lam in [1.0, 100.0, 3000.0, 4095.5, 4096.0, up(4096.0), 5000.0]:
            out.append(("limit", lam, k))
    for lam in [4096.0, up(4096.0), 4097.0]:
        for k in [1, 50, 3000, 4000, 4096, 4200, 5000]:
            out.append(("limit", lam, k))
    # k = 0 (closed form) and lambda <= 0
    for lam in [5e-324, 1e-300, 1e-10, 1e-6, 0.5, 1.0, 30.0, 700.0, 745.0, 800.0, 1e4]:
        out.append(("k0", lam, 0))
    for lam in [0.0, -1.0]:
        for k in [0, 3]:
            out.append(("k0", lam, k))
    # the floor the callers put under lambda
    for k in [1, 2, 5, 20, 30]:
        for lam in [1e-10, up(1e-10), 1.0000000001e-10, 1e-9, 1e-8, 3e-7]:
            out.append(("floor", lam, k))
    # the 168 points of poisson_vectors.json
    for r in json.load(open(os.path.join(HERE, "poisson_vectors.json")))["poisson"]:
        out.append(("grid", float(r["lambda"]), r["k"]))
    # seeded random points: log-uniform, then around the mode
    rng = random.Random(20261017)
    for _ in range(600):
        k = int(math.floor(2.0 ** rng.uniform(0, 13)))
        out.append(("random", 2.0 ** rng.uniform(-20, 13), k))
    for _ in range(600):
        k = int(math.floor(2.0 ** rng.uniform(0, 13)))
        out.append(("random", min(8192.0, max(1e-10, k + 3.0 * rng.gauss(0, 1) * math.sqrt(k + 1))), k))
    out += underflow_points()
    # beyond the domain for which 1e-10 is asserted
    for n in [10000, 16384, 32768, 100000, 300000, 1 << 20]:
        for f in [0.9, 0.99, 1.0, 1.01, 1.1]:
            out.append(("outer", f * n, n))
    out += [("outer", 10000.0, 1), ("outer", 10000.0, 10500), ("outer", 1e5, 5), ("outer", 3.0, 1 << 20)]
    return out


def main():
    stats = {}
    rows, seen = [], set()
    pts = points()
    for i, (family, lam, k) in enumerate(pts):
        key = (family, float(lam).hex(), k)
        if key in seen:
            continue
        seen.add(key)
        rows.append(make_row(family, lam, k, stats))
        if i % 100 == 0:
            print(i, len(pts), file=sys.stderr)
    under = [r for r in rows if r["family"] == "underflow"]
    for lam in [0.05, 1.0, 47.3]:
        bands = [r["band"] for r in under if r["lambda_hex"] == lam.hex() and r["k"] < 4096]
        assert bands == sorted(bands, key=["normal", "denormal", "zero"].index), bands  # k ascending: one edge after the other
        assert bands.count("normal") >= 1 and bands.count("denormal") >= 1 and bands.count("zero") >= 1, bands
    assert sum(r["band"] == "denormal" for r in under) >= 6 and sum(r["band"] == "zero" for r in under) >= 6
    assert all(r["band"] == "zero" for r in under if r["k"] > 4096)
    with open(os.path.join(HERE, "poisson_edge_vectors.json"), "w") as f:
        f.write('{"poisson": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
    print(len(rows), "rows; second evaluations:", stats)


if __name__ == "__main__":
    main()
