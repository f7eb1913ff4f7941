"""--estimate's rule restated in plain Python / numpy, and the histograms the tests hold the product to (tests/test_estimate.py on the
CPU, tests/test_gpu_estimate.py on the GPU).

restate()       bdx_estimate_insert_size (csrc/bdx_estimate.h) with the same sums in the same order: bin by bin in ascending x, in double,
                count * x for the means and count * (x - mean)^2 for the deviations; a deviation over fewer than two observations is 0.
observations()  bdx_insert_size_histogram's rule over a structure of arrays, brute force.
run_libraries() the CLI's step from an estimate to the four values a run uses: %.2f text read back as float32.
"""
import math

import numpy as np

BINS = 32768


def restate(hist):
    """the estimate of one library from hist[BINS] (any integer sequence), as a dict of Python ints and floats"""
    hist = np.asarray(hist)
    xs = [int(x) for x in np.nonzero(hist)[0]]          # (ascending; an empty bin adds nothing in the product either)
    cs = [int(hist[x]) for x in xs]

    def mean_of(pairs):
        s, n = 0.0, 0
        for x, c in pairs:
            s += float(c) * float(x)
            n += c
        return (s / float(n) if n else 0.0), n

    def dev_of(pairs, mean):
        s, n = 0.0, 0
        for x, c in pairs:
            d = float(x) - mean
            s += float(c) * (d * d)
            n += c
        return (math.sqrt(s / float(n - 1)) if n >= 2 else 0.0), n

    allp = list(zip(xs, cs))
    mean_all, n = mean_of(allp)
    sd_all, _ = dev_of(allp, mean_all)
    cut = mean_all + 5 * sd_all
    kept = [(x, c) for x, c in allp if not (float(x) > cut)]
    mean, n_kept = mean_of(kept)
    sd, _ = dev_of(kept, mean)
    sd_minus, n_minus = dev_of([(x, c) for x, c in kept if not (float(x) > mean)], mean)
    sd_plus, n_plus = dev_of([(x, c) for x, c in kept if float(x) > mean], mean)
    return dict(mean_all=mean_all, sd_all=sd_all, mean=mean, sd=sd, sd_minus=sd_minus, sd_plus=sd_plus, n=n, n_kept=n_kept,
                n_minus=n_minus, n_plus=n_plus, valid=int(n_kept >= 100 and n_minus >= 2 and n_plus >= 2), cut=cut)


def two_decimals(v):
    return "%.2f" % v


def run_libraries(est, c=3):
    """(mean, std, upper, lower) of a valid estimate as float32 values, and the four %.2f texts (lower, upper, mean, std)"""
    upper = est["mean"] + c * est["sd_plus"]
    lower = max(0.0, est["mean"] - c * est["sd_minus"])
    text = dict(lower=two_decimals(lower), upper=two_decimals(upper), mean=two_decimals(est["mean"]), std=two_decimals(est["sd"]))
    vals = {k: np.float32(v) for k, v in text.items()}
    return vals, text, dict(lower=lower, upper=upper, mean=est["mean"], std=est["sd"])


def preconditions_hold(est, c=3):
    """Generated inputs stay clear of the two places where one ulp decides: the 5-sd threshold further than 1e-6 from an integer, and no
    printed value within 1e-6 of a %.2f rounding boundary."""
    if abs(est["cut"] - round(est["cut"])) <= 1e-6:
        return False
    if est["valid"]:
        for v in run_libraries(est, c)[2].values():
            f = (v * 100.0) % 1.0
            if abs(f - 0.5) <= 1e-4:          # (1e-6 of the value is 1e-4 of its hundredths)
                return False
    return True


def hist_of(values):
    h = np.zeros(BINS, dtype=np.uint64)
    v = np.asarray(values, dtype=np.int64)
    np.add.at(h, v[(v >= 0) & (v < BINS)], 1)
    return h


def hand_cases():
    """name -> hist[BINS]"""
    cases = {}
    cases["empty"] = hist_of([])
    cases["one"] = hist_of([300])
    cases["all_equal"] = hist_of([250] * 500)
    cases["kept_99"] = hist_of([400] * 50 + [410] * 49)
    cases["kept_100"] = hist_of([400] * 50 + [410] * 50)
    # (a single observation above the mean survives the trim only in a small library: beside n equal values it lies sqrt(n) deviations out)
    cases["n_plus_1"] = hist_of([300] * 18 + [200] + [400])
    cases["outlier_trimmed"] = hist_of([300 + (i % 41) for i in range(2000)] + [30000])
    cases["bin_edges"] = hist_of([0] * 120 + [BINS - 1] * 130)
    cases["bimodal"] = hist_of([200 + (i % 31) for i in range(3000)] + [2500 + (i % 301) for i in range(1500)])
    return cases


def generated_cases(seed=7, count=24):
    """roughly normal libraries of different sizes, means and spreads, some with a tail; only those the preconditions let through"""
    rng = np.random.default_rng(seed)
    out = {}
    k = 0
    while len(out) < count:
        k += 1
        n = int(rng.integers(50, 40000))
        mean, sd = float(rng.uniform(150, 6000)), float(rng.uniform(5, 400))
        v = np.rint(rng.normal(mean, sd, n)).astype(np.int64)
        if rng.random() < 0.5:
            v = np.concatenate([v, rng.integers(0, BINS, int(rng.integers(1, 40)))])
        h = hist_of(np.clip(v, 0, BINS - 1))
        if preconditions_hold(restate(h)):
            out["generated_%d" % k] = h
    return out


def observations(soa, nlibs, min_mapq):
    """(hist[nlibs][BINS], n_over[nlibs]) of bdx_insert_size_histogram's rule over the arrays of soa, brute force.  min_mapq: the
    libraries' resolved minima; soa['lib'] is ignored with one library."""
    flag = np.asarray(soa["flag"]).astype(np.int64)
    isize = np.asarray(soa["isize"]).astype(np.int64)
    lib = np.zeros(len(flag), dtype=np.int64) if nlibs == 1 else np.asarray(soa["lib"]).astype(np.int64)
    lib = np.where(lib < nlibs, lib, 0)
    minq = np.asarray(min_mapq, dtype=np.int64)[lib]
    obs = ((flag & 0x1) != 0) & ((flag & (0x400 | 0x4 | 0x8)) == 0) & (np.asarray(soa["mtid"]) == np.asarray(soa["tid"])) & \
          ((flag & 0x2) != 0) & (isize >= 0) & (np.asarray(soa["mapq"]).astype(np.int64) > minq)
    hist = np.zeros((nlibs, BINS), dtype=np.uint64)
    over = np.zeros(nlibs, dtype=np.uint64)
    inb = obs & (isize < BINS)
    np.add.at(hist, (lib[inb], isize[inb]), 1)
    np.add.at(over, lib[obs & (isize >= BINS)], 1)
    return hist, over
