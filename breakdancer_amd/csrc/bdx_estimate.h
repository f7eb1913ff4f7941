// --estimate: a library's insert-size figures from its histogram, defined ONCE for the library (bdx_estimate_insert_size), the CLI
// (host/estimate.cpp) and the check tool (host/estimate_check_main.cpp).  Host only.
//
// The arithmetic is bam2cfg's (perl/bam2cfg.pl:153-197, restated in host/bam2cfg_main.cpp): mean and standard deviation (n - 1) over all
// observations; every x with !(x > mean_all + 5 sd_all) is kept; mean and sd again over the kept ones; the one-sided deviations around
// that mean over the kept x <= mean (n_minus) and x > mean (n_plus), each with its own n - 1.  The observations arrive as a histogram
// hist[x] = number of observations with value x, 0 <= x < BDX_ISIZE_BINS, so every sum runs bin by bin in ascending x, in double:
// count * x for the means, count * (x - mean)^2 for the deviations.  A deviation over fewer than two observations is 0 (the script
// would divide by zero; such an estimate is not valid anyway).  valid: n_kept >= 100 (bam2cfg's own figure), n_minus >= 2, n_plus >= 2.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/bdx.h"

namespace bdx {

inline void estimate_insert_size(const uint64_t* hist, bdx_insert_estimate* out) {
    bdx_insert_estimate e{};
    // mean and deviation of the bins [0, end) that `keep` lets through
    auto mean_of = [&](int end, uint64_t* n) {
        double sum = 0;
        uint64_t cnt = 0;
        for (int x = 0; x < end; ++x)
            if (hist[x]) { sum += (double)hist[x] * (double)x; cnt += hist[x]; }
        *n = cnt;
        return cnt ? sum / (double)cnt : 0.0;
    };
    auto dev_of = [&](int begin, int end, double mean, uint64_t* n) {
        double sum = 0;
        uint64_t cnt = 0;
        for (int x = begin; x < end; ++x)
            if (hist[x]) { const double d = (double)x - mean; sum += (double)hist[x] * (d * d); cnt += hist[x]; }
        if (n) *n = cnt;
        return cnt >= 2 ? std::sqrt(sum / (double)(cnt - 1)) : 0.0;
    };
    e.mean_all = mean_of(BDX_ISIZE_BINS, &e.n);
    e.sd_all = dev_of(0, BDX_ISIZE_BINS, e.mean_all, nullptr);
    const double cut = e.mean_all + 5 * e.sd_all;
    int kept_end = 0;   // the kept bins are [0, kept_end): x is kept when !(x > cut)
    while (kept_end < BDX_ISIZE_BINS && !((double)kept_end > cut)) ++kept_end;
    e.mean = mean_of(kept_end, &e.n_kept);
    e.sd = dev_of(0, kept_end, e.mean, nullptr);
    int plus_begin = 0;   // x <= mean below it, x > mean from it on
    while (plus_begin < kept_end && !((double)plus_begin > e.mean)) ++plus_begin;
    e.sd_minus = dev_of(0, plus_begin, e.mean, &e.n_minus);
    e.sd_plus = dev_of(plus_begin, kept_end, e.mean, &e.n_plus);
    e.valid = e.n_kept >= 100 && e.n_minus >= 2 && e.n_plus >= 2 ? 1 : 0;
    *out = e;
}

}  // namespace bdx
