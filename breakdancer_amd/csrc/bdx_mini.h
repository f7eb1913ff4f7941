// --mini: the score of one row of bdx_window_insert_shift, defined ONCE for the library (bdx_insert_shift_score), the CLI (host/mini.cpp)
// and the check tool (host/mini_check_main.cpp).  Host only.
//
// A row's t_plus and t_minus are n N times the one-sided Kolmogorov-Smirnov distances between the window's n observations and the null of
// N (include/bdx.h, ROW): D = max(t_plus, t_minus) / (n N), the two factors converted to double one by one.  With Stephens' finite-n
// correction lambda = (sqrt(n) + 0.12 + 0.11 / sqrt(n)) D the asymptotic Kolmogorov tail is p = 2 sum_{j >= 1} (-1)^(j-1) exp(-2 j^2 lambda^2).
// exp(-2 lambda^2) leaves the double range near lambda = 19, so the leading factor is taken out of the sum and only its logarithm is used:
//   ln p = ln 2 - 2 lambda^2 + ln S,   S = sum_{j >= 1} (-1)^(j-1) exp(-2 (j^2 - 1) lambda^2) = 1 - exp(-6 lambda^2) + exp(-16 lambda^2) - ...
// The terms are added in ascending j, and the first one below 1e-17 is the last one added.  Below lambda = 0.4 the series converges slowly and
// p is above 0.99: score 0.  score = -10 ln p / ln 10 (Phred).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/bdx.h"

namespace bdx {

inline void insert_shift_score(const bdx_insert_shift& r, uint64_t N, double* score, double* D) {
    double sc = 0, d = 0;
    if (r.n && N && !r.saturated) {
        const int64_t t = r.t_plus > r.t_minus ? r.t_plus : r.t_minus;
        d = (double)t / ((double)r.n * (double)N);
        const double rn = std::sqrt((double)r.n);
        const double lam = (rn + 0.12 + 0.11 / rn) * d;
        if (!(lam < 0.4)) {
            const double l2 = lam * lam;
            double S = 0, sign = 1;
            for (int j = 1;; ++j) {
                const double term = std::exp(-2.0 * ((double)j * (double)j - 1.0) * l2);
                S += sign * term;
                sign = -sign;
                if (term < 1e-17) break;
            }
            const double lnp = std::log(2.0) - 2.0 * l2 + std::log(S);
            sc = -10.0 * lnp / std::log(10.0);
        }
    }
    if (score) *score = sc;
    if (D) *D = d;
}

}  // namespace bdx
