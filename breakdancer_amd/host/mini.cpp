#include "mini.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <ostream>
#include <stdexcept>
#include <string>

#include "../csrc/bdx_mini.h"

namespace bdhost {

int64_t mini_mean_window(const std::vector<bdx_lib>& libs) {
    double best = 0;
    for (const bdx_lib& l : libs) {
        const double m = (double)l.mean_insertsize;
        if (std::isfinite(m) && m > 0) best = std::max(best, std::ceil(m));
    }
    if (!(best > 0)) throw std::runtime_error("--mini: no library has a finite positive mean insert size, give --mini-window");
    return (int64_t)std::min(best, 1073741824.0);
}

MiniNull mini_null(const uint64_t* hist, size_t nlibs) {
    MiniNull n;
    n.N.assign(nlibs, 0); n.mu.assign(nlibs, 0.0); n.usable.assign(nlibs, 0);
    for (size_t l = 0; l < nlibs; ++l) {
        const uint64_t* h = hist + l * (size_t)BDX_ISIZE_BINS;
        double sum = 0;
        uint64_t cnt = 0;
        for (int x = 0; x < BDX_ISIZE_BINS; ++x)
            if (h[x]) { sum += (double)h[x] * (double)x; cnt += h[x]; }
        n.N[l] = cnt;
        n.mu[l] = cnt ? sum / (double)cnt : 0.0;
        n.usable[l] = cnt >= kMiniUsable;
    }
    return n;
}

MiniWindow mini_window(const bdx_insert_shift* rows, const MiniNull& null, int min_pairs) {
    MiniWindow w;
    double moved = 0, best = -1;
    for (size_t l = 0; l < null.N.size(); ++l) {
        const bdx_insert_shift& r = rows[l];
        if (r.saturated) w.saturated = true;
        if (!null.usable[l] || r.saturated || r.n < (uint32_t)min_pairs) continue;
        double sc, d;
        bdx::insert_shift_score(r, null.N[l], &sc, &d);
        w.scoring = true;
        w.score += sc;
        w.pairs += r.n;
        moved += (double)r.sum - (double)r.n * null.mu[l];
        if (sc > best) { best = sc; w.D = d; }
    }
    if (w.scoring) {
        w.shift = moved / (double)w.pairs;
        w.del = w.shift > 0;
    }
    return w;
}

int mini_default_threshold(uint64_t scoring_windows) {
    // 20 + ceil(10 log10 W).  With 10^d <= W < 10^(d + 1), found in integers: W == 10^d gives 10 d exactly -- the only W at which a tenth
    // of a decade is met exactly (10^(r / 10) is irrational for r = 1 .. 9), so the one place where a rounding error in pow or log10 could
    // move the result is decided without floating point.  Otherwise W / 10^d lies strictly inside (1, 10) and strictly between two of the
    // irrational steps: the smallest r in 1 .. 10 with 10^(r / 10) >= W / 10^d, in long double.
    const uint64_t W = scoring_windows;
    if (W <= 1) return 20;
    int d = 0;
    uint64_t p10 = 1;
    while (W / p10 >= 10) { p10 *= 10; ++d; }
    if (W == p10) return 20 + 10 * d;
    const long double m = (long double)W / (long double)p10;
    int r = 1;
    while (r < 10 && std::pow(10.0L, (long double)r / 10.0L) < m) ++r;
    return 20 + 10 * d + r;
}

std::vector<MiniCall> mini_merge(const std::vector<MiniKept>& kept, int threshold, const MiniParams& p, const std::vector<uint32_t>& lengths) {
    std::vector<MiniCall> calls;
    const MiniKept* prev = nullptr;
    for (const MiniKept& k : kept) {
        if (!k.w.scoring || !(k.w.score >= (double)threshold)) continue;
        const int64_t len = (size_t)k.seq < lengths.size() ? (int64_t)lengths[k.seq] : 0;
        const int64_t end = std::min<int64_t>(k.j * p.step + p.window, len);
        if (prev && prev->seq == k.seq && prev->j + 1 == k.j && prev->w.del == k.w.del) {
            MiniCall& c = calls.back();
            c.end = end;
            ++c.windows;
            if (k.w.score > c.score) { c.score = k.w.score; c.shift = k.w.shift; c.D = k.w.D; c.pairs = k.w.pairs; }
        } else {
            calls.push_back(MiniCall{k.seq, k.j * p.step + 1, end, k.w.del, k.w.shift, k.w.score, k.w.D, k.w.pairs, 1});
        }
        prev = &k;
    }
    return calls;
}

void mini_write_table(std::ostream& out, const std::vector<MiniCall>& calls, const std::vector<std::string>& names) {
    out << "#Chr\tBeg\tEnd\tType\tShift\tScore\tPairs\tD\tWindows\n";
    char buf[256];
    for (const MiniCall& c : calls) {
        const double r = std::floor(c.score + 0.5);
        snprintf(buf, sizeof buf, "\t%lld\t%lld\t%s\t%.1f\t%lld\t%llu\t%.3f\t%llu\n", (long long)c.beg, (long long)c.end, c.del ? "DEL" : "INS", c.shift,
                 (long long)(r > 99999.0 ? 99999.0 : r), (unsigned long long)c.pairs, c.D, (unsigned long long)c.windows);
        out << ((size_t)c.seq < names.size() ? names[c.seq] : std::to_string(c.seq)) << buf;
    }
}

}  // namespace bdhost
