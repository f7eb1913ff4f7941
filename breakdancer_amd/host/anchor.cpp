#include "anchor.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <ostream>
#include <stdexcept>
#include <string>

namespace bdhost {

int64_t anchor_default_window(const std::vector<bdx_lib>& libs) {
    double best = 0;
    for (const bdx_lib& l : libs) {
        const double u = (double)l.uppercutoff;
        if (std::isfinite(u)) best = std::max(best, 2.0 * std::ceil(u));
    }
    if (!(best >= 1)) throw std::runtime_error("--anchor: no library has a finite positive uppercutoff, give --anchor-window");
    return (int64_t)std::min(best, 1073741824.0);
}

namespace {

bool better(const bdx_anchor_split& a, const bdx_anchor_split& b) {
    const uint64_t ua = (uint64_t)a.u_left + a.u_right, ub = (uint64_t)b.u_left + b.u_right;
    if (ua != ub) return ua > ub;
    const uint64_t na = (uint64_t)a.n_left + a.n_right, nb = (uint64_t)b.n_left + b.n_right;
    if (na != nb) return na > nb;
    return a.split < b.split;
}

}  // namespace

std::vector<AnchorCall> anchor_merge(std::vector<AnchorCall> called) {
    // (a call has n_left > 0, so last_left == split - 1: the order by split is the order by the intervals' left ends, and one sweep that
    // keeps the group's largest right end finds the connected groups)
    std::stable_sort(called.begin(), called.end(), [](const AnchorCall& a, const AnchorCall& b) {
        if (a.seq != b.seq) return a.seq < b.seq;
        if (a.row.split != b.row.split) return a.row.split < b.row.split;
        return a.row.last_left < b.row.last_left;
    });
    std::vector<AnchorCall> out;
    int64_t reach = -1;   // the group's largest first_right
    for (const AnchorCall& c : called) {
        if (!out.empty() && out.back().seq == c.seq && (int64_t)c.row.last_left <= reach) {
            AnchorCall& g = out.back();
            g.windows += c.windows;
            if (better(c.row, g.row)) g.row = c.row;
            reach = std::max<int64_t>(reach, c.row.first_right);
        } else {
            out.push_back(c);
            reach = c.row.first_right;
        }
    }
    // (the rows kept of two groups keep the groups' order: each lies inside its group's span, and the spans are disjoint)
    return out;
}

void anchor_write_table(std::ostream& out, const std::vector<AnchorCall>& calls, const std::vector<std::string>& names) {
    out << "#Chr\tPos1\tPos2\tType\tLeft\tRight\tDistinctLeft\tDistinctRight\tLowQual\tWindows\n";
    char buf[256];
    for (const AnchorCall& c : calls) {
        const bdx_anchor_split& r = c.row;
        snprintf(buf, sizeof buf, "\t%lld\t%lld\tINS\t%u\t%u\t%u\t%u\t%u\t%llu\n", (long long)r.last_left + 1, (long long)r.first_right + 1, r.n_left, r.n_right,
                 r.u_left, r.u_right, r.n_low, (unsigned long long)c.windows);
        out << ((size_t)c.seq < names.size() ? names[c.seq] : std::to_string(c.seq)) << buf;
    }
}

}  // namespace bdhost
