// --exclude: the region mask of the reader filter, defined ONCE for the device (kb_records.hip, kx_exclude.hip) and the host readers
// (host/column_reader.cpp, host/producer.cpp).  No counterpart in the reference, whose only lever is -x: a region dropped after its reads
// have been counted.
//
// The mask is a set of half-open, 0-based intervals [beg, end) per reference sequence, sorted and merged (touching ones too), laid out as
//   first[ntids + 1]   the slice of sequence t is [first[t], first[t + 1])
//   beg[], end[]       ascending and disjoint within a slice
// A record that passed the reader filter is dropped when its own start (tid, pos) or its mate's (mtid, mpos) lies in an interval.  Only
// the coordinates the record itself carries are looked at -- no CIGAR end: the mate's is not known to the record -- so both mates of a
// consistent pair go together.  A tid / mtid below 0, beyond the mask's sequences or with an empty slice is never dropped.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BDX_EXCLUDE_HD __host__ __device__
#else
#define BDX_EXCLUDE_HD
#endif

namespace bdx {

constexpr size_t kMaxExcludeIntervals = (size_t)1 << 24;   // merged intervals (a 128 MiB table)
constexpr int64_t kMaxExcludeTids = (int64_t)1 << 24;       // sequences the table's first[] spans

struct ExcludeMask {
    const uint32_t* first;
    const int32_t* beg;
    const int32_t* end;
    int32_t ntids;   // 0: no mask
};

// upper bound of pos among the slice's begs, then pos < end of the interval in front of it
BDX_EXCLUDE_HD inline bool exclude_hit(const ExcludeMask& m, int32_t tid, int32_t pos) {
    if (tid < 0 || tid >= m.ntids) return false;
    const uint32_t lo0 = m.first[tid];
    uint32_t lo = lo0, hi = m.first[tid + 1];
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (m.beg[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    return lo > lo0 && pos < m.end[lo - 1];
}

BDX_EXCLUDE_HD inline bool exclude_record(const ExcludeMask& m, int32_t tid, int32_t pos, int32_t mtid, int32_t mpos) {
    return exclude_hit(m, tid, pos) || exclude_hit(m, mtid, mpos);
}

// The table of a list of intervals in any order (they may overlap or touch; beg == end is empty and ignored).  Interval: anything with
// int32 members tid, beg, end; the caller has checked tid >= 0 and 0 <= beg <= end.  Returns the number of merged intervals.
template <class Interval>
inline size_t exclude_build(const Interval* iv, size_t n, std::vector<uint32_t>& first, std::vector<int32_t>& beg, std::vector<int32_t>& end) {
    struct Key { int32_t tid, beg, end; };
    std::vector<Key> k;
    k.reserve(n);
    int32_t ntids = 0;
    for (size_t i = 0; i < n; ++i) {
        if (iv[i].beg == iv[i].end) continue;
        k.push_back(Key{iv[i].tid, iv[i].beg, iv[i].end});
        ntids = std::max(ntids, iv[i].tid + 1);
    }
    std::sort(k.begin(), k.end(), [](const Key& a, const Key& b) { return a.tid != b.tid ? a.tid < b.tid : a.beg != b.beg ? a.beg < b.beg : a.end < b.end; });
    first.assign(k.empty() ? 0 : (size_t)ntids + 1, 0);
    beg.clear();
    end.clear();
    std::vector<int32_t> tid_of;
    for (const Key& x : k) {
        if (!beg.empty() && tid_of.back() == x.tid && x.beg <= end.back()) {
            end.back() = std::max(end.back(), x.end);
            continue;
        }
        tid_of.push_back(x.tid);
        beg.push_back(x.beg);
        end.push_back(x.end);
    }
    for (int32_t t : tid_of) ++first[(size_t)t + 1];
    for (size_t t = 1; t < first.size(); ++t) first[t] += first[t - 1];
    return beg.size();
}

}  // namespace bdx
