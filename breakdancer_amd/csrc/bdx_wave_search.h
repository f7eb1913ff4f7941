// The 64-ary ballot search of the kernels that answer queries over the resident store (K8, KS, KI: kq_queries.hip), which reach it through
// the window walk of bdx_window.h.
// Pinned on its own, against bisect_left, by tests/test_gpu_prims.py (harness: tests/prims/prims.hip).
#pragma once
#include "bdx_dev.h"

namespace bdx {

// First index in [0, n) whose (tid, pos) is not below (t, p), in a store sorted by (tid, pos); the answer is wave-uniform.  The 64
// lanes probe 64 evenly spaced records and one ballot says how many lie in front: ~5 rounds of one load each for 2^27 records; the last
// round (64 records or fewer left) probes every one of them.  Every lane of the wave has to call it.
static __device__ uint64_t wave_lower_bound(const int32_t* __restrict__ tid, const int32_t* __restrict__ pos, uint64_t n, int32_t t, int64_t p) {
    const int lane = lane_id();
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t len = hi - lo;
        const bool last = len <= 64;
        // (len > 64: lane l probes lo + len * (l + 1) / 65, strictly increasing and inside [lo, hi))
        const uint64_t idx = last ? lo + (uint64_t)lane : lo + len * (uint64_t)(lane + 1) / 65;
        bool below = false;
        if (idx < hi) {
            const int32_t ti = tid[idx];
            below = ti < t || (ti == t && (int64_t)pos[idx] < p);
        }
        const int c = popc64(ballot64(below));
        if (last) return lo + (uint64_t)c;
        const uint64_t lo0 = lo;
        if (c > 0) lo = lo0 + len * (uint64_t)c / 65 + 1;
        if (c < 64) hi = lo0 + len * (uint64_t)(c + 1) / 65;
    }
    return lo;
}

}  // namespace bdx
