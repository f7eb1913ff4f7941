// KI -- breakpoint intervals of given SV sites from their supporting pairs (bdx_site_breakpoint_bounds; CIPOS / CIEND of the CLI's --ci).
// No counterpart in the reference, whose table gives a call's position and nothing about how far the breakpoint may lie from it.
//
// The records that count for a site are KS's (ks_sites.hip; the rule is in include/bdx.h), all keys pooled.  Each gives one observation
// per end: (x, reverse, U) with x the 0-based start of the read on that end, reverse its strand bit (inverted with -l) and U its
// library's insert-size bound.  The read lies wholly on one side of the breakpoint its fragment crosses and the fragment reaches no
// further than U from the read's start: with P = x + 1 a forward read bounds the breakpoint to [P, P + U], a reverse read to [P - U, P].
// lo = the maximum of the lower bounds, hi = the minimum of the upper bounds, per end, clamped to [1, 2^31 - 1] at the end; n == 0: all 0.
// A record that matches the forward route (near pos1, mate near pos2) gives (pos, 0x10) to end 1 and (mpos, 0x20) to end 2; one that
// matches the reverse route only gives (mpos, 0x20) to end 1 and (pos, 0x10) to end 2.
//
// The sibling of KS: one wavefront per site, the window's first record by the 64-ary ballot search (bdx_wave_search.h), then the lanes
// stride the window 64 records at a time until a record lies behind it; the union of the two windows is scanned once when they
// overlap.  Where it differs: every lane keeps four running 64-bit extrema and a count, one xor-shuffle reduction closes the site, and
// lane 0 writes the 20-byte result.  No LDS.  All arithmetic on positions is 64-bit: window and U may be 2^30 and positions 2^31 - 1.
#include <hip/hip_runtime.h>

#include "../../include/bdx.h"
#include "bdx_dev.h"
#include "bdx_shard.h"
#include "bdx_wave_search.h"

namespace bdx {

static_assert(sizeof(KiBounds) == sizeof(bdx_site_bounds) && sizeof(KiBounds) == 20, "KiBounds is bdx_site_bounds");

namespace {

constexpr int kKiWaves = 4;
constexpr int64_t kKiNone = (int64_t)1 << 62;   // (beyond every bound: |P| < 2^31, U <= 2^30)

__device__ __forceinline__ bool ki_near(int32_t t, int64_t s, int32_t T, int64_t P, int64_t w) {
    const int64_t d = s + 1 - P;
    return t == T && d <= w && -d <= w;
}

__device__ __forceinline__ int64_t ki_clamp(int64_t v) { return v < 1 ? 1 : (v > 2147483647ll ? 2147483647ll : v); }

__global__ __launch_bounds__(kKiWaves * 64) void ki_bounds_kernel(KiParams p) {
    const int lane = lane_id();
    const uint32_t q = blockIdx.x * kKiWaves + (uint32_t)wave_id();
    if (q >= p.nq) return;   // (wave-uniform; the kernel has no barrier)
    int64_t lo1 = -kKiNone, hi1 = kKiNone, lo2 = -kKiNone, hi2 = kKiNone;
    uint32_t cnt = 0;
    if (p.n) {
        const KsSite st = p.sites[q];
        const int32_t t1 = st.tid1, t2 = st.tid2;
        const int64_t p1 = st.pos1, p2 = st.pos2, win = p.window;
        const uint32_t mask = st.flag_mask;
        const bool many = p.nlibs > 1;
        // read-start windows [p1 - 1 - win, p1 - 1 + win] and [p2 - 1 - win, p2 - 1 + win]: one scan over their union when they overlap
        const bool overlap = t1 == t2 && p2 - p1 <= 2 * win;
        const int64_t wlo = p1 - 1 - win, whi = (overlap ? p2 : p1) - 1 + win;
        for (uint64_t base = wave_lower_bound(p.tid, p.pos, p.n, t1, wlo);; base += 64) {
            const uint64_t i = base + (uint64_t)lane;
            bool in = i < p.n;
            int64_t s = 0;
            if (in) {
                s = p.pos[i];
                in = p.tid[i] == t1 && s <= whi;
            }
            const uint64_t m_in = ballot64(in);
            if (in) {
                const uint32_t c = p.cls[i];
                if ((c & BDX_CLS_PASS) && ((mask >> BDX_CLS_FLAG(c)) & 1u)) {
                    const int32_t mt = p.mtid[i];
                    const int64_t ms = p.mpos[i];
                    const uint32_t fl = p.flag[i];
                    // the pair's lower mate (the record's tid is t1 here)
                    const bool lower = t1 < mt || (t1 == mt && (s < ms || (s == ms && (fl & 0x40))));
                    const bool fwd = ki_near(t1, s, t1, p1, win) && ki_near(mt, ms, t2, p2, win);
                    const bool rev = overlap && ki_near(t1, s, t2, p2, win) && ki_near(mt, ms, t1, p1, win);
                    if (lower && (fwd || rev)) {
                        int64_t U = p.u0;
                        if (many) {
                            uint32_t l = p.lib[i];
                            l = l < (uint32_t)p.nlibs ? l : 0u;   // (an index out of range is library 0, like everywhere in the store)
                            U = p.utab[l];
                        }
                        const bool r_own = ((fl & 0x10) != 0) != (p.long_insert != 0), r_mate = ((fl & 0x20) != 0) != (p.long_insert != 0);
                        // (a record matching both routes is taken by the forward one)
                        const int64_t P1 = (fwd ? s : ms) + 1, P2 = (fwd ? ms : s) + 1;
                        const bool r1 = fwd ? r_own : r_mate, r2 = fwd ? r_mate : r_own;
                        const int64_t a1 = r1 ? P1 - U : P1, b1 = r1 ? P1 : P1 + U;
                        const int64_t a2 = r2 ? P2 - U : P2, b2 = r2 ? P2 : P2 + U;
                        lo1 = a1 > lo1 ? a1 : lo1; hi1 = b1 < hi1 ? b1 : hi1;
                        lo2 = a2 > lo2 ? a2 : lo2; hi2 = b2 < hi2 ? b2 : hi2;
                        ++cnt;
                    }
                }
            }
            if (m_in != ~0ull) break;   // (sorted: the first record behind the window ends it)
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long a = __shfl_xor((long long)lo1, o), b = __shfl_xor((long long)hi1, o);
        const long long c = __shfl_xor((long long)lo2, o), d = __shfl_xor((long long)hi2, o);
        lo1 = a > lo1 ? a : lo1; hi1 = b < hi1 ? b : hi1;
        lo2 = c > lo2 ? c : lo2; hi2 = d < hi2 ? d : hi2;
        cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) {
        KiBounds r{};
        r.n = cnt;
        if (cnt) { r.lo1 = (int32_t)ki_clamp(lo1); r.hi1 = (int32_t)ki_clamp(hi1); r.lo2 = (int32_t)ki_clamp(lo2); r.hi2 = (int32_t)ki_clamp(hi2); }
        p.out[q] = r;
    }
}

}  // namespace

void launch_ki(const KiParams& p, hipStream_t s) {
    if (!p.nq) return;
    hipLaunchKernelGGL(ki_bounds_kernel, dim3((p.nq + kKiWaves - 1) / kKiWaves), dim3(kKiWaves * 64), 0, s, p);
}

}  // namespace bdx

// (bdx_warm_up: the HIP runtime loads a translation unit's device code at the first launch of any of its kernels)
__global__ void ki_noop_kernel() {}
namespace bdx { void warm_ki(hipStream_t s) { hipLaunchKernelGGL(ki_noop_kernel, dim3(1), dim3(64), 0, s); } }
