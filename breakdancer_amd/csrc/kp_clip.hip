// KP -- where the clipped reads pile up around one end of given SV sites (bdx_site_clip_peaks; the CL* keys of the CLI's --clip).  No
// counterpart in the reference.  The rule in words: include/bdx.h.
//
// Shaped like KM (kq_queries.hip): one wavefront per query, four per block, no workgroup barrier -- a wave without a query leaves at once.
// A query is (site, end); (T, P) the asked end.  A record gives a left observation at X = pos + 1 and a right one at X = pos + span (clip
// word: bdx_clip.h), and one counts when the record passes, tid == T and |X - P| <= window.  The wave walks the ONE window of read starts
// (T, [P - window - BDX_CLIP_SPAN_MAX, P - 1 + window]): a left clip's read starts at X - 1, a right clip's up to BDX_CLIP_SPAN_MAX in front
// of its X.  Every wave owns a row of 2 (2 window + 1) words of dynamic LDS -- bin X - (P - window) of the left half or of the right one --
// sized from the call's window, at most 4094 words (16 KiB a wave, 64 KiB a block).  The wave clears its row, adds with one LDS atomic per
// observation, then scans it: lane l looks at bins l, l + 64, ... of either half and keeps its best under the tie rule (larger count, then
// smaller |X - P|, then smaller X) as one 64-bit key, one xor-shuffle max per side closes the query, and lane 0 writes the 24 bytes.  The
// class byte is loaded first; the clip word only for records that pass.
#include <hip/hip_runtime.h>

#include "../../include/bdx.h"
#include "bdx_dev.h"
#include "bdx_shard.h"
#include "bdx_window.h"

namespace bdx {

static_assert(sizeof(KpPeaks) == sizeof(bdx_clip_peaks) && sizeof(KpPeaks) == 24 && alignof(KpPeaks) == 4, "KpPeaks is bdx_clip_peaks");
static_assert(BDX_CLIP_WINDOW_MAX == 1023 && BDX_CLIP_SPAN_MAX <= 65535, "the key below packs |X - P| into 10 bits and the bin into 11");

namespace {

constexpr int kQueryWaves = 4;

// what orders one wave's accesses to its own row -- the clear before the atomics, the atomics before the reads: km_wave_order (kq_queries.hip)
__device__ __forceinline__ void kp_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// A bin's rank under the tie rule as one number, larger is better: the count, then the closeness to P, then the smaller bin.  0: empty.
__device__ __forceinline__ uint64_t kp_key(uint32_t cnt, uint32_t bin, uint32_t win) {
    const uint32_t dist = bin > win ? bin - win : win - bin;   // |X - P| <= 1023
    return cnt ? ((uint64_t)cnt << 22) | ((uint64_t)(1023u - dist) << 11) | (uint64_t)(2047u - bin) : 0ull;
}

__global__ __launch_bounds__(kQueryWaves * 64) void kp_clip_kernel(KpParams p) {
    extern __shared__ uint32_t s_row[];   // [kQueryWaves][2 nb], nb = 2 window + 1
    const StoreView& v = p.st;
    const uint32_t q = blockIdx.x * kQueryWaves + (uint32_t)wave_id();
    if (q >= p.nq) return;   // (wave-uniform; the kernel has no workgroup barrier)
    const int lane = lane_id();
    const uint32_t win = (uint32_t)p.window, nb = 2u * win + 1u;
    uint32_t* row = s_row + (size_t)wave_id() * 2u * nb;
    for (uint32_t k = (uint32_t)lane; k < 2u * nb; k += 64) row[k] = 0;
    kp_wave_order();
    const KsSite st = p.sites[q];
    const bool second = p.end[q] == 2;
    const int32_t T = second ? st.tid2 : st.tid1;
    const int64_t P = second ? st.pos2 : st.pos1, x0 = P - (int64_t)win;   // bin 0's X
    if (v.n) {
        const uint32_t least = (uint32_t)p.min_clip;
        wave_window_walk(v.tid, v.pos, v.n, T, x0 - BDX_CLIP_SPAN_MAX, P - 1 + (int64_t)win, [&](uint64_t i, int64_t s, bool in) {
            if (!in || !(v.cls[i] & BDX_CLS_PASS)) return;
            const uint32_t w = p.clip[i];
            const uint32_t left = w & 255u, right = (w >> 8) & 255u, span = w >> 16;
            // (bins are X - x0 in [0, nb): one unsigned comparison; X itself must be a 1-based position an int32 holds)
            const int64_t xl = s + 1, xr = s + (int64_t)span;
            if (left >= least && xl >= 1 && xl <= 2147483647ll && (uint64_t)(xl - x0) < (uint64_t)nb) atomicAdd(&row[(uint32_t)(xl - x0)], 1u);
            if (right >= least && span >= 1u && span <= (uint32_t)BDX_CLIP_SPAN_MAX && xr >= 1 && xr <= 2147483647ll && (uint64_t)(xr - x0) < (uint64_t)nb)
                atomicAdd(&row[nb + (uint32_t)(xr - x0)], 1u);
        });
    }
    kp_wave_order();
    uint32_t n_l = 0, n_r = 0;
    uint64_t best_l = 0, best_r = 0;
    for (uint32_t k = (uint32_t)lane; k < nb; k += 64) {
        const uint32_t a = row[k], b = row[nb + k];
        n_l += a; n_r += b;
        const uint64_t ka = kp_key(a, k, win), kb = kp_key(b, k, win);
        best_l = ka > best_l ? ka : best_l;
        best_r = kb > best_r ? kb : best_r;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t a = (uint64_t)__shfl_xor((long long)best_l, o), b = (uint64_t)__shfl_xor((long long)best_r, o);
        best_l = a > best_l ? a : best_l;
        best_r = b > best_r ? b : best_r;
        n_l += __shfl_xor(n_l, o);
        n_r += __shfl_xor(n_r, o);
    }
    if (lane == 0) {
        KpPeaks r{};
        r.n_left = n_l; r.n_right = n_r;
        if (best_l) { r.peak_left = (uint32_t)(best_l >> 22); r.pos_left = (int32_t)(x0 + (int64_t)(2047u - (uint32_t)(best_l & 2047u))); }
        if (best_r) { r.peak_right = (uint32_t)(best_r >> 22); r.pos_right = (int32_t)(x0 + (int64_t)(2047u - (uint32_t)(best_r & 2047u))); }
        p.out[q] = r;
    }
}

}  // namespace

constexpr size_t kp_lds_bytes(int32_t window) { return (size_t)kQueryWaves * 2 * (2 * (size_t)window + 1) * 4; }
static_assert(kp_lds_bytes(BDX_CLIP_WINDOW_MAX) <= 65536, "the rows of a block at the largest window fit the 64 KiB a launch may ask for");

void launch_kp(const KpParams& p, hipStream_t s) {
    if (!p.nq) return;
    hipLaunchKernelGGL(kp_clip_kernel, dim3((p.nq + kQueryWaves - 1) / kQueryWaves), dim3(kQueryWaves * 64), kp_lds_bytes(p.window), s, p);
}

}  // namespace bdx

// (bdx_warm_up: the HIP runtime loads a translation unit's device code at the first launch of any of its kernels)
__global__ void kp_noop_kernel() {}
namespace bdx { void warm_kp(hipStream_t s) { hipLaunchKernelGGL(kp_noop_kernel, dim3(1), dim3(64), 0, s); } }
