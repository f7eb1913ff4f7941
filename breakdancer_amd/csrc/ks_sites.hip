// KS -- alternate-supporting read pairs at given SV sites (bdx_count_site_pairs; the DV column of the CLI's --sites).
// No counterpart in the reference: its supporting-pair count exists only for the calls its own walk makes.
//
// A site is (tid1, pos1, tid2, pos2, flag_mask), positions 1-based, (tid1, pos1) <= (tid2, pos2).  A record is near P on T when its
// tid == T and |pos + 1 - P| <= window; its mate when mtid == T and |mpos + 1 - P| <= window.  Record i counts when K1 let it pass and
// its ReadFlag (after the pass-2 remaps) is in flag_mask, it is its pair's lower mate ((tid, pos) < (mtid, mpos), or equal and first in
// pair: each pair once), and it is near pos1 with its mate near pos2 (forward) or near pos2 with its mate near pos1 (reverse).  Only the
// record's own fields are looked at.  A lower mate near pos2 whose mate is near pos1 exists only when the two windows overlap (same
// chromosome, pos2 - pos1 <= 2 window): then their union is scanned once and both routes are tested per record (one that matches both
// ways counts once); otherwise window 1 alone is scanned, forward only.
//
// One wavefront per site, as K8 (k8_junction.hip): the first record of the read-start window [pos1 - 1 - window, ...] is found by the
// 64-ary ballot search (bdx_wave_search.h), then the lanes stride the window 64 records at a time until a record lies behind it.  Counts
// per key: one ballot + popcount per step with one key; per-wave LDS counters otherwise (at most 255 keys).  All arithmetic on positions
// is 64-bit: window may be 2^30 and positions 2^31 - 1.
#include <hip/hip_runtime.h>

#include "../../include/bdx.h"
#include "bdx_dev.h"
#include "bdx_shard.h"
#include "bdx_wave_search.h"

namespace bdx {

static_assert(sizeof(KsSite) == sizeof(bdx_site) && sizeof(KsSite) == 20, "KsSite is bdx_site");

namespace {

constexpr int kKsWaves = 4;

__device__ __forceinline__ bool ks_near(int32_t t, int64_t s, int32_t T, int64_t P, int64_t w) {
    const int64_t d = s + 1 - P;
    return t == T && d <= w && -d <= w;
}

__global__ __launch_bounds__(kKsWaves * 64) void ks_sites_kernel(KsParams p) {
    extern __shared__ uint32_t s_cnt[];   // [kKsWaves][nkeys] (nkeys > 1 only)
    const int lane = lane_id(), w = wave_id();
    const uint32_t q = blockIdx.x * kKsWaves + (uint32_t)w;
    const bool live = q < p.nq;   // (wave-uniform: every wave reaches the barriers)
    const int nkeys = p.nkeys;
    uint32_t* cnt = s_cnt + w * nkeys;
    const bool many = nkeys > 1;
    if (many) {
        for (int k = lane; k < nkeys; k += 64) cnt[k] = 0;
        __syncthreads();
    }
    uint32_t single = 0;
    if (live && p.n) {
        const KsSite st = p.sites[q];
        const int32_t t1 = st.tid1, t2 = st.tid2;
        const int64_t p1 = st.pos1, p2 = st.pos2, win = p.window;
        const uint32_t mask = st.flag_mask;
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
            bool hit = false;
            uint32_t key = 0;
            if (in) {
                const uint32_t c = p.cls[i];
                if ((c & BDX_CLS_PASS) && ((mask >> BDX_CLS_FLAG(c)) & 1u)) {
                    const int32_t mt = p.mtid[i];
                    const int64_t ms = p.mpos[i];
                    // the pair's lower mate (the record's tid is t1 here)
                    const bool lower = t1 < mt || (t1 == mt && (s < ms || (s == ms && (p.flag[i] & 0x40))));
                    const bool fwd = ks_near(t1, s, t1, p1, win) && ks_near(mt, ms, t2, p2, win);
                    const bool rev = overlap && ks_near(t1, s, t2, p2, win) && ks_near(mt, ms, t1, p1, win);
                    hit = lower && (fwd || rev);
                    if (hit && many) {
                        key = p.key[i];
                        key = key < (uint32_t)nkeys ? key : 0u;   // (an index out of range counts as 0, like everywhere in the store)
                    }
                }
            }
            if (many) {
                if (hit) atomicAdd(&cnt[key], 1u);
            } else {
                single += (uint32_t)popc64(ballot64(hit));
            }
            if (m_in != ~0ull) break;   // (sorted: the first record behind the window ends it)
        }
    }
    if (many) {
        __syncthreads();
        if (live)
            for (int k = lane; k < nkeys; k += 64) p.counts[(uint64_t)q * nkeys + k] = cnt[k];
    } else if (live && lane == 0) {
        p.counts[q] = single;
    }
}

}  // namespace

void launch_ks(const KsParams& p, hipStream_t s) {
    if (!p.nq) return;
    const size_t lds = p.nkeys > 1 ? (size_t)kKsWaves * p.nkeys * 4 : 0;
    hipLaunchKernelGGL(ks_sites_kernel, dim3((p.nq + kKsWaves - 1) / kKsWaves), dim3(kKsWaves * 64), lds, s, p);
}

}  // namespace bdx

// (bdx_warm_up: the HIP runtime loads a translation unit's device code at the first launch of any of its kernels)
__global__ void ks_noop_kernel() {}
namespace bdx { void warm_ks(hipStream_t s) { hipLaunchKernelGGL(ks_noop_kernel, dim3(1), dim3(64), 0, s); } }
