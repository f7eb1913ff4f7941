// KH -- insert-size histogram per library over the resident record store (bdx_insert_size_histogram; the CLI's --estimate).
// No counterpart in the reference: bam2cfg takes these observations from the first ~10,000 pairs of a file on the host.
//
// A record is an observation x = isize of its library when flag has 0x1 and 0x2 and none of 0x4, 0x8, 0x400, mtid == tid, isize >= 0 and
// its quality is above the library's minimum (int comparison, the minimum resolved as for K1); x >= BDX_ISIZE_BINS only counts in
// n_over.  All counts are integers: the result does not depend on the order the atomics land in.
//
// HBM-bound by design: 16 B/read in (tid, mtid, isize, u16 flag, u8 mapq, u8 lib; 15 B with one library, whose column is not resident),
// in K1's access shape -- a tile is 256 consecutive reads = one wave64, lane l owns reads [4l, 4l + 4), one 16/8/4-byte load per lane
// and column, no workgroup barrier inside the tile loop.
// Counting: persistent workgroups, each with a private table of kLdsBins 32-bit counters in LDS (32 KiB, 35 with the three small tables:
// four workgroups per CU).  The table is cut evenly among the libraries: library L owns a WINDOW of W = kLdsBins / nlibs values (8192 for
// one library, 2048 for four, 32 for 255), [off, off + W) with off = clamp(int(mean) - W / 2, 0, BDX_ISIZE_BINS - W) around the mean the
// library was created or last set with -- the prefix [0, W) while the mean is below W / 2 (every library up to eight at a 400 bp insert)
// or not given (a bare configuration: mean 0).  The window only decides which route an observation takes, never the result.
// An observation inside its library's window is ONE LDS atomic; a slot whose observations all carry the same value (a wave
// of equal inserts: the worst case of same-address serialisation) adds its popcount once.  Observations outside the range -- a tail, or
// a mate-pair library beside many others -- take the global route: the wave groups its lanes by (library, value) and one lane per group
// adds the group's size to the 64-bit global table.  At the end every workgroup adds its non-zero LDS counters to the global table:
// (workgroups x touched bins) 64-bit atomics, consecutive bins from consecutive lanes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/bdx.h"
#include "bdx_dev.h"

namespace bdx {

namespace {

constexpr int kLdsBins = 8192;
static_assert(kLdsBins <= BDX_ISIZE_BINS, "a library's LDS range is a prefix of its bins");
static_assert(kLdsBins / 255 >= 1, "every library owns at least one LDS bin");

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned short v4us __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kBlock) void kh_hist_kernel(const KhParams p) {
    __shared__ uint32_t s_hist[kLdsBins];
    __shared__ uint32_t s_over[256];
    __shared__ int32_t s_minq[256];
    __shared__ uint32_t s_off[256];   // first value of the library's LDS window
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int nlibs = p.nlibs;
    const uint32_t W = (uint32_t)kLdsBins / (uint32_t)nlibs;
    for (int i = t; i < kLdsBins; i += kBlock) s_hist[i] = 0;
    for (int i = t; i < 256; i += kBlock) {
        s_over[i] = 0;
        s_minq[i] = i < nlibs ? p.libs[i].min_mapq : 0;
        // (fmaxf drops a NaN mean; the clamps keep [off, off + W) inside the bins for any float)
        const float m = i < nlibs ? fminf(fmaxf(p.lib_mean[i], 0.f), (float)BDX_ISIZE_BINS) : 0.f;
        const int lo = (int)m - (int)(W / 2), hi = BDX_ISIZE_BINS - (int)W;
        s_off[i] = (uint32_t)(lo < 0 ? 0 : lo > hi ? hi : lo);
    }
    __syncthreads();

    const uint64_t ntiles = (p.n + kTile - 1) / kTile;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t tile = (uint64_t)blockIdx.x * kWaves + w; tile < ntiles; tile += nwaves) {
        const uint64_t base = tile * kTile + (uint64_t)lane * 4;
        int tid[4], mtid[4], isz[4];
        unsigned sam[4];
        unsigned mqp = 0, libp = 0;   // the four slots' bytes, slot r in byte r
        int nvalid = 0;
        if (base + 4 <= p.n) {
            nvalid = 4;
            const v4i a = __builtin_nontemporal_load((const v4i*)(p.tid + base));
            const v4i c = __builtin_nontemporal_load((const v4i*)(p.mtid + base));
            const v4i e = __builtin_nontemporal_load((const v4i*)(p.isize + base));
            const v4us f = __builtin_nontemporal_load((const v4us*)(p.flag + base));
            mqp = __builtin_nontemporal_load((const uint32_t*)(p.mapq + base));
            libp = p.lib ? __builtin_nontemporal_load((const uint32_t*)(p.lib + base)) : 0u;
            tid[0] = a.x; tid[1] = a.y; tid[2] = a.z; tid[3] = a.w;
            mtid[0] = c.x; mtid[1] = c.y; mtid[2] = c.z; mtid[3] = c.w;
            isz[0] = e.x; isz[1] = e.y; isz[2] = e.z; isz[3] = e.w;
            sam[0] = f.x; sam[1] = f.y; sam[2] = f.z; sam[3] = f.w;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t i = base + r;
                const bool v = i < p.n;
                nvalid += v;
                tid[r] = v ? p.tid[i] : 0; mtid[r] = v ? p.mtid[i] : 0; isz[r] = v ? p.isize[i] : 0; sam[r] = v ? p.flag[i] : 0;
                mqp |= (v ? (unsigned)p.mapq[i] : 0u) << (8 * r);
                libp |= (v && p.lib ? (unsigned)p.lib[i] : 0u) << (8 * r);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned L = (libp >> (8 * r)) & 0xffu;
            L = L < (unsigned)nlibs ? L : 0u;   // (an index out of range counts as 0, like everywhere in the store)
            const int x = isz[r];
            // paired, proper, both ends mapped, not a duplicate; the lower mate of a pair on one sequence; well mapped
            const bool obs = r < nvalid && (sam[r] & 0x40Fu) == 0x3u && tid[r] == mtid[r] && x >= 0 && (int)((mqp >> (8 * r)) & 0xffu) > s_minq[L];
            const bool over = obs && x >= BDX_ISIZE_BINS;
            const bool in = obs && !over;
            const uint32_t rel = (uint32_t)x - s_off[L];                     // (wraps to a large value below the window)
            const bool local = in && rel < W;
            const uint32_t slot = L * W + rel;                               // (meaningful where local)
            const uint32_t bin = L * (uint32_t)BDX_ISIZE_BINS + (uint32_t)x; // (meaningful where in)
            if (over) atomicAdd(&s_over[L], 1u);
            const uint64_t m_local = ballot64(local);
            if (m_local) {
                const int first = __builtin_ctzll(m_local);
                const uint32_t slot0 = __shfl(slot, first);
                if (ballot64(local && slot == slot0) == m_local) {   // (wave-uniform) one value: one add of the popcount
                    if (lane == first) atomicAdd(&s_hist[slot0], (uint32_t)popc64(m_local));
                } else if (local) {
                    atomicAdd(&s_hist[slot], 1u);
                }
            }
            // the global route: one add per distinct (library, value) among the wave's lanes
            uint64_t pend = ballot64(in && !local);
            while (pend) {
                const int first = __builtin_ctzll(pend);
                const uint32_t bin0 = __shfl(bin, first);
                const uint64_t same = ballot64(in && !local && bin == bin0);
                if (lane == first) atomicAdd(&p.hist[bin0], (unsigned long long)popc64(same));
                pend &= ~same;
            }
        }
    }
    __syncthreads();
    const uint32_t used = W * (uint32_t)nlibs;
    for (uint32_t i = t; i < used; i += kBlock) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&p.hist[(size_t)(i / W) * BDX_ISIZE_BINS + s_off[i / W] + i % W], (unsigned long long)v);
    }
    for (int i = t; i < nlibs; i += kBlock)
        if (s_over[i]) atomicAdd(&p.n_over[i], (unsigned long long)s_over[i]);
}

}  // namespace

void launch_kh(const KhParams& p, hipStream_t s) {
    if (!p.n) return;
    const uint64_t ntiles = (p.n + kTile - 1) / kTile;
    const int grid = (int)std::min<uint64_t>((ntiles + kWaves - 1) / kWaves, (uint64_t)kKhMaxGrid);
    hipLaunchKernelGGL(kh_hist_kernel, dim3(grid), dim3(kBlock), 0, s, p);
}

}  // namespace bdx
