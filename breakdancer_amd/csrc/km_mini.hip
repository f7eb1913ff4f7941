// KW -- insert-size shift of the read pairs that start inside given windows of the resident, (tid, pos)-sorted record store
// (bdx_window_insert_shift; the CLI's --mini).  No counterpart in the C++ reference; the rule is in include/bdx.h.
//
// One wavefront per window, four per block, a persistent grid striding over the windows.  The wave walks the window's read starts
// (wave_window_walk, bdx_window.h: (tid, [beg, end - 1])).  The class byte is the first column loaded; isize, mtid, mpos, flag and lib are
// loaded only for records whose class byte qualifies (passed, and one of the four insert-size classes), as SiteRule::match does.
//
// What a step's observations give at once, per library: n, n_over and the sum of x.  The wave groups its lanes by library (a ballot loop
// over the distinct libraries present, as KH groups its lanes), one popcount / one wave sum per group, and the library's OWNER lane adds
// them to its registers: lane l owns libraries l, l + 64, l + 128, l + 192 (KwAcc).  These stay exact for a window of any size.
//
// The ranks need all observations of the window at once.  The walk compacts them into the wave's slice of LDS, value and library packed into
// one word (x in bits 0..14, the library in 15..22; BDX_MINI_CAP words = 16 KiB per wave, 64 KiB per block, two blocks per CU); an
// observation beyond the slice is counted and not stored, and such a window is SATURATED: its t's are 0.  Then one of two routes:
//   registers  at most 64 observations (the common case: tens of pairs at 30x): lane l takes observation l back into a register, and a
//              loop over the occupied lanes (one v_readlane each: the lane's word comes back in a scalar register) counts, per lane, the
//              observations of its library that are <= and < its own, and the library's n.
//   staged     up to BDX_MINI_CAP (and at every size under bdx_set_debug "mini_staged"): 64 observations at a time take the lanes, and an
//              all-pairs pass over the slice counts the same three numbers -- four words per LDS read, all lanes the same address (a
//              broadcast); the slice's last quad is padded with a word no library matches.
// Either way the lane then reads N_L, C_L(x) and C_L(x - 1) straight from the device table (256 KiB per library: it lives in L2), forms
// its two int64 candidates, and a second ballot loop over the distinct libraries takes the per-library maxima to the owner lanes.  The wave
// writes all nlibs rows of its window, zeros included.  No float, no atomics, no workgroup barrier: a wave touches no LDS but its own slice,
// and what orders its writes and reads there is written out (kw_wave_order).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/bdx.h"
#include "bdx_dev.h"
#include "bdx_window.h"

namespace bdx {

static_assert(sizeof(KwShift) == sizeof(bdx_insert_shift) && sizeof(KwShift) == 40 && alignof(KwShift) == 8, "KwShift is bdx_insert_shift");

namespace {

constexpr int kMiniWaves = 4;
constexpr int kMiniMaxGrid = 512;           // two blocks per CU (LDS) on 256 CUs
constexpr uint32_t kCap = BDX_MINI_CAP;
constexpr uint32_t kNoWord = 0xFFFFFFFFu;   // (its library field is 0x1FFFF: no observation's)
constexpr uint32_t kMiniClasses = (1u << BDX_NORMAL_FR) | (1u << BDX_NORMAL_RF) | (1u << BDX_ARP_LARGE_INSERT) | (1u << BDX_ARP_SMALL_INSERT);
static_assert(BDX_ISIZE_BINS == 1 << 15, "an observation is 15 bits of its word");
static_assert(kCap % 4 == 0 && (size_t)kMiniWaves * kCap * 4 <= 65536, "the slices are read in quads and fill a block's static LDS at most");

// One wave's accesses to its own slice: its stores before the loads that follow, and a window's loads before the next window's stores.  The
// LDS serves one wave's operations in the order they were issued; the fence pins the memory operations for the compiler, the wave barrier
// (no instruction) keeps the lanes' code from being moved across it.
__device__ __forceinline__ void kw_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int64_t wave_max_i64(int64_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_xor((long long)v, o);
        v = t > v ? t : v;
    }
    return v;
}

// per-library results in registers: lane l owns libraries l + 64 k, slot k (scalars, not arrays: they must stay registers)
struct KwSlot {
    uint32_t n = 0, over = 0;
    uint64_t sum = 0;
    int64_t tp = 0, tm = 0;
};
struct KwAcc {
    KwSlot s0, s1, s2, s3;

    // (lib is wave-uniform.  Every slot takes a masked operand: a slot chosen by pointer or by branch would send them all to scratch)
    __device__ __forceinline__ void count(uint32_t lib, uint32_t cnt, uint32_t ov, uint32_t sx) {
        const bool mine = lane_id() == (int)(lib & 63u);
        const uint32_t k = lib >> 6;
        auto add = [&](KwSlot& s, bool on) { s.n += on ? cnt : 0u; s.over += on ? ov : 0u; s.sum += on ? sx : 0u; };
        add(s0, mine && k == 0); add(s1, mine && k == 1); add(s2, mine && k == 2); add(s3, mine && k == 3);
    }
    // (p, m >= 0, and so is every slot)
    __device__ __forceinline__ void raise(uint32_t lib, int64_t p, int64_t m) {
        const bool mine = lane_id() == (int)(lib & 63u);
        const uint32_t k = lib >> 6;
        auto top = [&](KwSlot& s, bool on) {
            const int64_t a = on ? p : 0, b = on ? m : 0;
            s.tp = a > s.tp ? a : s.tp; s.tm = b > s.tm ? b : s.tm;
        };
        top(s0, mine && k == 0); top(s1, mine && k == 1); top(s2, mine && k == 2); top(s3, mine && k == 3);
    }
};

// A lane's observation w (valid lanes only) with le / lt = the observations of its library <= / < its own and cnt = the library's n: the
// lane's two candidates, and their maxima per library to the owner lanes.  Called by all 64 lanes.
__device__ __forceinline__ void kw_finish(const uint64_t* __restrict__ ctab, uint32_t w, bool valid, uint32_t le, uint32_t lt, uint32_t cnt, KwAcc& acc) {
    int64_t tp = 0, tm = 0;
    const uint32_t lib = w >> 15, x = w & 0x7FFFu;
    if (valid) {
        const uint64_t* row = ctab + (size_t)lib * BDX_ISIZE_BINS;
        const int64_t N = (int64_t)row[BDX_ISIZE_BINS - 1], Cx = (int64_t)row[x], Cm = x ? (int64_t)row[x - 1] : 0;
        // (every product is below 2^63: a count <= BDX_MINI_CAP = 2^12 times a null count <= N < 2^51)
        tp = (int64_t)le * N - Cx * (int64_t)cnt;
        tm = Cm * (int64_t)cnt - (int64_t)lt * N;
        tp = tp < 0 ? 0 : tp;
        tm = tm < 0 ? 0 : tm;
    }
    uint64_t pend = ballot64(valid);
    while (pend) {
        const uint32_t lib0 = (uint32_t)__shfl((int)lib, __builtin_ctzll(pend));
        const bool g = valid && lib == lib0;
        const int64_t gp = wave_max_i64(g ? tp : 0), gm = wave_max_i64(g ? tm : 0);
        acc.raise(lib0, gp, gm);
        pend &= ~ballot64(g);
    }
}

__global__ __launch_bounds__(kMiniWaves * 64) void kw_shift_kernel(KwParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t s_obs[kMiniWaves][kCap];
    const StoreView& v = p.st;
    const int lane = lane_id();
    uint32_t* slice = s_obs[wave_id()];
    const uint32_t nlibs = (uint32_t)p.nlibs;
    const bool many = nlibs > 1;
    const uint64_t below = (1ull << lane) - 1;
    // (q is wave-uniform; the kernel has no workgroup barrier)
    for (uint64_t q = (uint64_t)blockIdx.x * kMiniWaves + (uint64_t)wave_id(); q < p.nq; q += (uint64_t)gridDim.x * kMiniWaves) {
        const KrInterval iv = p.iv[q];
        const int32_t t = iv.tid;
        KwAcc acc;
        uint64_t nobs = 0;
        kw_wave_order();   // (the last window's loads are issued)
        wave_window_walk(v.tid, v.pos, v.n, t, (int64_t)iv.beg, (int64_t)iv.end - 1, [&](uint64_t i, int64_t s, bool in) {
            bool obs = false, over = false;
            uint32_t lib = 0, x = 0;
            if (in) {
                const uint32_t c = v.cls[i];
                if ((c & BDX_CLS_PASS) && ((kMiniClasses >> BDX_CLS_FLAG(c)) & 1u)) {
                    const int32_t mt = v.mtid[i];
                    const int64_t ms = v.mpos[i];
                    const uint32_t fl = v.flag[i];
                    const int64_t z = v.isize[i];
                    // (the record's tid is t) on one sequence, and its pair's lower mate
                    if (mt == t && (s < ms || (s == ms && (fl & 0x40u)))) {
                        const int64_t ax = z < 0 ? -z : z;
                        if (many) {
                            lib = p.lib[i];
                            lib = lib < nlibs ? lib : 0u;   // (an index out of range is library 0, like everywhere in the store)
                        }
                        over = ax >= BDX_ISIZE_BINS;
                        obs = !over;
                        x = obs ? (uint32_t)ax : 0u;
                    }
                }
            }
            const uint64_t m_obs = ballot64(obs);
            uint64_t pend = ballot64(obs || over);
            while (pend) {   // one round per distinct library among the step's lanes
                const uint32_t lib0 = (uint32_t)__shfl((int)lib, __builtin_ctzll(pend));
                const bool g = (obs || over) && lib == lib0;
                const uint64_t m_g = ballot64(g);
                const uint32_t cnt = (uint32_t)popc64(m_g & m_obs);
                acc.count(lib0, cnt, (uint32_t)popc64(m_g) - cnt, wave_sum_u32(g ? x : 0u));   // (x is 0 on an `over` lane; 64 x 32767 fits)
                pend &= ~m_g;
            }
            const uint64_t at = nobs + (uint64_t)popc64(m_obs & below);
            if (obs && at < kCap) slice[at] = (lib << 15) | x;
            nobs += (uint64_t)popc64(m_obs);
        });
        const bool saturated = nobs > kCap;
        if (!saturated && nobs) {   // (wave-uniform)
            const uint32_t m = (uint32_t)nobs;
            if (m <= 64 && !p.staged) {
                kw_wave_order();
                const bool valid = (uint32_t)lane < m;
                const uint32_t w = valid ? slice[lane] : kNoWord;
                uint32_t le = 0, lt = 0, cnt = 0;
                for (uint32_t j = 0; j < m; ++j) {
                    const uint32_t wj = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)j);   // (j is wave-uniform: the value comes back in a scalar register)
                    const bool same = (wj >> 15) == (w >> 15);
                    cnt += same; le += same && wj <= w; lt += same && wj < w;
                }
                kw_finish(p.ctab, w, valid, le, lt, cnt, acc);
            } else {
                const uint32_t quads = (m + 3) / 4;
                if (m + (uint32_t)lane < 4 * quads) slice[m + lane] = kNoWord;   // (at most three words, below kCap: kCap is a multiple of 4)
                kw_wave_order();
                const uint4* all = (const uint4*)slice;
                for (uint32_t base = 0; base < m; base += 64) {
                    const bool valid = base + (uint32_t)lane < m;
                    const uint32_t w = valid ? slice[base + lane] : kNoWord;
                    const uint32_t wl = w >> 15;
                    uint32_t le = 0, lt = 0, cnt = 0;
                    for (uint32_t j = 0; j < quads; ++j) {
                        const uint4 o = all[j];
                        const bool s0 = (o.x >> 15) == wl, s1 = (o.y >> 15) == wl, s2 = (o.z >> 15) == wl, s3 = (o.w >> 15) == wl;
                        cnt += (uint32_t)s0 + s1 + s2 + s3;
                        le += (uint32_t)(s0 && o.x <= w) + (s1 && o.y <= w) + (s2 && o.z <= w) + (s3 && o.w <= w);
                        lt += (uint32_t)(s0 && o.x < w) + (s1 && o.y < w) + (s2 && o.z < w) + (s3 && o.w < w);
                    }
                    kw_finish(p.ctab, w, valid, le, lt, cnt, acc);
                }
            }
        }
        auto write = [&](const KwSlot& a, uint32_t k) {
            const uint32_t lib = (uint32_t)lane + 64u * k;
            if (lib < nlibs) {
                KwShift r{};
                r.n = a.n; r.n_over = a.over; r.saturated = saturated ? 1u : 0u; r.sum = a.sum;
                r.t_plus = saturated ? 0 : a.tp;
                r.t_minus = saturated ? 0 : a.tm;
                p.out[q * nlibs + lib] = r;
            }
        };
        write(acc.s0, 0); write(acc.s1, 1); write(acc.s2, 2); write(acc.s3, 3);
    }
}

}  // namespace

void launch_kw(const KwParams& p, hipStream_t s) {
    if (!p.nq) return;
    const uint32_t blocks = (p.nq + kMiniWaves - 1) / kMiniWaves;
    hipLaunchKernelGGL(kw_shift_kernel, dim3(std::min<uint32_t>(blocks, kMiniMaxGrid)), dim3(kMiniWaves * 64), 0, s, p);
}

}  // namespace bdx
