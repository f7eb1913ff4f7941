// KA -- the one-end-anchored reads (class byte BDX_MATE_UNMAPPED: mapped, mate unmapped) that start inside given windows of the resident,
// (tid, pos)-sorted record store, and the position that best splits them into right-pointing anchors on its left and left-pointing ones
// on its right (bdx_window_anchor_split; the CLI's --anchor).  No counterpart in the C++ reference; the rule is in include/bdx.h.
//
// One wavefront per window, four per block, a persistent grid striding over the windows, as KW (km_mini.hip).  The wave walks the window's
// read starts (wave_window_walk, bdx_window.h: (tid, [beg, end - 1])).  The class byte is the first column loaded; the SAM flag, the quality
// and the library are loaded only for records whose byte is 9, the library only when the quality test is per library and there are several.
//
// First walk: the split.  With d = +1 for an anchor that points right, -1 for one that points left and 0 for every other record,
// A(S) + B(S) = D(S) + n_rev where D(S) is the sum of d over the records with pos < S: the split is the smallest S with the largest D.  D
// changes only behind a position that holds records, so the candidates are S = beg and S = pos + 1 for every pos present.  Per 64-record
// step a lane takes the previous record's pos (one __shfl_up; lane 0 the last step's last, beg - 1 in front of the first record) and the
// exclusive prefix of d (the wave scan of bdx_scan.h plus the total carried from the steps before): that pair is a candidate when the lane's
// own pos differs from the previous one -- inside a run of equal positions the prefix is no D(S) of any S: the rule speaks of positions --,
// and the first lane behind the window closes the last run.  Every lane keeps the largest key (D biased into 32 bits, then ~S: the smaller
// S wins a tie) it has seen; one 64-bit wave maximum at the end.
// Second walk, skipped (wave-uniformly) when the first saw no anchor: with the split known, the counts on either side by ballots, last_left
// and first_right from the highest and the lowest lane of their masks (the store is sorted), and the distinct starts: a lane finds the
// previous anchor of its side through the ballot mask below its lane and one shuffle of pos (the last step's last one is carried) and
// counts when the two differ.  No LDS, no atomics, no workgroup barrier, no float.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/bdx.h"
#include "bdx_dev.h"
#include "bdx_scan.h"
#include "bdx_window.h"

namespace bdx {

static_assert(sizeof(KaSplit) == sizeof(bdx_anchor_split) && sizeof(KaSplit) == 40 && alignof(KaSplit) == 4, "KaSplit is bdx_anchor_split");

namespace {

constexpr int kAnchorWaves = 4;
constexpr int kAnchorMaxGrid = 2048;        // eight blocks = 32 waves per CU on 256 CUs: nothing but registers limits it

// what a record is to a window: 0 nothing, 1 a candidate of low quality, 2 an anchor that points right, 3 one that points left
struct KaKind {
    const KaParams& p;
    const bool many;
    __device__ __forceinline__ explicit KaKind(const KaParams& pp) : p(pp), many(pp.qtab != nullptr) {}
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
        if (p.st.cls[i] != BDX_MATE_UNMAPPED) return 0u;   // (the whole byte: such a record never carries BDX_CLS_PASS)
        const uint32_t fl = p.st.flag[i];
        const int32_t qual = p.mapq[i];
        int32_t least = p.q0;
        if (many) {
            uint32_t l = p.lib[i];
            l = l < (uint32_t)p.nlibs ? l : 0u;   // (an index out of range is library 0, like everywhere in the store)
            least = p.qtab[l];
        }
        if (qual <= least) return 1u;
        return (((fl & 0x10u) != 0) != (p.long_insert != 0)) ? 3u : 2u;
    }
};

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_xor((unsigned long long)v, o);
        v = t > v ? t : v;
    }
    return v;
}

__global__ __launch_bounds__(kAnchorWaves * 64) void ka_split_kernel(KaParams p) {
    const StoreView& v = p.st;
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1;
    const KaKind kind(p);
    // (q is wave-uniform; the kernel has no workgroup barrier)
    for (uint64_t q = (uint64_t)blockIdx.x * kAnchorWaves + (uint64_t)wave_id(); q < p.nq; q += (uint64_t)gridDim.x * kAnchorWaves) {
        const KrInterval iv = p.iv[q];
        const int32_t t = iv.tid;
        const int64_t beg = iv.beg, whi = (int64_t)iv.end - 1;
        KaSplit r{};
        r.split = iv.beg;
        r.last_left = -1;
        r.first_right = -1;
        // ---- first walk: n_fwd, n_rev, n_low and the split
        uint64_t best = 0;           // per lane: (D + 2^31) << 32 | ~S
        int32_t carry_d = 0;         // sum of d over the steps before this one (|D| < 2^31: the counts of a row are 32-bit)
        int64_t carry_s = beg - 1;   // the last record's pos of the step before
        wave_window_walk(v.tid, v.pos, v.n, t, beg, whi, [&](uint64_t i, int64_t s, bool in) {
            const uint32_t k = in ? kind(i) : 0u;
            const uint64_t m_in = ballot64(in);
            r.n_low += (uint32_t)popc64(ballot64(k == 1u));
            r.n_fwd += (uint32_t)popc64(ballot64(k == 2u));
            r.n_rev += (uint32_t)popc64(ballot64(k == 3u));
            const int32_t d = k == 2u ? 1 : k == 3u ? -1 : 0;
            const int32_t inc = (int32_t)wave_incl_scan_t<uint32_t>((uint32_t)d);
            const int32_t up = __shfl_up((int32_t)s, 1);
            const int64_t prev = lane ? (int64_t)up : carry_s;   // (read only where the lane before is inside, or this is lane 0)
            // a lane inside opens a run of equal positions or continues one; the first lane behind the window closes the last run
            const bool cand = in ? s != prev : m_in == below;
            if (cand) {
                const int64_t D = (int64_t)carry_d + inc - d, S = prev + 1;   // (beg <= S <= end <= 2^31 - 1)
                const uint64_t key = ((uint64_t)(D + 2147483648ll) << 32) | (uint32_t)~(uint32_t)S;
                best = key > best ? key : best;
            }
            carry_d += __shfl(inc, 63);
            carry_s = (int64_t)__shfl((int32_t)s, 63);   // (used by the next step only, which exists only when lane 63 is inside)
        });
        if (r.n_fwd + r.n_rev) {   // (wave-uniform)
            best = wave_max_u64(best);
            const int64_t split = (int64_t)(uint32_t)~(uint32_t)best;
            r.split = (int32_t)split;
            // ---- second walk: the two sides of the split
            int64_t prev_l = -1, prev_r = -1;   // the last anchor's pos of either side in the steps before (-1: none; a pos is >= 0)
            wave_window_walk(v.tid, v.pos, v.n, t, beg, whi, [&](uint64_t i, int64_t s, bool in) {
                const uint32_t k = in ? kind(i) : 0u;
                const bool left = k == 2u && s < split, right = k == 3u && s >= split;
                const uint64_t m_l = ballot64(left), m_r = ballot64(right);
                const uint64_t b_l = m_l & below, b_r = m_r & below;
                // (one shuffle serves both sides: a lane is on one side at most)
                const uint64_t b = left ? b_l : b_r;
                const int32_t got = __shfl((int32_t)s, b ? 63 - __builtin_clzll(b) : 0);
                const int64_t before = b ? (int64_t)got : left ? prev_l : prev_r;
                r.n_left += (uint32_t)popc64(m_l);
                r.n_right += (uint32_t)popc64(m_r);
                r.u_left += (uint32_t)popc64(ballot64(left && s != before));
                r.u_right += (uint32_t)popc64(ballot64(right && s != before));
                if (m_l) {
                    prev_l = (int64_t)__shfl((int32_t)s, 63 - __builtin_clzll(m_l));
                    r.last_left = (int32_t)prev_l;
                }
                if (m_r) {
                    if (prev_r < 0) r.first_right = __shfl((int32_t)s, __builtin_ctzll(m_r));
                    prev_r = (int64_t)__shfl((int32_t)s, 63 - __builtin_clzll(m_r));
                }
            });
        }
        if (lane == 0) p.out[q] = r;
    }
}

}  // namespace

void launch_ka(const KaParams& p, hipStream_t s) {
    if (!p.nq) return;
    const uint64_t blocks = (p.nq + kAnchorWaves - 1) / kAnchorWaves;
    hipLaunchKernelGGL(ka_split_kernel, dim3((uint32_t)std::min<uint64_t>(blocks, kAnchorMaxGrid)), dim3(kAnchorWaves * 64), 0, s, p);
}

}  // namespace bdx

// (bdx_warm_up: the HIP runtime loads a translation unit's device code at the first launch of any of its kernels)
__global__ void ka_noop_kernel() {}
namespace bdx { void warm_ka(hipStream_t s) { hipLaunchKernelGGL(ka_noop_kernel, dim3(1), dim3(64), 0, s); } }
