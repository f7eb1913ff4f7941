// K8, KS, KI, KM -- the kernels that answer queries over the resident, (tid, pos)-sorted record store after a run.  None has a
// counterpart in the reference: its table has no genotype, its supporting-pair count exists only for the calls its own walk makes, and it
// says nothing about how far a breakpoint may lie from a call's position.
//
// All of them: one wavefront per query, four per block.  The wave walks the query's window of read starts (wave_window_walk, bdx_window.h:
// first record by the 64-ary ballot search, then 64 records a step until one lies behind the window) and applies its own test to every
// record; K8 and KS count the hits per key (WaveKeyCounts, bdx_window.h), KS and KI share the rule of which records count for a site
// (SiteRule, bdx_window.h).
//
// K8 -- reference-supporting read pairs at SV junctions (bdx_count_junction_pairs; the input of the CLI's --vcf DR / GT columns).
// A query is one chromosome and one or two junctions a <= b (the boundary between base p and p + 1, 1-based).  A read counts for the
// query when K1 marked it BDX_CLS_NORMAL_LEFT (each normal pair once, by its leftmost mate) and its fragment [s + 1, s + |isize|]
// (s = 0-based pos) covers p and p + 1 of at least one of the junctions.  A normal pair's |isize| never exceeds lmax (the largest
// library cutoff, and -m: host side), so only reads with s in [p + 1 - lmax, p - 1] can cover p.  The two junctions' windows are
// walked as one when they overlap; otherwise separately, and then a read of the first window cannot reach b, nor one of the second a.
//
// KS -- alternate-supporting read pairs at given SV sites (bdx_count_site_pairs; the DV column of the CLI's --sites).
// A site is (tid1, pos1, tid2, pos2, flag_mask), positions 1-based, (tid1, pos1) <= (tid2, pos2).  Record i counts when K1 let it pass and
// its ReadFlag (after the pass-2 remaps) is in flag_mask, it is its pair's lower mate, and it is near pos1 with its mate near pos2
// (forward) or near pos2 with its mate near pos1 (reverse); one that matches both ways counts once.  Only the record's own fields are
// looked at.  SiteRule holds the rule and the window it needs.
//
// KI -- breakpoint intervals of given SV sites from their supporting pairs (bdx_site_breakpoint_bounds; CIPOS / CIEND of the CLI's --ci).
// The records that count for a site are KS's, all keys pooled.  Each gives one observation per end: (x, reverse, U) with x the 0-based
// start of the read on that end, reverse its strand bit (inverted with -l) and U its library's insert-size bound.  The read lies wholly on
// one side of the breakpoint its fragment crosses and the fragment reaches no further than U from the read's start: with P = x + 1 a
// forward read bounds the breakpoint to [P, P + U], a reverse read to [P - U, P].  lo = the maximum of the lower bounds, hi = the minimum
// of the upper bounds, per end, clamped to [1, 2^31 - 1] at the end; n == 0: all 0.  A record on the forward route gives (pos, 0x10) to
// end 1 and (mpos, 0x20) to end 2; one on the reverse route (mpos, 0x20) to end 1 and (pos, 0x10) to end 2.  Every lane keeps four
// running 64-bit extrema and a count, one xor-shuffle reduction closes the site, and lane 0 writes the 20-byte result.  No LDS.
//
// KM -- mapping quality at one end of given SV sites (bdx_site_end_quality; the SQ* / LQ* keys of the CLI's --mapq).
// A query is (site, end); the wave walks the ONE window (T, [P - 1 - window, P - 1 + window]) of the asked end.  Every record inside gives
// its SAM flag and its quality: two ballots count the records around the end (0x4 clear) and the low ones among them (quality <= the
// library's minimum; the library column and the table of minima are read only when there are several libraries).  A record whose class byte
// passes the site's mask also gives its mate columns, and when the mate is near the other end -- no lower-mate condition: each mate counts
// at its own end -- its quality goes into the wave's own row of a [4][256]-word LDS histogram, one LDS atomic.  Selection: lane l owns bins
// 4l .. 4l + 3 (one 16-byte LDS load), one inclusive wave scan of the lane totals gives the first lane whose running count reaches a rank,
// that lane resolves the rank among its four bins, and qmin / qmax are the first / last non-empty bin.  Lane 0 writes the 16-byte result.
// The kernel has no workgroup barrier (a wave without a query leaves at once): a wave touches no row but its own, once, and what orders its
// clear, its atomics and its reads is written out (km_wave_order).
#include <hip/hip_runtime.h>

#include "../../include/bdx.h"
#include "bdx_dev.h"
#include "bdx_scan.h"
#include "bdx_shard.h"
#include "bdx_window.h"

namespace bdx {

static_assert(sizeof(KsSite) == sizeof(bdx_site) && sizeof(KsSite) == 20, "KsSite is bdx_site");
static_assert(sizeof(KiBounds) == sizeof(bdx_site_bounds) && sizeof(KiBounds) == 20, "KiBounds is bdx_site_bounds");
static_assert(sizeof(KmQuality) == sizeof(bdx_site_quality) && sizeof(KmQuality) == 16 && alignof(KmQuality) == 4, "KmQuality is bdx_site_quality");

namespace {

constexpr int kQueryWaves = 4;
constexpr int64_t kKiNone = (int64_t)1 << 62;   // (beyond every bound: |P| < 2^31, U <= 2^30)

__device__ __forceinline__ bool k8_covers(int64_t s, int64_t L, int64_t p) { return s + 1 <= p && p + 1 <= s + L; }

__device__ __forceinline__ int64_t ki_clamp(int64_t v) { return v < 1 ? 1 : (v > 2147483647ll ? 2147483647ll : v); }

__global__ __launch_bounds__(kQueryWaves * 64) void k8_junction_kernel(K8Params p) {
    extern __shared__ uint32_t s_cnt[];   // [kQueryWaves][nkeys] (nkeys > 1 only)
    const StoreView& v = p.st;
    const uint32_t q = blockIdx.x * kQueryWaves + (uint32_t)wave_id();
    const bool live = q < p.nq;   // (wave-uniform: every wave reaches the counters' barriers)
    WaveKeyCounts kc;
    kc.open(s_cnt, p.nkeys);
    if (live && p.lmax >= 2 && v.n) {
        const int32_t t = p.q_tid[q];
        const int64_t a = p.q_a[q], b = p.q_b[q], lm = p.lmax;
        // windows of read starts: [a + 1 - lm, a - 1] and [b + 1 - lm, b - 1], as one when they overlap or touch
        const bool merged = b + 1 - lm <= a;
        const int nwin = merged ? 1 : 2;
        for (int wi = 0; wi < nwin; ++wi) {
            const int64_t wlo = (wi == 0 ? a : b) + 1 - lm, whi = (wi == 0 && !merged ? a : b) - 1;
            const bool test_a = wi == 0, test_b = merged || wi == 1;
            wave_window_walk(v.tid, v.pos, v.n, t, wlo, whi, [&](uint64_t i, int64_t s, bool in) {
                bool hit = false;
                if (in && (v.cls[i] & BDX_CLS_NORMAL_LEFT)) {
                    const int64_t z = v.isize[i], L = z < 0 ? -z : z;
                    hit = (test_a && k8_covers(s, L, a)) || (test_b && k8_covers(s, L, b));
                }
                kc.add(hit, p.key, i);
            });
        }
    }
    kc.close(live, p.counts, q);
}

__global__ __launch_bounds__(kQueryWaves * 64) void ks_sites_kernel(KsParams p) {
    extern __shared__ uint32_t s_cnt[];   // [kQueryWaves][nkeys] (nkeys > 1 only)
    const StoreView& v = p.st;
    const uint32_t q = blockIdx.x * kQueryWaves + (uint32_t)wave_id();
    const bool live = q < p.nq;   // (wave-uniform: every wave reaches the counters' barriers)
    WaveKeyCounts kc;
    kc.open(s_cnt, p.nkeys);
    if (live && v.n) {
        const SiteRule site(p.sites[q], p.window);
        wave_window_walk(v.tid, v.pos, v.n, site.t1, site.wlo, site.whi, [&](uint64_t i, int64_t s, bool in) {
            kc.add(in && site.match(v, i, s).route != kSiteNone, p.key, i);
        });
    }
    kc.close(live, p.counts, q);
}

__global__ __launch_bounds__(kQueryWaves * 64) void ki_bounds_kernel(KiParams p) {
    const StoreView& v = p.st;
    const uint32_t q = blockIdx.x * kQueryWaves + (uint32_t)wave_id();
    if (q >= p.nq) return;   // (wave-uniform; the kernel has no barrier)
    int64_t lo1 = -kKiNone, hi1 = kKiNone, lo2 = -kKiNone, hi2 = kKiNone;
    uint32_t cnt = 0;
    if (v.n) {
        const SiteRule site(p.sites[q], p.window);
        const bool many = p.nlibs > 1;
        wave_window_walk(v.tid, v.pos, v.n, site.t1, site.wlo, site.whi, [&](uint64_t i, int64_t s, bool in) {
            if (!in) return;
            const SiteMatch m = site.match(v, i, s);
            if (m.route == kSiteNone) return;
            int64_t U = p.u0;
            if (many) {
                uint32_t l = p.lib[i];
                l = l < (uint32_t)p.nlibs ? l : 0u;   // (an index out of range is library 0, like everywhere in the store)
                U = p.utab[l];
            }
            const bool fwd = m.route == kSiteForward;
            const bool r_own = ((m.fl & 0x10) != 0) != (p.long_insert != 0), r_mate = ((m.fl & 0x20) != 0) != (p.long_insert != 0);
            const int64_t P1 = (fwd ? s : m.ms) + 1, P2 = (fwd ? m.ms : s) + 1;
            const bool r1 = fwd ? r_own : r_mate, r2 = fwd ? r_mate : r_own;
            const int64_t a1 = r1 ? P1 - U : P1, b1 = r1 ? P1 : P1 + U;
            const int64_t a2 = r2 ? P2 - U : P2, b2 = r2 ? P2 : P2 + U;
            lo1 = a1 > lo1 ? a1 : lo1; hi1 = b1 < hi1 ? b1 : hi1;
            lo2 = a2 > lo2 ? a2 : lo2; hi2 = b2 < hi2 ? b2 : hi2;
            ++cnt;
        });
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long a = __shfl_xor((long long)lo1, o), b = __shfl_xor((long long)hi1, o);
        const long long c = __shfl_xor((long long)lo2, o), d = __shfl_xor((long long)hi2, o);
        lo1 = a > lo1 ? a : lo1; hi1 = b < hi1 ? b : hi1;
        lo2 = c > lo2 ? c : lo2; hi2 = d < hi2 ? d : hi2;
        cnt += __shfl_xor(cnt, o);
    }
    if (lane_id() == 0) {
        KiBounds r{};
        r.n = cnt;
        if (cnt) { r.lo1 = (int32_t)ki_clamp(lo1); r.hi1 = (int32_t)ki_clamp(hi1); r.lo2 = (int32_t)ki_clamp(lo2); r.hi2 = (int32_t)ki_clamp(hi2); }
        p.out[q] = r;
    }
}

// What orders one wave's accesses to its own histogram row: the row's clear before its atomics, the atomics before the reads.  The LDS
// serves one wave's operations in the order they were issued, so no wait is needed -- the reads' own wait covers what was issued before
// them -- but the compiler must keep that order: a wavefront-scope fence pins the memory operations, the wave barrier (no instruction)
// keeps the lanes' code from being moved across it.
__device__ __forceinline__ void km_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the smallest bin b of the wave's histogram with #(quality <= b) >= rank (1 <= rank <= n): inc is the inclusive scan of the lanes'
// totals, b0..b3 the lane's own bins 4 lane .. 4 lane + 3.  The same value in all lanes.
__device__ __forceinline__ uint32_t km_select(uint64_t rank, uint32_t inc, uint32_t tot, uint32_t b0, uint32_t b1, uint32_t b2) {
    const int owner = __builtin_ctzll(ballot64((uint64_t)inc >= rank));   // (rank <= n = lane 63's inc: some lane reaches it)
    const uint64_t c0 = (uint64_t)(inc - tot) + b0, c1 = c0 + b1, c2 = c1 + b2;
    const uint32_t k = c0 >= rank ? 0u : c1 >= rank ? 1u : c2 >= rank ? 2u : 3u;
    return (uint32_t)__shfl((int)(4u * (uint32_t)lane_id() + k), owner);
}

__global__ __launch_bounds__(kQueryWaves * 64) void km_quality_kernel(KmParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[kQueryWaves][256];
    const StoreView& v = p.st;
    const uint32_t q = blockIdx.x * kQueryWaves + (uint32_t)wave_id();
    if (q >= p.nq) return;   // (wave-uniform; the kernel has no workgroup barrier)
    const int lane = lane_id();
    uint32_t* row = s_hist[wave_id()];
    uint4* mine = (uint4*)(row + 4 * lane);
    *mine = uint4{0u, 0u, 0u, 0u};
    km_wave_order();
    uint32_t n_all = 0, n_low = 0;
    if (v.n) {
        const KsSite st = p.sites[q];
        const bool second = p.end[q] == 2;
        const int32_t T = second ? st.tid2 : st.tid1, To = second ? st.tid1 : st.tid2;
        const int64_t P = second ? st.pos2 : st.pos1, Po = second ? st.pos1 : st.pos2, win = p.window;
        const uint32_t mask = st.flag_mask;
        const bool many = p.nlibs > 1;
        // (in: tid == T and P - 1 - win <= pos <= P - 1 + win, which is NEAR P on T)
        wave_window_walk(v.tid, v.pos, v.n, T, P - 1 - win, P - 1 + win, [&](uint64_t i, int64_t, bool in) {
            bool around = false, low = false, sup = false;
            uint32_t qual = 0;
            if (in) {
                around = (v.flag[i] & 0x4u) == 0;
                qual = p.mapq[i];
                int32_t least = p.q0;
                if (many) {
                    uint32_t l = p.lib[i];
                    l = l < (uint32_t)p.nlibs ? l : 0u;   // (an index out of range is library 0, like everywhere in the store)
                    least = p.qtab[l];
                }
                low = around && (int32_t)qual <= least;
                const uint32_t c = v.cls[i];
                if ((c & BDX_CLS_PASS) && ((mask >> BDX_CLS_FLAG(c)) & 1u)) sup = site_near(v.mtid[i], v.mpos[i], To, Po, win);
            }
            n_all += (uint32_t)popc64(ballot64(around));
            n_low += (uint32_t)popc64(ballot64(low));
            if (sup) atomicAdd(&row[qual], 1u);   // (qual < 256: a byte)
        });
    }
    km_wave_order();
    const uint4 b = *mine;
    const uint32_t tot = b.x + b.y + b.z + b.w;
    const uint32_t inc = wave_incl_scan_t<uint32_t>(tot);
    const uint32_t n = (uint32_t)__shfl((int)inc, 63);
    KmQuality r{};
    r.n = n; r.n_all = n_all; r.n_low = n_low;
    if (n) {   // (wave-uniform)
        const uint64_t filled = ballot64(tot != 0);
        const int first = __builtin_ctzll(filled), last = 63 - __builtin_clzll(filled);
        const uint32_t lo = 4u * (uint32_t)lane + (b.x ? 0u : b.y ? 1u : b.z ? 2u : 3u), hi = 4u * (uint32_t)lane + (b.w ? 3u : b.z ? 2u : b.y ? 1u : 0u);
        r.qmin = (uint8_t)__shfl((int)lo, first);
        r.qmax = (uint8_t)__shfl((int)hi, last);
        r.q1 = (uint8_t)km_select(((uint64_t)n + 3) / 4, inc, tot, b.x, b.y, b.z);
        r.median = (uint8_t)km_select(((uint64_t)n + 1) / 2, inc, tot, b.x, b.y, b.z);
    }
    if (lane == 0) p.out[q] = r;
}

// a wave per query; the counting kernels' LDS: one row of nkeys words per wave when there are several keys
template <class P>
void launch_query(void (*kernel)(P), const P& p, int nkeys, hipStream_t s) {
    if (!p.nq) return;
    const size_t lds = nkeys > 1 ? (size_t)kQueryWaves * nkeys * 4 : 0;
    hipLaunchKernelGGL(kernel, dim3((p.nq + kQueryWaves - 1) / kQueryWaves), dim3(kQueryWaves * 64), lds, s, p);
}

}  // namespace

void launch_k8(const K8Params& p, hipStream_t s) { launch_query(k8_junction_kernel, p, p.nkeys, s); }
void launch_ks(const KsParams& p, hipStream_t s) { launch_query(ks_sites_kernel, p, p.nkeys, s); }
void launch_ki(const KiParams& p, hipStream_t s) { launch_query(ki_bounds_kernel, p, 1, s); }
void launch_km(const KmParams& p, hipStream_t s) { launch_query(km_quality_kernel, p, 1, s); }   // (its histogram is static LDS)

}  // namespace bdx

// (bdx_warm_up: the HIP runtime loads a translation unit's device code at the first launch of any of its kernels)
__global__ void kq_noop_kernel() {}
namespace bdx { void warm_kq(hipStream_t s) { hipLaunchKernelGGL(kq_noop_kernel, dim3(1), dim3(64), 0, s); } }
