// K4 -- mate join and region x region connection groups.
//
// Replaces (reference file:line under src/lib/breakdancer):
//   ReadRegionData.cpp:108-113   _read_regions[qname] -> [region ids]; 2nd sighting increments an edge
//   ReadRegionData.cpp:177-199   collapse: names of reads in rejected candidates are forgotten
//   SvBuilder.cpp:101-118        _observe_read: pair mates by name; the *second observed* mate decides
//                                flag, library and |isize| of the pair
//
// A pair exists iff both mates sit in accepted regions.  Up to kDirectJoinMax entries meet in one
// open-addressing table in HBM; beyond that they are partitioned by a hash of the name key into buckets
// that fit an LDS table (160 KiB per CU on gfx950) and each bucket is joined by one workgroup with open
// addressing in LDS.  The pairs are aggregated per (region_lo, region_hi, flag, library) by K6; the edge
// weight of the reference's graph is the sum of a group's pair counts.
#include "bdx_k3.h"
#include "bdx_scan.h"

namespace bdx {

__device__ __forceinline__ uint64_t mix64(uint64_t h) {
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}
__device__ __forceinline__ uint32_t bucket_of(uint64_t h, uint32_t log2b) { return log2b ? (uint32_t)(h >> (64 - log2b)) : 0u; }

constexpr int kPartChunk = 512;   // compact reads per workgroup in the partition kernels (>= 1 workgroup per CU at 150 k reads)

__global__ __launch_bounds__(256) void k4_count_kernel(K4Arrays k4, Entries en, const uint32_t* n_ptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* s_h = (uint32_t*)smem;
    const uint32_t na = *n_ptr;
    const uint32_t base = blockIdx.x * kPartChunk;
    if (base >= na) return;
    for (uint32_t b = threadIdx.x; b < k4.nbuckets; b += 256) s_h[b] = 0;
    __syncthreads();
    for (int it = 0; it < kPartChunk / 256; ++it) {
        const uint32_t j = base + it * 256 + threadIdx.x;
        if (j < na) atomicAdd(&s_h[bucket_of(mix64(en.key[j]), k4.log2b)], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < k4.nbuckets; b += 256)
        if (s_h[b]) atomicAdd(&k4.bcnt[b], s_h[b]);
}

__global__ __launch_bounds__(1024) void k4_bucket_scan_kernel(K4Arrays k4, StageCounts* counts) {
    __shared__ uint32_t s_ws[16];
    __shared__ uint32_t s_carry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < k4.nbuckets; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < k4.nbuckets ? k4.bcnt[i] : 0u;
        const uint32_t inc = wave_incl_scan(v);
        if (lane == 63) s_ws[w] = inc;
        __syncthreads();
        uint32_t off = s_carry;
        for (int k = 0; k < w; ++k) off += s_ws[k];
        if (i < k4.nbuckets) { k4.boff[i] = off + inc - v; k4.bcur[i] = 0; k4.bcnt[i] = 0; }  // bcnt is left clean for the next run
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = off + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) { k4.boff[k4.nbuckets] = s_carry; counts->n_entries = s_carry; }
}

__global__ __launch_bounds__(256) void k4_scatter_kernel(K4Arrays k4, Entries en, const uint32_t* n_ptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* s_h = (uint32_t*)smem;
    uint32_t* s_base = s_h + k4.nbuckets;
    const uint32_t na = *n_ptr;
    const uint32_t base = blockIdx.x * kPartChunk;
    if (base >= na) return;
    for (uint32_t b = threadIdx.x; b < k4.nbuckets; b += 256) s_h[b] = 0;
    __syncthreads();
    for (int it = 0; it < kPartChunk / 256; ++it) {
        const uint32_t j = base + it * 256 + threadIdx.x;
        if (j < na) atomicAdd(&s_h[bucket_of(mix64(en.key[j]), k4.log2b)], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < k4.nbuckets; b += 256) {
        const uint32_t c = s_h[b];
        if (c) s_base[b] = k4.boff[b] + atomicAdd(&k4.bcur[b], c);
        s_h[b] = 0;
    }
    __syncthreads();
    for (int it = 0; it < kPartChunk / 256; ++it) {
        const uint32_t j = base + it * 256 + threadIdx.x;
        if (j < na) {
            const uint64_t key = en.key[j];
            const uint32_t b = bucket_of(mix64(key), k4.log2b);
            const uint32_t slot = s_base[b] + atomicAdd(&s_h[b], 1u);
            k4.e_key[slot] = key;
            k4.e_idx[slot] = j;
        }
    }
}

// One workgroup joins one bucket.  Two phases around a barrier: (A) every entry claims its own slot by
// linear probing from hash(key) (no key comparison, so the table is a multiset), (B) every entry walks its
// probe run until the first empty slot and takes the other entry with the same key as its mate.
constexpr uint32_t kMaxProbes = 4096;  // a name key shared by thousands of reads is malformed input: fail instead of crawling

template <bool kLds>
__device__ __forceinline__ void join_bucket(uint64_t* tkey, int32_t* tidx, uint32_t cap, const K4Arrays& k4, const int32_t* region,
                                            const uint64_t* check, uint32_t off, uint32_t cnt, StageCounts* counts) {
    for (uint32_t s = threadIdx.x; s < cap; s += blockDim.x) tidx[s] = -1;
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < cnt; e += blockDim.x) {
        const uint64_t key = k4.e_key[off + e];
        const int32_t j = (int32_t)k4.e_idx[off + e];
        uint32_t s = (uint32_t)(mix64(key) & 0xffffffffu) % cap;
        uint32_t probes = 0;
        bool placed = true;
        while (atomicCAS(&tidx[s], -1, j) != -1) {
            s = s + 1 == cap ? 0 : s + 1;
            if (++probes > kMaxProbes) { placed = false; break; }
        }
        if (placed) tkey[s] = key;
        else counts->irregular = 1;
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < cnt; e += blockDim.x) {
        const uint64_t key = k4.e_key[off + e];
        const int32_t j = (int32_t)k4.e_idx[off + e];
        uint32_t s = (uint32_t)(mix64(key) & 0xffffffffu) % cap;
        int32_t mate = -1;
        const uint32_t lim = cap < kMaxProbes ? cap : kMaxProbes;
        for (uint32_t probes = 0; probes < lim; ++probes) {  // to the end of the probe run: a second match is a name seen three times
            const int32_t o = tidx[s];
            if (o == -1) break;
            if (o != j && tkey[s] == key && (!check || check[o] == check[j])) {  // (equal keys of two different names: not mates)
                if (mate != -1) counts->irregular = 1;
                mate = o;
            }
            s = s + 1 == cap ? 0 : s + 1;
        }
        if (mate >= 0 && (region[j] < 0 || region[mate] < 0)) mate = -2;  // a mate in a rejected candidate: the name was forgotten
        k4.partner[j] = mate;
    }
}

__global__ __launch_bounds__(256) void k4_join_kernel(K4Arrays k4, const int32_t* region, const uint64_t* check, StageCounts* counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t b = blockIdx.x;
    const uint32_t off = k4.boff[b], cnt = k4.boff[b + 1] - off;
    if (cnt == 0) return;
    if (2 * cnt <= (uint32_t)kJoinLdsSlots) {
        uint64_t* tkey = (uint64_t*)smem;
        int32_t* tidx = (int32_t*)(tkey + kJoinLdsSlots);
        join_bucket<true>(tkey, tidx, 2 * cnt, k4, region, check, off, cnt, counts);
    } else {
        join_bucket<false>(k4.t_key + 2 * (size_t)off, k4.t_idx + 2 * (size_t)off, 2 * cnt, k4, region, check, off, cnt, counts);
    }
}

// Direct path: one table of 64-bit words (hash tag << 32 | entry index) for all entries, one launch.  The first mate
// to arrive claims the first free slot of its probe sequence; the second walks the same sequence, meets that word
// (slots are never freed), confirms the full key and records the pair for both.  At the sizes of one chromosome the
// table (8 B per slot, load <= 0.25) lives in L2 / Infinity Cache, and the partitioning launches of the bucketed
// path are not worth their latency.  partner[] must be -1 and the table all ones on entry.
constexpr uint32_t kJoinForwardBlocks = 32;
constexpr uint32_t kJoinForwardAhead = 4;   // 16-byte words a forwarding lane requests per turn (a turn of all of them: kJoinForwardBlocks * 256 * this many words)

// dst[0 .. quads) = src[0 .. quads), thread t of gsz: a turn's loads are all issued before its stores, and the NEXT turn's loads before them too.
// The stores go over the link; vmcnt counts them with the loads and retires in order, so a load issued behind a store waits for that store's
// acknowledgement -- copied word by word, a wave had one store in flight.  (Past the end a lane reads the last word again and stores nothing.)
__device__ __forceinline__ void forward_quads(uint4* dst, const uint4* src, uint32_t quads, uint32_t t, uint32_t gsz) {
    if (quads == 0) return;
    static_assert(kJoinForwardAhead == 4, "four named words (an array of them is kept in scratch memory)");
    const uint32_t last = quads - 1u;
    uint4 c0 = src[min(t, last)], c1 = src[min(t + gsz, last)], c2 = src[min(t + 2 * gsz, last)], c3 = src[min(t + 3 * gsz, last)];
    uint32_t i = t;
    for (; i + 3 * gsz < quads; i += 4 * gsz) {   // whole turns: no branch around a store, so the waits at the loop's end can be counted ones
        const uint4 n0 = src[min(i + 4 * gsz, last)], n1 = src[min(i + 5 * gsz, last)], n2 = src[min(i + 6 * gsz, last)], n3 = src[min(i + 7 * gsz, last)];
        dst[i] = c0; dst[i + gsz] = c1; dst[i + 2 * gsz] = c2; dst[i + 3 * gsz] = c3;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    if (i < quads) dst[i] = c0;   // the last, partial turn
    if (i + gsz < quads) dst[i + gsz] = c1;
    if (i + 2 * gsz < quads) dst[i + 2 * gsz] = c2;
}
__global__ __launch_bounds__(256) void k4_direct_join_kernel(K4Arrays k4, Entries en, const uint32_t* n_ptr, StageCounts* counts) {
    const uint32_t na = *n_ptr;
    // The region table's way to the host (single-context runs: the host's share of the walk reads it): kJoinForwardBlocks workgroups IN FRONT
    // of the joining ones do nothing else.  When every joining wave forwarded a few words before its own work, those stores -- 5.7 MB at a
    // genome share, 110 us of link time -- sat in front of every wave's loads: 6 us for a coalesced load at the median, 145 us for a launch
    // that takes 94 by itself (profiles/r06_join_kernel.txt).  32 workgroups keep the link busy (16 bytes per lane in flight); they are
    // dispatched first and run beside the join.
    const uint32_t fwd = en.r_rec_host ? kJoinForwardBlocks : 0u;
    if (blockIdx.x < fwd) {
        const uint32_t nr = en.counts->n_regions;
        const uint32_t t = blockIdx.x * 256 + threadIdx.x, gsz = fwd * 256;
        constexpr uint32_t kw = sizeof(RegionRec) / 4;
        {
            const uint32_t words = nr * kw, quads = words / 4;   // (the tables start on 256-byte boundaries)
            forward_quads((uint4*)en.r_rec_host, (const uint4*)en.r_rec_dev, quads, t, gsz);
            if (t < words - quads * 4) ((uint32_t*)en.r_rec_host)[quads * 4 + t] = ((const uint32_t*)en.r_rec_dev)[quads * 4 + t];
        }
        {
            const uint32_t words = nr * (uint32_t)en.nkeys2, quads = words / 4;
            forward_quads((uint4*)en.r_pk_host, (const uint4*)en.r_pk_dev, quads, t, gsz);
            if (t < words - quads * 4) en.r_pk_host[quads * 4 + t] = en.r_pk_dev[quads * 4 + t];
        }
    }
    // (a forwarding workgroup holds no entry: it leaves at the bound check below.  Leaving right after the copy instead cost the kernel
    // 17 more SGPRs, and a wave slot per SIMD)
    const uint32_t j = blockIdx.x < fwd ? 0xFFFFFFFFu : (blockIdx.x - fwd) * 256 + threadIdx.x;
    const uint32_t kp = (blockIdx.x - fwd) * 4 + (threadIdx.x >> 6);   // (measurement build: this wave's row of clocks)
    (void)kp;
    KPROF(kp, 0);
    KPROF(kp, 1);
    if (j >= na) return;
    // (sharded runs: the entries behind the context's own are foreign -- see Entries::n_local)
    const uint32_t nl = en.n_local ? *en.n_local : na;
    const bool jf = j >= nl;
    int rj;
    if (jf) {
        rj = en.fregion[j - nl];
    } else if (en.c_rid) {
        rj = en.c_rid[en.cand[j]];
        en.region_out[j] = rj;
        if (en.k6_scratch) {  // out_deg, label, bad_v, bad, mcount, pcount
            const size_t cap = en.scratch_cap;
            en.k6_scratch[j] = 0; en.k6_scratch[cap + j] = j; en.k6_scratch[2 * cap + j] = 0; en.k6_scratch[3 * cap + j] = 0;
            en.k6_scratch[4 * cap + j] = 0; en.k6_scratch[5 * cap + j] = 0;
        }
    } else {
        rj = en.region[j];
    }
    // (a read of a rejected candidate joins the table as well: it never forms a pair, but a third sighting of its name
    // must be noticed wherever the three reads lie)
    const uint64_t key = jf ? en.fkey[j - nl] : en.key[j];
    const uint64_t chk = en.check ? (jf ? en.fcheck[j - nl] : en.check[j]) : 0ull;
    const uint64_t h = mix64(key);
    if (key != 0x5555AAAA5555AAAAull) KPROF(kp, 2);   // (the key and the region have arrived)
    const uint32_t tag = (uint32_t)(h >> 32);
    unsigned long long* table = (unsigned long long*)k4.t_key;
    const unsigned long long mine = ((unsigned long long)tag << 32) | j;
    uint32_t s = (uint32_t)h & k4.t_mask;
    for (uint32_t probes = 0; probes <= kMaxProbes; ++probes) {
        const unsigned long long old = atomicCAS(&table[s], ~0ull, mine);
        if (probes == 0 && old != 0x5555AAAA5555AAAAull) KPROF(kp, 3);   // (lane 0's first compare-and-swap is back)
        if (old == ~0ull) return;  // first of its name so far
        if ((uint32_t)(old >> 32) == tag) {
            const uint32_t o = (uint32_t)old;
            const bool of = o >= nl;
            const uint64_t okey = of ? en.fkey[o - nl] : en.key[o];
            if (okey == key && (!en.check || (of ? en.fcheck[o - nl] : en.check[o]) == chk)) {  // (equal keys of two different names: probe on)
                const int ro = of ? en.fregion[o - nl] : (en.c_rid ? en.c_rid[en.cand[o]] : en.region[o]);
                const bool alive = rj >= 0 && ro >= 0;  // both mates in accepted regions (ReadRegionData.cpp:177-199)
                if (!jf) k4.partner[j] = alive ? (int32_t)o : -2;
                if (!of && atomicExch(&k4.partner[o], alive ? (int32_t)j : -2) != -1) counts->irregular = 1;  // a third read with this name
                if (alive && k4.pair_lo) {  // the later read in stream order is the second-observed mate
                    if (jf != of) {          // (a foreign entry lies on an earlier chromosome: the context's own read is the later one)
                        if (jf) k4.pair_lo[o] = rj; else k4.pair_lo[j] = ro;
                    } else if (!jf) {
                        if (o < j) k4.pair_lo[j] = ro;
                        else k4.pair_lo[o] = rj;
                    }
                }
                KPROF(kp, 4);   // (lane 0 was a second mate: its partner's key, region and the exchange are done)
                return;
            }
        }
        s = (s + 1) & k4.t_mask;
    }
    counts->irregular = 1;  // (a probe sequence this long: thousands of reads share one name)
}

// mate join only: the pair groups are formed per region by K6
void launch_k4_join_only(const K4Arrays& k4, const Entries& en, const uint32_t* n_ptr, uint32_t n_anom_host, StageCounts* counts,
                         hipStream_t s) {
    if (n_anom_host == 0) return;
    const uint32_t g = (n_anom_host + kPartChunk - 1) / kPartChunk;
    if (k4.direct) {
        const uint32_t gd = (n_anom_host + 255) / 256 + (en.r_rec_host ? kJoinForwardBlocks : 0u);
        hipLaunchKernelGGL(k4_direct_join_kernel, dim3(gd), dim3(256), 0, s, k4, en, n_ptr, counts);
        return;
    }
    // bcnt is zero on entry (zeroed at allocation, then by every bucket scan); partner[] needs no initialisation: the join
    // kernel writes the entry of every read of an accepted region and nothing else is ever read
    hipLaunchKernelGGL(k4_count_kernel, dim3(g), dim3(256), (size_t)k4.nbuckets * 4, s, k4, en, n_ptr);
    hipLaunchKernelGGL(k4_bucket_scan_kernel, dim3(1), dim3(1024), 0, s, k4, counts);
    hipLaunchKernelGGL(k4_scatter_kernel, dim3(g), dim3(256), (size_t)k4.nbuckets * 8, s, k4, en, n_ptr);
    static bool attr_set = false;
    if (!attr_set) {  // more than 64 KiB of dynamic LDS has to be opted into
        (void)hipFuncSetAttribute((const void*)k4_join_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kJoinLdsSlots * 12);
        attr_set = true;
    }
    hipLaunchKernelGGL(k4_join_kernel, dim3(k4.nbuckets), dim3(256), (size_t)kJoinLdsSlots * 12, s, k4, en.region, en.check, counts);
}

}  // namespace bdx

// (bdx_warm_up: the HIP runtime loads a translation unit's device code at the first launch of any of its kernels)
__global__ void k4_noop_kernel() {}
namespace bdx { void warm_k4(hipStream_t s) { hipLaunchKernelGGL(k4_noop_kernel, dim3(1), dim3(64), 0, s); } }

#ifdef BDX_KPROF
extern "C" int bdx_debug_kprof4(unsigned long long* out, size_t n) {
    const int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(bdx::g_kprof), n * sizeof(unsigned long long));
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(bdx::g_kprof)) == hipSuccess) (void)hipMemset(p, 0, sizeof(unsigned long long) * 8 * 65536);
    return rc;
}
#endif
