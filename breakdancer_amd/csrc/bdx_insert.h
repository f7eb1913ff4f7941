// The order-key insertion merge of K6 (k6_insert_kernel, k6_ranksort_kernel) with its constants, its bucket function and the two
// launches, in a header of its own: k6_assemble.hip includes it for the product, tests/prims/prims.hip includes it unchanged and
// holds every ranking route to a plain stable merge at the sizes where the routes change (tests/test_gpu_insert.py).
#pragma once
#include "bdx_k3.h"
#include "bdx_scan.h"

namespace bdx {

// (the order key of a candidate that is placed by key, its constants and the bounds of its sequence number: bdx_k3.h.  The rank and bucket
// routes of the merge below assume keys that differ; k6_ranksort_kernel alone settles equal keys by index.)

__device__ __forceinline__ uint32_t count_below(const uint32_t* v, uint32_t n, uint32_t x) {  // #elements < x, v ascending
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t count_below64(const uint64_t* v, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The candidates that are placed by order key -- the host walk's list (sorted, pinned host memory) and the device's
// candidates from traversals started at a vertex of an earlier window (k6_walk_kernel's list, any order) -- merged into
// one list sorted by key, with the running totals of their list entries.  One workgroup of 1,024 threads (k6_insert_kernel): sort the
// device's list (by rank counting up to 1,024 entries, bitonic in LDS up to 2,048; a longer list arrives with its ranks counted by the
// whole GPU, k6_ranksort_kernel, launched behind the device walk so that it runs beside the host's), then every entry finds its place by a
// binary search in the other list (no key occurs in both: a start vertex belongs to one component, and that is walked either here or by the host).
// Round 6: lists of 1,025..8,192 device entries (a GPU's share of a genome has ~6 k) are ranked inside this launch through BUCKETS of the
// keys' flush threshold -- a histogram in LDS, its running sums, every entry compared with its own bucket's few others: 127 us of rank-sort
// launch + one workgroup adding up ten partial ranks per entry became one pass over keys that stay in LDS (profiles/r06_insert_buckets.txt).
// A list whose keys crowd into one bucket (kInsBucketDepth) takes the old bitonic sort.
constexpr uint32_t kInsLds = 2048;
constexpr uint32_t kInsThreads = 1024;
constexpr uint32_t kInsBucketMax = 8192;     // device entries the bucket path takes
constexpr uint32_t kInsCntLds = 10240;       // merged entries whose counts stay in LDS
constexpr uint32_t kInsBuckets = 2048;
constexpr uint32_t kInsBucketDepth = 128;    // entries of one bucket beyond which the bucket path gives up
constexpr uint32_t kInsPerBucketPath = kInsBucketMax / kInsThreads;
constexpr uint32_t kInsSub = 64;             // sub-slots of one flush window in the bucket function
constexpr uint32_t kRankGrid = 256;          // workgroups of k6_ranksort_kernel
// how k6_ranksort_kernel cuts its work for a list of nd entries: chunks of 256 entries x slices of the list they are compared against
__device__ __forceinline__ void rank_layout(uint32_t nd, uint32_t* nchunk, uint32_t* nslice, uint32_t* per) {
    *nchunk = (nd + kScanBlock - 1) / kScanBlock;
    *nslice = min(kK6RankSlices, max(1u, kRankGrid / *nchunk));
    *per = (nd + *nslice - 1) / *nslice;
}

// An entry's bucket is a monotone function of its key (so a bucket's entries lie between its neighbours') that spreads what the keys
// crowd around: the device's entries all carry a flush threshold T = window x period and differ in their start vertex -- mostly one of
// the window before (local links), any earlier one for translocations.  Windows x 64 sub-slots by the start vertex, scaled to kInsBuckets.
// span: ins_bucket_span() of the run's regions and the same period
__device__ __forceinline__ uint64_t ins_bucket_span(uint32_t n_regions, uint32_t period) {
    const uint32_t nwin = n_regions / period + 2;
    return (uint64_t)nwin * kInsSub + 1;
}
__device__ __forceinline__ uint32_t ins_bucket_of(uint64_t key, uint32_t period, uint64_t span) {
    constexpr uint32_t kSub = kInsSub;
    const uint32_t T = (uint32_t)(key >> kKeyShiftT), own = (uint32_t)(key >> kKeyShiftOwn) & 1u, start = (uint32_t)(key >> kKeyShiftStart) & kKeyStartMask;
    const uint32_t W = T / period, r = T - W * period;
    uint32_t sub = kSub;   // (a threshold inside a window, or a candidate of its own window: behind every entry of that flush)
    if (!r && !own) {
        if (start >= T) sub = kSub - 1;
        else if (start + period >= T) sub = kSub / 2 + min(kSub / 2 - 1, (uint32_t)(((uint64_t)(start + period - T) * (kSub / 2)) / period));
        else sub = (uint32_t)(((uint64_t)start * (kSub / 2)) / T);
    }
    return (uint32_t)min((uint64_t)(kInsBuckets - 1), (((uint64_t)W * kSub + sub) * kInsBuckets) / span);
}

struct InsertJob {
    K6Arrays a;
    __device__ void operator()() const;
};

__device__ void InsertJob::operator()() const {
    constexpr uint32_t kThreads = kInsThreads;
    constexpr uint32_t kPer = kInsCntLds / kThreads;  // list entries per thread in the LDS prefix pass
    // One workgroup, nothing else on its compute unit: 130 of gfx950's 160 KB of LDS.  s_ord: the device's keys bucket by bucket (bucket
    // path); the other paths keep their keys, slots and rank-counting copy in it
    __shared__ uint64_t s_ord[kInsBucketMax];
    __shared__ uint32_t s_cnt[kInsCntLds];        // lib_count | cn_count << 16 of the merged list
    __shared__ uint64_t s_hk[kInsLds];
    __shared__ uint32_t s_hist[kInsBuckets + 1];
    __shared__ uint32_t s_ws[2][kThreads / 64];
    __shared__ uint32_t s_crowded;
    uint64_t* const s_dk = s_ord;
    uint32_t* const s_dv = (uint32_t*)(s_ord + kInsLds);
    uint64_t* const s_tmp = s_ord + 2 * kInsLds;
    static_assert(2 * kInsLds + kThreads <= kInsBucketMax, "keys, slots and the rank-counting copy of the smaller paths fit s_ord");
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const uint32_t nh = a.nh;
    const uint32_t nd = a.counts->n_old;
    // the host's keys and counts come over the link: ask for them before anything waits
    uint64_t* hk = nh <= kInsLds ? s_hk : a.hs_key_dev;
    for (uint32_t i = tid; i < nh; i += kThreads) hk[i] = a.hs_key[i];
    uint32_t hc[kInsLds / kThreads];   // (the counts of this thread's host entries on the bucket path: the same round trip over the link as the keys')
#pragma unroll
    for (uint32_t q = 0; q < kInsLds / kThreads; ++q) hc[q] = (nh <= kInsLds && tid + q * kThreads < nh) ? a.hs_cnt[tid + q * kThreads] : 0u;
    const uint32_t n = nh + nd;
    if (n > a.sv_cap) {  // cannot happen: every candidate consumes at least one read pair
        if (tid == 0) { a.counts->overflow = 1; a.counts->n_ins = 0; a.ins_pre_l[0] = 0; a.ins_pre_c[0] = 0; }
        return;
    }
    if (tid == 0) a.counts->n_ins = n;
    if (n == 0) {
        if (tid == 0) { a.ins_pre_l[0] = 0; a.ins_pre_c[0] = 0; }
        return;
    }
    const bool by_rank = nd <= kThreads;
    bool by_bucket = !by_rank && nd <= kInsBucketMax && a.ins_plain != 1;
    const bool small = n <= kInsCntLds;  // the merged list's counts stay in LDS for the running totals
    uint64_t* dk = nullptr;
    uint32_t* dv = nullptr;
    uint32_t my_cnt = 0;              // rank-sort path: lib_count | cn_count << 16 of this thread's device entry
    if (by_bucket) {
        // (the bucket function: ins_bucket_of above)
        const uint32_t period = (uint32_t)max(a.period, 1);
        const uint64_t span = ins_bucket_span(a.counts->n_regions, period);
        auto bucket_of = [&](uint64_t key) { return ins_bucket_of(key, period, span); };
        for (uint32_t i = tid; i <= kInsBuckets; i += kThreads) s_hist[i] = 0;
        if (tid == 0) s_crowded = a.ins_plain == 2 ? 1u : 0u;
        __syncthreads();
        uint64_t key[kInsPerBucketPath];
        uint32_t slot[kInsPerBucketPath], bk[kInsPerBucketPath], at[kInsPerBucketPath], cnt[kInsPerBucketPath];
#pragma unroll
        for (uint32_t k = 0; k < kInsPerBucketPath; ++k) {
            const uint32_t d = tid + k * kThreads;
            key[k] = d < nd ? a.old_key[d] : ~0ull;
            slot[k] = d < nd ? a.old_slot[d] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kInsPerBucketPath; ++k) {
            const uint32_t d = tid + k * kThreads;
            bk[k] = 0; at[k] = 0; cnt[k] = 0;
            if (d < nd) {
                cnt[k] = (uint32_t)a.sv_stage[slot[k]].sv.lib_count | ((uint32_t)a.sv_stage[slot[k]].sv.cn_count << 16);
                bk[k] = bucket_of(key[k]);
                at[k] = atomicAdd(&s_hist[bk[k]], 1u);
                if (at[k] >= kInsBucketDepth) s_crowded = 1u;
            }
        }
        __syncthreads();
        by_bucket = s_crowded == 0;   // (the same answer in every thread)
        if (by_bucket) {
            // running sums of the histogram: s_hist[b] = first place of bucket b in the bucket-ordered list, s_hist[kInsBuckets] = nd
            static_assert(kInsBuckets == 2 * kThreads, "two buckets per thread");
            const uint32_t h0 = s_hist[2 * tid], h1 = s_hist[2 * tid + 1];
            const uint32_t inc = wave_incl_scan_t(h0 + h1);
            if (lane == 63) s_ws[0][w] = inc;
            __syncthreads();
            uint32_t off = inc - (h0 + h1);
            for (int q = 0; q < w; ++q) off += s_ws[0][q];
            s_hist[2 * tid] = off; s_hist[2 * tid + 1] = off + h0;
            if (tid == 0) s_hist[kInsBuckets] = nd;
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kInsPerBucketPath; ++k)
                if (tid + k * kThreads < nd) s_ord[s_hist[bk[k]] + at[k]] = key[k];
            __syncthreads();
            auto below = [&](uint64_t x, uint32_t b) {   // keys of the device's list below x, b = x's bucket
                const uint32_t lo = s_hist[b], hi = s_hist[b + 1];
                uint32_t r = lo;
                for (uint32_t j = lo; j < hi; ++j) r += s_ord[j] < x ? 1u : 0u;
                return r;
            };
#pragma unroll
            for (uint32_t k = 0; k < kInsPerBucketPath; ++k)
                if (tid + k * kThreads < nd) {
                    const uint32_t pos = below(key[k], bk[k]) + count_below64(hk, nh, key[k]);
                    a.ins_T[pos] = (uint32_t)(key[k] >> kKeyShiftT);
                    a.ins_src[pos] = slot[k];
                    if (small) s_cnt[pos] = cnt[k];
                    else { a.ins_pre_l[pos] = cnt[k] & 0xffffu; a.ins_pre_c[pos] = cnt[k] >> 16; }
                }
            static_assert(kInsLds / kThreads == 2, "two prefetched host counts per thread");
            for (uint32_t j = tid; j < nh; j += kThreads) {
                const uint64_t x = hk[j];
                const uint32_t pos = j + below(x, bucket_of(x)), c = nh <= kInsLds ? (j < kThreads ? hc[0] : hc[1]) : a.hs_cnt[j];
                a.ins_T[pos] = (uint32_t)(x >> kKeyShiftT);
                a.ins_src[pos] = 0x80000000u | j;
                if (small) s_cnt[pos] = c;
                else { a.ins_pre_l[pos] = c & 0xffffu; a.ins_pre_c[pos] = c >> 16; }
            }
        }
        __syncthreads();   // (s_ord is the other paths' from here)
    }
    if (by_bucket) {
        // (placed above, the host's entries too)
    } else if (by_rank) {
        // one entry per thread: its rank is the number of smaller keys (all keys differ)
        dk = s_dk; dv = s_dv;
        const uint64_t key = tid < nd ? a.old_key[tid] : ~0ull;
        const uint32_t slot = tid < nd ? a.old_slot[tid] : 0u;
        if (tid < nd) my_cnt = (uint32_t)a.sv_stage[slot].sv.lib_count | ((uint32_t)a.sv_stage[slot].sv.cn_count << 16);
        s_tmp[tid] = key;
        __syncthreads();
        uint32_t rank = 0;
        for (uint32_t q = 0; q < nd; ++q) rank += s_tmp[q] < key ? 1u : 0u;
        if (tid < nd) { dk[rank] = key; dv[rank] = slot; }
        __syncthreads();
        if (tid < nd) {
            const uint32_t pos = rank + count_below64(hk, nh, key);
            a.ins_T[pos] = (uint32_t)(key >> kKeyShiftT);
            a.ins_src[pos] = slot;
            if (small) s_cnt[pos] = my_cnt;
            else { a.ins_pre_l[pos] = my_cnt & 0xffffu; a.ins_pre_c[pos] = my_cnt >> 16; }
        }
    } else if (a.rank_part && nd > kInsLds && nd <= kK6RankSortMax && (nd > kInsBucketMax || a.ins_plain == 1)) {
        // (ranked by the whole GPU in the launch before this one: a bitonic sort of this many keys in HBM by ONE workgroup took half a millisecond,
        // one workgroup per 256 entries counting against the whole list 0.4 ms at 6 k entries -- a wave's compare loop is instruction-bound)
        uint32_t nchunk, nslice, per;
        rank_layout(nd, &nchunk, &nslice, &per);
        for (uint32_t d = tid; d < nd; d += kThreads) {
            uint32_t rank = 0;
            for (uint32_t sl = 0; sl < nslice; ++sl) rank += a.rank_part[(size_t)sl * nd + d];
            a.sorted_key[rank] = a.old_key[d];
            a.sorted_slot[rank] = a.old_slot[d];
        }
        __threadfence();
        __syncthreads();
        dk = a.sorted_key; dv = a.sorted_slot;
        for (uint32_t d = tid; d < nd; d += kThreads) {
            const uint64_t key = dk[d];
            const uint32_t pos = d + count_below64(hk, nh, key), slot = dv[d];
            const uint32_t cnt = (uint32_t)a.sv_stage[slot].sv.lib_count | ((uint32_t)a.sv_stage[slot].sv.cn_count << 16);
            a.ins_T[pos] = (uint32_t)(key >> kKeyShiftT);
            a.ins_src[pos] = slot;
            if (small) s_cnt[pos] = cnt;
            else { a.ins_pre_l[pos] = cnt & 0xffffu; a.ins_pre_c[pos] = cnt >> 16; }
        }
    } else {
        uint32_t m = 1;
        while (m < nd) m <<= 1;
        if (m <= kInsLds) {
            dk = s_dk; dv = s_dv;
            for (uint32_t i = tid; i < m; i += kThreads) { dk[i] = i < nd ? a.old_key[i] : ~0ull; dv[i] = i < nd ? a.old_slot[i] : 0u; }
        } else {
            dk = a.old_key; dv = a.old_slot;
            for (uint32_t i = nd + tid; i < m; i += kThreads) dk[i] = ~0ull;
        }
        __syncthreads();
        for (uint32_t ksz = 2; ksz <= m; ksz <<= 1)
            for (uint32_t j = ksz >> 1; j > 0; j >>= 1) {
                for (uint32_t t = tid; t < m / 2; t += kThreads) {
                    const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const bool up = (lo & ksz) == 0;
                    const uint64_t x = dk[lo], y = dk[hi];
                    if ((x > y) == up) {
                        dk[lo] = y; dk[hi] = x;
                        const uint32_t vx = dv[lo];
                        dv[lo] = dv[hi]; dv[hi] = vx;
                    }
                }
                __syncthreads();
            }
        for (uint32_t d = tid; d < nd; d += kThreads) {
            const uint64_t key = dk[d];
            const uint32_t pos = d + count_below64(hk, nh, key), slot = dv[d];
            const uint32_t cnt = (uint32_t)a.sv_stage[slot].sv.lib_count | ((uint32_t)a.sv_stage[slot].sv.cn_count << 16);
            a.ins_T[pos] = (uint32_t)(key >> kKeyShiftT);
            a.ins_src[pos] = slot;
            if (small) s_cnt[pos] = cnt;
            else { a.ins_pre_l[pos] = cnt & 0xffffu; a.ins_pre_c[pos] = cnt >> 16; }
        }
    }
    for (uint32_t j = tid; j < nh && !by_bucket; j += kThreads) {
        const uint64_t key = hk[j];
        const uint32_t pos = j + count_below64(dk, nd, key), cnt = a.hs_cnt[j];
        a.ins_T[pos] = (uint32_t)(key >> kKeyShiftT);
        a.ins_src[pos] = 0x80000000u | j;
        if (small) s_cnt[pos] = cnt;
        else { a.ins_pre_l[pos] = cnt & 0xffffu; a.ins_pre_c[pos] = cnt >> 16; }
    }
    __syncthreads();
    // exclusive running totals, the grand totals at [n]
    if (small) {
        uint32_t l[kPer], c[kPer], sl = 0, sc = 0;
#pragma unroll
        for (uint32_t q = 0; q < kPer; ++q) {
            const uint32_t i = tid * kPer + q;
            const uint32_t v = i < n ? s_cnt[i] : 0u;
            l[q] = v & 0xffffu; c[q] = v >> 16;
            sl += l[q]; sc += c[q];
        }
        const uint32_t il = wave_incl_scan_t(sl), ic = wave_incl_scan_t(sc);
        if (lane == 63) { s_ws[0][w] = il; s_ws[1][w] = ic; }
        __syncthreads();
        uint32_t ol = il - sl, oc = ic - sc, tl = 0, tc = 0;
        for (int q = 0; q < (int)kThreads / 64; ++q) {
            if (q < w) { ol += s_ws[0][q]; oc += s_ws[1][q]; }
            tl += s_ws[0][q]; tc += s_ws[1][q];
        }
#pragma unroll
        for (uint32_t q = 0; q < kPer; ++q) {
            const uint32_t i = tid * kPer + q;
            if (i < n) { a.ins_pre_l[i] = ol; a.ins_pre_c[i] = oc; }
            ol += l[q]; oc += c[q];
        }
        if (tid == 0) { a.ins_pre_l[n] = tl; a.ins_pre_c[n] = tc; }
        return;
    }
    uint32_t carry_l = 0, carry_c = 0;
    for (uint32_t base = 0; base < n; base += kThreads) {
        const uint32_t i = base + tid;
        const uint32_t l = i < n ? a.ins_pre_l[i] : 0u, c = i < n ? a.ins_pre_c[i] : 0u;
        const uint32_t il = wave_incl_scan_t(l), ic = wave_incl_scan_t(c);
        if (lane == 63) { s_ws[0][w] = il; s_ws[1][w] = ic; }
        __syncthreads();
        uint32_t ol = carry_l, oc = carry_c, tl = 0, tc = 0;
        for (int q = 0; q < (int)kThreads / 64; ++q) {
            if (q < w) { ol += s_ws[0][q]; oc += s_ws[1][q]; }
            tl += s_ws[0][q]; tc += s_ws[1][q];
        }
        if (i < n) { a.ins_pre_l[i] = ol + il - l; a.ins_pre_c[i] = oc + ic - c; }
        carry_l += tl; carry_c += tc;
        __syncthreads();
    }
    if (tid == 0) { a.ins_pre_l[n] = carry_l; a.ins_pre_c[n] = carry_c; }
}

// The device's insertion list (order keys of the candidates whose traversal started in an earlier flush window, any order) ranked by
// ALL of the GPU: every entry's rank is the number of keys below its own.  n^2 comparisons -- 3.5e7 at the 6 k entries of a GPU's share of
// a genome, microseconds on 256 compute units IF they are spread: a workgroup takes 256 entries and ONE SLICE of the list (up to 16 slices
// while there are fewer chunks than workgroups), tiles of the slice pass through LDS, a broadcast read per comparison, and leaves the
// partial ranks in rank_part[slice][entry]; k6_insert_kernel adds the slices up and places the entries.  Its own launch, enqueued behind the
// device walk: it runs while the host walks its share (until round 5 these workgroups rode in k6_insert_kernel's launch, whose last
// workgroup spun until they were through: one slice per entry, 0.4 ms, on the critical path -- and a wait HIP does not promise to end).
constexpr uint32_t kRankTile = 2048;
__global__ __launch_bounds__(kScanBlock) void k6_ranksort_kernel(K6Arrays a) {
    __shared__ uint64_t s_k[kRankTile];
    const uint32_t nd = a.counts->n_old;
    if (nd <= kInsLds || nd > kK6RankSortMax) return;
    if (nd <= kInsBucketMax && a.ins_plain != 1) return;   // (k6_insert_kernel ranks these through its buckets)
    uint32_t nchunk, nslice, per;
    rank_layout(nd, &nchunk, &nslice, &per);
    for (uint32_t item = blockIdx.x; item < nchunk * nslice; item += gridDim.x) {   // (whole workgroups stay in the loop: barriers inside)
        const uint32_t chunk = item % nchunk, slice = item / nchunk;
        const uint32_t i = chunk * kScanBlock + threadIdx.x;
        const uint64_t key = i < nd ? a.old_key[i] : ~0ull;
        const uint32_t k0 = min(nd, slice * per), k1 = min(nd, k0 + per);
        uint32_t rank = 0;
        for (uint32_t t0 = k0; t0 < k1; t0 += kRankTile) {
            const uint32_t cnt = min(kRankTile, k1 - t0);
            __syncthreads();
            for (uint32_t q = threadIdx.x; q < cnt; q += kScanBlock) s_k[q] = a.old_key[t0 + q];
            __syncthreads();
            for (uint32_t q = 0; q < cnt; ++q) {
                const uint64_t k = s_k[q];
                rank += (k < key || (k == key && t0 + q < i)) ? 1u : 0u;   // (keys of one run differ; the index settles it if they ever do not)
            }
        }
        if (i < nd) a.rank_part[(size_t)slice * nd + i] = rank;
    }
}

__global__ __launch_bounds__(kInsThreads) void k6_insert_kernel(K6Arrays a) { InsertJob{a}(); }

// the two launches as the product makes them (launch_k6_walk, launch_k6_table); the rank sort only where a.rank_part is not null
inline void launch_k6_ranksort(const K6Arrays& a, hipStream_t s) { hipLaunchKernelGGL(k6_ranksort_kernel, dim3(kRankGrid), dim3(kScanBlock), 0, s, a); }
inline void launch_k6_insert(const K6Arrays& a, hipStream_t s) { hipLaunchKernelGGL(k6_insert_kernel, dim3(1), dim3(kInsThreads), 0, s, a); }

}  // namespace bdx
