// KR -- passing read starts inside given intervals of the resident, (tid, pos)-sorted record store (bdx_count_interval_reads; the RCI / RCF /
// RDR columns of the CLI's --depth).  No counterpart in the reference, which says nothing about read depth.
//
// A record counts for interval (t, [beg, end)) when tid == t, beg <= pos < end and K1 let it pass (cls & BDX_CLS_PASS); counts are per key
// (WaveKeyCounts, bdx_window.h).  The store is sorted, so an interval is an index range [L, R) -- two 64-ary ballot searches -- and what is
// left is a count of passing records over an index range.  The query kernels of kq_queries.hip walk their windows record by record, which
// suits windows of a few hundred records; an interval here may hold a chromosome.  So the count comes from a table whose cost per
// interval does not grow with the interval, built anew by every call (nothing to invalidate when the store or the class bytes change):
//
//   kr_chunk_kernel   the store in chunks of C = BDX_DEPTH_CHUNK consecutive records, one workgroup of 256 threads per chunk.  Every thread
//                     loads 8 class bytes as one 64-bit word (the class buffer is the context's own and C is a multiple of 8: aligned);
//                     the word that would reach past n is loaded byte by byte, nothing at an index >= n.  One key: popcount of the pass
//                     bits, a wave reduction, the four waves' sum.  Several: the key bytes likewise and one LDS atomic per passing record
//                     into a row of nkeys words.  table[k][chunk] = passing records of key k in the chunk.
//   kr_prefix_kernel  one workgroup per key turns its row into the exclusive prefix, 256 chunks a step (block_incl_scan, bdx_scan.h) with a
//                     running total: table[k][0] = 0, table[k][nchunks] = the key's total (below 2^32: the store's own limit).
//   kr_query_kernel   one wavefront per interval, four per block.  With c0 = ceil(L / C) and c1 = floor(R / C): if c0 < c1 the whole chunks
//                     [c0, c1) are table[k][c1] - table[k][c0] and only the edges [L, c0 C) and [c1 C, R) are walked (wave_index_walk,
//                     bdx_window.h: below C records each); otherwise [L, R) is walked whole.  Without a table (bdx_set_debug
//                     "depth_plain") every interval is walked whole.  All position arithmetic is 64-bit.
#include <hip/hip_runtime.h>

#include "../../include/bdx.h"
#include "bdx_dev.h"
#include "bdx_scan.h"
#include "bdx_shard.h"
#include "bdx_window.h"

namespace bdx {

static_assert(sizeof(KrInterval) == sizeof(bdx_interval) && sizeof(KrInterval) == 12, "KrInterval is bdx_interval");

namespace {

constexpr int kQueryWaves = 4;
constexpr uint64_t kChunk = BDX_DEPTH_CHUNK;
constexpr int kChunkBlock = 256;
constexpr uint64_t kPassBits = 0x0101010101010101ull * BDX_CLS_PASS;
static_assert(kChunk == (uint64_t)kChunkBlock * 8, "a thread takes 8 records of its workgroup's chunk");
static_assert(kChunkBlock == kScanBlock, "block_incl_scan is written for kScanBlock threads");

// bytes [i, i + 8) of an 8-byte aligned column as one little-endian word; those at n and beyond are 0 and not loaded (i < n, i % 8 == 0)
__device__ __forceinline__ uint64_t load_bytes8(const uint8_t* __restrict__ col, uint64_t i, uint64_t n) {
    if (i + 8 <= n) return *reinterpret_cast<const uint64_t*>(col + i);
    uint64_t w = 0;
    for (uint64_t j = i; j < n; ++j) w |= (uint64_t)col[j] << (8 * (j - i));
    return w;
}

__global__ __launch_bounds__(kChunkBlock) void kr_chunk_kernel(KrParams p) {
    __shared__ uint32_t s_row[256];   // several keys: the chunk's count per key; one key: the four waves' counts
    const uint64_t n = p.st.n;
    const uint32_t chunk = blockIdx.x;
    const uint64_t i = (uint64_t)chunk * kChunk + (uint64_t)threadIdx.x * 8;
    const uint64_t pass = i < n ? load_bytes8(p.st.cls, i, n) & kPassBits : 0;
    const size_t stride = (size_t)p.nchunks + 1;
    if (p.nkeys > 1) {
        for (int k = threadIdx.x; k < p.nkeys; k += kChunkBlock) s_row[k] = 0;
        __syncthreads();
        if (pass) {
            const uint64_t keys = load_bytes8(p.key, i, n);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((pass >> (8 * j)) & BDX_CLS_PASS) {
                    const uint32_t k = (uint32_t)(keys >> (8 * j)) & 0xFFu;
                    atomicAdd(&s_row[k < (uint32_t)p.nkeys ? k : 0u], 1u);   // (an index out of range counts as 0, like everywhere in the store)
                }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < p.nkeys; k += kChunkBlock) p.table[(size_t)k * stride + chunk] = s_row[k];
    } else {
        uint32_t c = (uint32_t)popc64(pass);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) c += __shfl_xor(c, o);
        if (lane_id() == 0) s_row[wave_id()] = c;
        __syncthreads();
        if (threadIdx.x == 0) p.table[chunk] = s_row[0] + s_row[1] + s_row[2] + s_row[3];
    }
}

__global__ __launch_bounds__(kChunkBlock) void kr_prefix_kernel(KrParams p) {
    __shared__ uint32_t s_ws[kScanBlock / 64];
    uint32_t* row = p.table + (size_t)blockIdx.x * ((size_t)p.nchunks + 1);
    uint32_t carry = 0;
    for (uint32_t base = 0; base <= p.nchunks; base += kChunkBlock) {   // (entries 0 .. nchunks: the last one takes the total)
        const uint32_t j = base + threadIdx.x;
        const uint32_t v = j < p.nchunks ? row[j] : 0u;
        uint32_t tot;
        const uint32_t inc = block_incl_scan(v, s_ws, &tot);
        if (j <= p.nchunks) row[j] = carry + inc - v;
        carry += tot;
    }
}

__global__ __launch_bounds__(kQueryWaves * 64) void kr_query_kernel(KrParams p) {
    extern __shared__ uint32_t s_cnt[];   // [kQueryWaves][nkeys] (nkeys > 1 only)
    const StoreView& v = p.st;
    const uint32_t q = blockIdx.x * kQueryWaves + (uint32_t)wave_id();
    const bool live = q < p.nq;   // (wave-uniform: every wave reaches the counters' barriers)
    WaveKeyCounts kc;
    kc.open(s_cnt, p.nkeys);
    if (live && v.n) {
        const KrInterval iv = p.iv[q];
        const uint64_t L = wave_lower_bound(v.tid, v.pos, v.n, iv.tid, (int64_t)iv.beg);
        const uint64_t R = wave_lower_bound(v.tid, v.pos, v.n, iv.tid, (int64_t)iv.end);   // (end >= beg: R >= L)
        const uint64_t c0 = (L + kChunk - 1) / kChunk, c1 = R / kChunk;
        auto count = [&](uint64_t i, bool in) { kc.add(in && (v.cls[i] & BDX_CLS_PASS), p.key, i); };
        if (p.table && c0 < c1) {
            wave_index_walk(L, c0 * kChunk, count);
            wave_index_walk(c1 * kChunk, R, count);
            const size_t stride = (size_t)p.nchunks + 1;
            if (p.nkeys > 1) {
                for (int k = lane_id(); k < p.nkeys; k += 64) {
                    const uint32_t d = p.table[(size_t)k * stride + c1] - p.table[(size_t)k * stride + c0];
                    if (d) atomicAdd(&kc.row[k], d);   // (the row also takes the walks' atomics)
                }
            } else {
                kc.single += p.table[c1] - p.table[c0];
            }
        } else {
            wave_index_walk(L, R, count);
        }
    }
    kc.close(live, p.counts, q);
}

}  // namespace

void launch_kr_table(const KrParams& p, hipStream_t s) {
    if (!p.nchunks || !p.table) return;
    hipLaunchKernelGGL(kr_chunk_kernel, dim3(p.nchunks), dim3(kChunkBlock), 0, s, p);
    hipLaunchKernelGGL(kr_prefix_kernel, dim3(p.nkeys), dim3(kChunkBlock), 0, s, p);
}

void launch_kr_query(const KrParams& p, hipStream_t s) {
    if (!p.nq) return;
    const size_t lds = p.nkeys > 1 ? (size_t)kQueryWaves * p.nkeys * 4 : 0;
    hipLaunchKernelGGL(kr_query_kernel, dim3((p.nq + kQueryWaves - 1) / kQueryWaves), dim3(kQueryWaves * 64), lds, s, p);
}

}  // namespace bdx

// (bdx_warm_up: the HIP runtime loads a translation unit's device code at the first launch of any of its kernels)
__global__ void kr_noop_kernel() {}
namespace bdx { void warm_kr(hipStream_t s) { hipLaunchKernelGGL(kr_noop_kernel, dim3(1), dim3(64), 0, s); } }
