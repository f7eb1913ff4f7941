// KD -- duplicate marking (bdx_set_mark_duplicates / bdx_mark_duplicates; the CLI's --mark-dup).  No counterpart in the reference, which
// only ignores reads that already carry SAM flag 0x400 (io/IlluminaPEReadClassifier.cpp:66-74).  The rule is written down in
// include/bdx.h: runs of equal (tid, pos), candidates, the key K, the smallest (name_key, index) of a group survives.
//
// Two launches when no run is long, all over plain columns (19 B per read: tid, pos, mtid, mpos, flag, lib):
//   kd_scan     one lane per record.  It walks at most kDupT neighbours each way comparing (tid, pos).  A record that sees both ends of
//               its run and finds it kDupT records or shorter resolves its group by direct comparison with the run's other records (the
//               name keys are fetched only once an equal-K neighbour is found).  Any other record knows its run is longer than kDupT --
//               a property of the run, the same for each of its records -- and, if it is a candidate, sets its bit in a second bit array
//               and is counted.  The marks leave as one 64-bit word per wave: the flag column is NOT written here, since neighbours
//               still read it.
//   kd_apply    one lane per record: flag |= 0x400 where the bit is set (only those words are written), or the byte mask of
//               bdx_mark_duplicates.
// Only when the host reads a count of long-run candidates that is not zero (everything below is sized from it), between the two:
//   kd_list     one lane per record: the long-run candidates become the work list (appended per wave), and every record says whether
//               it starts a run (one bit).
//   kd_pre, kd_cbase, kd_runid   a prefix count over the run-start bits (per word inside chunks of 256 words, then over the chunks): a
//               work-list entry's RUN ID is the number of run starts up to it.  The rule's runs are stretches of CONSECUTIVE records, so
//               two stretches at one position that are not next to each other (unsorted input) are two runs with two ids.
//   kd_insert   one lane per work-list entry: an open-addressing table in HBM (linear probing on a 64-bit mix of run id and K, slots =
//               work-list indices claimed by compare-and-swap).  A slot that holds an entry of another run or K is stepped over; one of
//               the same is replaced while the newcomer's (name_key, index) is smaller.  What a slot stands for never changes once
//               claimed, so the table ends with every group's survivor in the group's slot whatever the order of arrival.
//   kd_resolve  one lane per work-list entry finds its group's slot again; a record that is not the survivor sets its bit, and the
//               first loser of a slot counts the group.
// Counters: kd_scan and kd_resolve stride over their records with a bounded grid and add up in registers -- one atomic per wave and
// counter for the whole launch (KX's one per wave and 64 records would meet on one address millions of times at a genome share).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bdx_dev.h"

namespace bdx {

namespace {

constexpr int kKdThreads = 256;
constexpr uint32_t kEmptySlot = 0xFFFFFFFFu;

// name key of record i: the resident column, or the caller's pinned batch that still holds it (K2Params' segments)
__device__ __forceinline__ uint64_t kd_key(const KdParams& p, uint64_t i) {
    if (p.nseg == 0) return p.key[i];
    int s = 0;
    while (s + 1 < p.nseg && p.seg_begin[s + 1] <= i) ++s;
    return p.seg_ptr[s][i];
}

__device__ __forceinline__ bool kd_candidate(uint32_t flag, int32_t tid, int32_t mtid) {
    return (flag & 0x1) && !(flag & (0x4 | 0x8 | 0x100 | 0x400 | 0x800)) && tid >= 0 && mtid >= 0;
}

struct KdRec {
    int32_t tid, pos, mtid, mpos;
    uint32_t flag, lib;
};
__device__ __forceinline__ KdRec kd_load(const KdParams& p, uint64_t i) {
    KdRec r;
    r.tid = p.tid[i]; r.pos = p.pos[i]; r.mtid = p.mtid[i]; r.mpos = p.mpos[i]; r.flag = p.flag[i];
    r.lib = p.lib ? p.lib[i] : 0u;   // (a context with one library never copies the column)
    return r;
}
// equal K for two records of one run (tid and pos are the run's; compared all the same)
__device__ __forceinline__ bool kd_same_k(const KdRec& a, const KdRec& b) {
    return a.tid == b.tid && a.pos == b.pos && a.mtid == b.mtid && a.mpos == b.mpos && a.lib == b.lib && ((a.flag ^ b.flag) & 0x70) == 0;
}
__device__ __forceinline__ uint64_t kd_fmix(uint64_t h) {
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return h;
}
__device__ __forceinline__ uint64_t kd_hash(const KdRec& r, uint32_t run) {   // (the run id stands for tid and pos)
    const uint64_t a = run, b = ((uint64_t)(uint32_t)r.mtid << 32) | (uint32_t)r.mpos;
    return kd_fmix(a ^ kd_fmix(b + 0x9e3779b97f4a7c15ull * (uint64_t)((r.lib << 8) | (r.flag & 0x70))));
}

__global__ __launch_bounds__(kKdThreads) void kd_scan_kernel(KdParams p) {
    const uint64_t n = p.n;
    const int lane = threadIdx.x & 63;
    uint32_t n_loser = 0, n_group = 0, n_long = 0;   // this wave's counts (wave-uniform), added to the global ones once, at the end
    // (the block's base is uniform, so all lanes of a wave take every turn of the loop together: the ballots see whole waves)
    for (uint64_t base = (uint64_t)blockIdx.x * kKdThreads; base < n; base += (uint64_t)gridDim.x * kKdThreads) {
    const uint64_t i = base + threadIdx.x;
    bool loser = false, group = false, to_list = false;
    if (i < n) {
        const int32_t t = p.tid[i], ps = p.pos[i];
        // the run's ends, as far as kDupT records away
        uint64_t b = i, e = i + 1;
        while (b > 0 && i - b < (uint64_t)kDupT && p.tid[b - 1] == t && p.pos[b - 1] == ps) --b;
        const bool saw_begin = b == 0 || !(p.tid[b - 1] == t && p.pos[b - 1] == ps);
        while (e < n && e - i - 1 < (uint64_t)kDupT && p.tid[e] == t && p.pos[e] == ps) ++e;
        const bool saw_end = e == n || !(p.tid[e] == t && p.pos[e] == ps);
        const bool is_short = saw_begin && saw_end && e - b <= (uint64_t)kDupT;
        if (e - b > 1 || !is_short) {
            const KdRec me = kd_load(p, i);
            if (kd_candidate(me.flag, me.tid, me.mtid)) {
                if (!is_short) {
                    to_list = true;
                } else {
                    bool have = false;
                    uint64_t mine = 0;
                    for (uint64_t j = b; j < e; ++j) {
                        if (j == i) continue;
                        const KdRec o = kd_load(p, j);
                        if (!kd_candidate(o.flag, o.tid, o.mtid) || !kd_same_k(me, o)) continue;
                        if (!have) { mine = kd_key(p, i); have = true; }
                        const uint64_t theirs = kd_key(p, j);
                        loser |= theirs < mine || (theirs == mine && j < i);
                    }
                    group = have && !loser;   // (the survivor counts its group)
                }
            }
        }
    }
    const uint64_t m_loser = ballot64(loser), m_group = ballot64(group), m_list = ballot64(to_list);
    if (lane == 0 && i < n) {   // (i is a multiple of 64 here: one word per wave and array, zeros included)
        p.bits[i >> 6] = m_loser;
        p.longbits[i >> 6] = m_list;
    }
    n_loser += (uint32_t)popc64(m_loser);
    n_group += (uint32_t)popc64(m_group);
    n_long += (uint32_t)popc64(m_list);
    }
    if (lane == 0) {
        if (n_loser) atomicAdd(&p.cnt->marked, (unsigned long long)n_loser);
        if (n_group) atomicAdd(&p.cnt->groups, (unsigned long long)n_group);
        if (n_long) atomicAdd(&p.cnt->nwork, n_long);
    }
}

// ---- runs longer than kDupT ----
constexpr int kKdChunkWords = kKdThreads;   // words of run-start bits per workgroup of kd_pre (16,384 records)

// the work list from kd_scan's bits, and one bit per record: it starts a run
__global__ __launch_bounds__(kKdThreads) void kd_list_kernel(KdParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * kKdThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool start = false, is_long = false;
    if (i < p.n) {
        start = i == 0 || p.tid[i - 1] != p.tid[i] || p.pos[i - 1] != p.pos[i];
        is_long = (p.longbits[i >> 6] >> (i & 63)) & 1ull;
    }
    const uint64_t m_start = ballot64(start), m_long = ballot64(is_long);
    if (lane == 0 && i < p.n) p.starts[i >> 6] = m_start;
    if (m_long) {
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&p.cnt->nlist, (uint32_t)popc64(m_long));
        at = __shfl(at, 0);
        if (is_long) p.work[at + (uint32_t)popc64(m_long & ((1ull << lane) - 1))] = (uint32_t)i;
    }
}

// run starts in the words before each word of its chunk, and the chunk's total
__global__ __launch_bounds__(kKdThreads) void kd_pre_kernel(KdParams p, uint64_t nwords) {
    __shared__ uint32_t s_wave[kKdThreads / 64];
    const uint64_t w = (uint64_t)blockIdx.x * kKdChunkWords + threadIdx.x;
    const uint32_t c = w < nwords ? (uint32_t)popc64(p.starts[w]) : 0u;
    const uint32_t incl = wave_incl_scan(c);
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) before += s_wave[k];
    if (w < nwords) p.pre[w] = before + incl - c;
    if (threadIdx.x == kKdThreads - 1) p.cbase[blockIdx.x] = before + incl;
}

// the chunks' totals into the run starts before each chunk, in place: one workgroup, every thread a stretch of chunks
__global__ __launch_bounds__(kKdThreads) void kd_cbase_kernel(uint32_t* cbase, uint32_t nchunks) {
    __shared__ uint32_t s_wave[kKdThreads / 64];
    const uint32_t per = (nchunks + kKdThreads - 1) / kKdThreads;
    const uint32_t lo = min(threadIdx.x * per, nchunks), hi = min(lo + per, nchunks);
    uint32_t sum = 0;
    for (uint32_t k = lo; k < hi; ++k) sum += cbase[k];
    const uint32_t incl = wave_incl_scan(sum);
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) run += s_wave[k];
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t c = cbase[k];
        cbase[k] = run;
        run += c;
    }
}

// run id of every work-list entry: the run starts up to and including its record
__global__ __launch_bounds__(kKdThreads) void kd_runid_kernel(KdParams p, uint32_t nwork) {
    const uint32_t w = blockIdx.x * kKdThreads + threadIdx.x;
    if (w >= nwork) return;
    const uint32_t i = p.work[w];
    const uint32_t word = i >> 6, bit = i & 63;
    const uint64_t upto = bit == 63 ? ~0ull : ((1ull << (bit + 1)) - 1);
    p.wrun[w] = p.cbase[word / kKdChunkWords] + p.pre[word] + (uint32_t)popc64(p.starts[word] & upto);
}

// (name_key, index) of a before that of b
__device__ __forceinline__ bool kd_before(uint64_t ka, uint32_t a, uint64_t kb, uint32_t b) { return ka < kb || (ka == kb && a < b); }

__global__ __launch_bounds__(kKdThreads) void kd_insert_kernel(KdParams p, uint32_t nwork) {
    const uint32_t w = blockIdx.x * kKdThreads + threadIdx.x;
    if (w >= nwork) return;
    const uint32_t i = p.work[w], run = p.wrun[w];
    const KdRec me = kd_load(p, i);
    const uint64_t mine = kd_key(p, i);
    uint64_t s = kd_hash(me, run) & p.tmask;
    for (uint64_t probes = 0; probes <= p.tmask; ++probes, s = (s + 1) & p.tmask) {   // (slots >= 2 entries: a free slot always turns up)
        uint32_t cur = __hip_atomic_load(&p.table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmptySlot) {
            cur = atomicCAS(&p.table[s], kEmptySlot, w);
            if (cur == kEmptySlot) return;
        }
        if (p.wrun[cur] != run || !kd_same_k(me, kd_load(p, p.work[cur]))) continue;   // another group's slot
        // my group's slot, for good: take it while I come before its holder
        for (;;) {
            const uint32_t ci = p.work[cur];
            if (!kd_before(mine, i, kd_key(p, ci), ci)) break;
            const uint32_t old = atomicCAS(&p.table[s], cur, w);
            if (old == cur) break;
            cur = old;
        }
        return;
    }
}

__global__ __launch_bounds__(kKdThreads) void kd_resolve_kernel(KdParams p, uint32_t nwork) {
    uint32_t n_loser = 0, n_group = 0;
    for (uint32_t base = blockIdx.x * kKdThreads; base < nwork; base += gridDim.x * kKdThreads) {
    const uint32_t w = base + threadIdx.x;
    bool loser = false, group = false;
    if (w < nwork) {
        const uint32_t i = p.work[w], run = p.wrun[w];
        const KdRec me = kd_load(p, i);
        uint64_t s = kd_hash(me, run) & p.tmask;
        for (uint64_t probes = 0; probes <= p.tmask; ++probes, s = (s + 1) & p.tmask) {
            const uint32_t cur = p.table[s];
            if (cur == kEmptySlot) break;   // (cannot happen: every entry was inserted)
            if (cur != w && (p.wrun[cur] != run || !kd_same_k(me, kd_load(p, p.work[cur])))) continue;
            if (cur != w) {
                loser = true;
                atomicOr(&((uint32_t*)p.bits)[i >> 5], 1u << (i & 31));   // (little endian: bit i & 63 of word i >> 6)
                group = atomicExch(&p.multi[s], 1u) == 0u;                // the slot's first loser counts the group
            }
            break;
        }
    }
    n_loser += (uint32_t)popc64(ballot64(loser));
    n_group += (uint32_t)popc64(ballot64(group));
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_loser) atomicAdd(&p.cnt->marked, (unsigned long long)n_loser);
        if (n_group) atomicAdd(&p.cnt->groups, (unsigned long long)n_group);
    }
}

__global__ __launch_bounds__(kKdThreads) void kd_fill_kernel(uint32_t* a, uint64_t na, uint32_t va, uint32_t* b, uint64_t nb, uint32_t vb) {
    const uint64_t i = (uint64_t)blockIdx.x * kKdThreads + threadIdx.x;
    if (i < na) a[i] = va;
    if (i < nb) b[i] = vb;
}

__global__ __launch_bounds__(kKdThreads) void kd_apply_kernel(const uint64_t* __restrict__ bits, uint64_t n, uint16_t* flag, uint8_t* mask) {
    const uint64_t i = (uint64_t)blockIdx.x * kKdThreads + threadIdx.x;
    if (i >= n) return;
    const bool dup = (bits[i >> 6] >> (i & 63)) & 1ull;
    if (mask) mask[i] = dup ? 1 : 0;
    if (flag && dup) flag[i] = (uint16_t)(flag[i] | 0x400);
}

unsigned kd_grid(uint64_t n) { return (unsigned)((n + kKdThreads - 1) / kKdThreads); }
constexpr unsigned kKdMaxGrid = 4096;   // the counting kernels stride over the records: 256 CUs x 16 workgroups, 4 waves each
unsigned kd_strided_grid(uint64_t n) { return std::min(kd_grid(n), kKdMaxGrid); }

}  // namespace

void launch_kd_scan(const KdParams& p, hipStream_t s) {
    if (!p.n) return;
    hipLaunchKernelGGL(kd_scan_kernel, dim3(kd_strided_grid(p.n)), dim3(kKdThreads), 0, s, p);
}

uint32_t kd_chunks(uint64_t n) { return (uint32_t)(((n + 63) / 64 + kKdChunkWords - 1) / kKdChunkWords); }

// p.work / p.wrun hold nwork entries, p.starts / p.pre a word per 64 records, p.cbase kd_chunks(p.n) words, p.table / p.multi
// p.tmask + 1 slots each
void launch_kd_long(const KdParams& p, uint32_t nwork, hipStream_t s) {
    if (!nwork) return;
    const uint64_t slots = p.tmask + 1, nwords = (p.n + 63) / 64;
    hipLaunchKernelGGL(kd_list_kernel, dim3(kd_grid(p.n)), dim3(kKdThreads), 0, s, p);
    hipLaunchKernelGGL(kd_pre_kernel, dim3(kd_chunks(p.n)), dim3(kKdThreads), 0, s, p, nwords);
    hipLaunchKernelGGL(kd_cbase_kernel, dim3(1), dim3(kKdThreads), 0, s, p.cbase, kd_chunks(p.n));
    hipLaunchKernelGGL(kd_runid_kernel, dim3(kd_grid(nwork)), dim3(kKdThreads), 0, s, p, nwork);
    hipLaunchKernelGGL(kd_fill_kernel, dim3(kd_grid(slots)), dim3(kKdThreads), 0, s, p.table, slots, kEmptySlot, p.multi, slots, 0u);
    hipLaunchKernelGGL(kd_insert_kernel, dim3(kd_grid(nwork)), dim3(kKdThreads), 0, s, p, nwork);
    hipLaunchKernelGGL(kd_resolve_kernel, dim3(kd_strided_grid(nwork)), dim3(kKdThreads), 0, s, p, nwork);
}

void launch_kd_apply(const KdParams& p, uint16_t* flag, uint8_t* mask, hipStream_t s) {
    if (!p.n) return;
    hipLaunchKernelGGL(kd_apply_kernel, dim3(kd_grid(p.n)), dim3(kKdThreads), 0, s, p.bits, p.n, flag, mask);
}

}  // namespace bdx
