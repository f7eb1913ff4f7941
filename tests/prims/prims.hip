// Test-only harness (tests/test_gpu_prims.py, tests/test_gpu_insert.py) around the shared primitive headers, included unchanged:
// csrc/bdx_scan.h (the three-launch scan, the look-back scan and its walk), csrc/bdx_wave_search.h and csrc/bdx_window.h (the window
// walk of the query kernels and their per-wave key counters), and csrc/bdx_insert.h (K6's order-key insertion merge: k6_ranksort_kernel
// and k6_insert_kernel through the header's own two launches, and its bucket function).  Built into tests/prims/libbdx_prims.so;
// nothing of it is part of libbdx.so.  Every entry point takes host pointers, does its own allocations and copies, waits for
// the stream and returns HIP's error code (hipErrorInvalidValue for a call that breaks a precondition of the look-back scan:
// such a launch would spin, so it is refused here and never made).  Elements are uint32_t words, a U4 four of them in a row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string.h>

#include <algorithm>
#include <new>
#include <unordered_set>
#include <vector>

#include "bdx_insert.h"
#include "bdx_scan.h"
#include "bdx_wave_search.h"
#include "bdx_window.h"

using namespace bdx;

namespace {

#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    template <class T> T* as() const { return (T*)p; }
};

constexpr unsigned char kFill = 0xA5;               // outputs start out as 0xA5A5A5A5 words: what no launch wrote keeps them
constexpr uint32_t kLbMaxN = (1u << 20) + 1;        // no look-back grid beyond 4,097 workgroups from a test
enum : int { kFlagN = 0, kFlagE = 1, kFlagLanes = 2, kFlagWords = 4 };

__device__ __forceinline__ bool same(uint32_t a, uint32_t b) { return a == b; }
__device__ __forceinline__ bool same(const U4& a, const U4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// The functors load and store, and note what the scans promise their callers: the n handed over is *n_ptr ...
template <class T> struct In {
    const T* src;
    const uint32_t* n_ptr;
    uint32_t* flags;
    __device__ T operator()(uint32_t j, uint32_t n) const {
        if (n != *n_ptr) flags[kFlagN] = 1u;
        return src[j];
    }
};
// ... e is the element's input, and the lanes of one call hold consecutive elements from lane 0 on (K3's HeadOut shuffles on that)
template <class T> struct Out {
    T* dst;
    const T* src;
    const uint32_t* n_ptr;
    uint32_t* flags;
    __device__ void operator()(uint32_t j, uint32_t n, const T& inc, const T& e) const {
        if (n != *n_ptr) flags[kFlagN] = 1u;
        if (!same(e, src[j])) flags[kFlagE] = 1u;
        const uint64_t act = __ballot(1);
        const uint32_t up = (uint32_t)__shfl_up((int)j, 1);
        if ((act & (act + 1)) != 0 || ((threadIdx.x & 63) != 0 && up != j - 1)) flags[kFlagLanes] = 1u;
        dst[j] = inc;
    }
};

// in / out: [n_upper] elements; flags: [kFlagWords]
template <class T> struct ScanBufs {
    DevBuf in, out, n, flags;
    uint32_t n_upper = 0;
    int open(const uint32_t* h_in, uint32_t n_now, uint32_t n_up) {
        n_upper = n_up;
        CK(in.alloc((size_t)n_up * sizeof(T)));
        CK(out.alloc((size_t)n_up * sizeof(T)));
        CK(n.alloc(4));
        CK(flags.alloc(kFlagWords * 4));
        if (n_up) CK(hipMemcpy(in.p, h_in, (size_t)n_up * sizeof(T), hipMemcpyHostToDevice));
        if (n_up) CK(hipMemset(out.p, kFill, (size_t)n_up * sizeof(T)));
        CK(hipMemcpy(n.p, &n_now, 4, hipMemcpyHostToDevice));
        CK(hipMemset(flags.p, 0, kFlagWords * 4));
        return 0;
    }
    In<T> fin() const { return In<T>{in.as<T>(), n.as<uint32_t>(), flags.as<uint32_t>()}; }
    Out<T> fout() const { return Out<T>{out.as<T>(), in.as<T>(), n.as<uint32_t>(), flags.as<uint32_t>()}; }
    int close(uint32_t* h_out, uint32_t* h_flags) {
        CK(hipGetLastError());
        CK(hipStreamSynchronize(nullptr));
        if (n_upper) CK(hipMemcpy(h_out, out.p, (size_t)n_upper * sizeof(T), hipMemcpyDeviceToHost));
        CK(hipMemcpy(h_flags, flags.p, kFlagWords * 4, hipMemcpyDeviceToHost));
        return 0;
    }
};

template <class T> int scan3(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t n_upper, uint32_t* total, uint32_t* flags) {
    if (n > n_upper) return (int)hipErrorInvalidValue;
    ScanBufs<T> b;
    if (const int rc = b.open(in, n, n_upper)) return rc;
    DevBuf blk, tot;
    const size_t blk_bytes = (size_t)scan_grid(n_upper) * sizeof(T);
    CK(blk.alloc(blk_bytes));
    CK(hipMemset(blk.p, 0xFF, blk_bytes));   // (the workspace need not start out as anything)
    CK(tot.alloc(sizeof(T)));
    CK(hipMemset(tot.p, kFill, sizeof(T)));
    scan_launch<T>(b.fin(), b.fout(), b.n.template as<uint32_t>(), n_upper, blk.as<T>(), tot.as<T>(), nullptr);
    if (const int rc = b.close(out, flags)) return rc;
    CK(hipMemcpy(total, tot.p, sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

// look-back words of one scan: sized for n_upper, zero once, and the stamps they have seen since
struct LbState {
    unsigned long long* words = nullptr;
    uint32_t cap_wg = 0;
    int cols = 0;
    std::unordered_set<uint32_t> used;
};

int lb_admit(LbState* st, int cols, uint32_t n, uint32_t n_upper, uint32_t stamp) {
    if (!st || st->cols != cols || n > n_upper || n_upper > kLbMaxN || scan_grid(n_upper, 1) > st->cap_wg) return (int)hipErrorInvalidValue;
    if (stamp == 0 || stamp > 0x3FFFFFFFu || !st->used.insert(stamp).second) return (int)hipErrorInvalidValue;
    return 0;
}

template <class T, int kIters> int scan_lb(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t n_upper, void* state, uint32_t stamp, uint32_t* flags) {
    LbState* st = (LbState*)state;
    if (const int rc = lb_admit(st, ScanCols<T>::n, n, n_upper, stamp)) return rc;
    ScanBufs<T> b;
    if (const int rc = b.open(in, n, n_upper)) return rc;
    scan_launch_lb<T, kIters>(b.fin(), b.fout(), b.n.template as<uint32_t>(), n_upper, st->words, stamp, nullptr);
    return b.close(out, flags);
}

// k6_place_kernel's head: a workgroup per 256 elements of n, its total handed in, the walk called by every thread
__global__ __launch_bounds__(kScanBlock) void head_kernel(const U4* tots, const uint32_t* n_ptr, unsigned long long* state, uint32_t stamp, U4* carry_out) {
    __shared__ uint32_t s_prefix[4];
    const uint32_t n = *n_ptr;
    const uint32_t bid = blockIdx.x, base = bid * kScanBlock;
    if (base >= n) return;
    const U4 tot = tots[bid];
    const U4 carry = lookback_exclusive<U4>(tot, state, stamp, bid, s_prefix);
    carry_out[(size_t)base + threadIdx.x] = carry;
}

// four waves a workgroup, a query each
__global__ __launch_bounds__(256) void search_kernel(const int32_t* tid, const int32_t* pos, uint64_t n, const int32_t* qt, const int64_t* qp, uint32_t nq, uint64_t* out) {
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    out[(size_t)q * 64 + (threadIdx.x & 63)] = wave_lower_bound(tid, pos, n, qt[q], qp[q]);
}

// the window walk: four waves a workgroup, a query (t, wlo, whi) each.  The body counts its calls and notes what the walk promises it:
// all 64 lanes in every call, lane l at the index lane 0 holds + l, s the record's pos; it adds 1 to the query's word of every record
// it is handed with `in` (a vector atomicAdd).  steps / flags: [nq][64], what every lane saw
enum : uint32_t { kWalkLanes = 1, kWalkOrder = 2, kWalkPos = 4 };
__global__ __launch_bounds__(256) void walk_kernel(const int32_t* tid, const int32_t* pos, uint64_t n, uint64_t n_upper, const int32_t* qt, const int64_t* qlo,
                                                   const int64_t* qhi, uint32_t nq, uint32_t* visits, uint32_t* steps, uint32_t* flags) {
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int lane = threadIdx.x & 63;
    uint32_t nsteps = 0, bad = 0;
    wave_window_walk(tid, pos, n, qt[q], qlo[q], qhi[q], [&](uint64_t i, int64_t s, bool in) {
        if (__ballot(1) != ~0ull) bad |= kWalkLanes;
        if (i != (uint64_t)__shfl((long long)i, 0) + (uint64_t)lane) bad |= kWalkOrder;
        if (in) {
            if (i >= n || s != (int64_t)pos[i]) bad |= kWalkPos;
            else atomicAdd(&visits[(size_t)q * n_upper + i], 1u);
        }
        ++nsteps;
    });
    steps[(size_t)q * 64 + lane] = nsteps;
    flags[(size_t)q * 64 + lane] = bad;
}

// the per-wave key counters under the walk, as K8 and KS use them: a record is a hit where its byte of `hit` is not zero, its key is its
// byte of `key`.  Every wave of a block opens and closes the counters, the waves without a query too
__global__ __launch_bounds__(256) void count_kernel(const int32_t* tid, const int32_t* pos, uint64_t n, const uint8_t* hit, const uint8_t* key, const int32_t* qt,
                                                    const int64_t* qlo, const int64_t* qhi, uint32_t nq, int nkeys, uint32_t* counts) {
    extern __shared__ uint32_t s_cnt[];   // [4][nkeys] (nkeys > 1 only)
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = q < nq;
    WaveKeyCounts kc;
    kc.open(s_cnt, nkeys);
    if (live) wave_window_walk(tid, pos, n, qt[q], qlo[q], qhi[q], [&](uint64_t i, int64_t, bool in) { kc.add(in && hit[i] != 0, key, i); });
    kc.close(live, counts, q);
}

// the store and the queries of the two walk entries on the device
struct WalkBufs {
    DevBuf tid, pos, qt, qlo, qhi;
    int open(const int32_t* h_tid, const int32_t* h_pos, uint64_t n_upper, const int32_t* h_qt, const int64_t* h_qlo, const int64_t* h_qhi, uint32_t nq) {
        CK(tid.alloc(n_upper * 4));
        CK(pos.alloc(n_upper * 4));
        CK(qt.alloc((size_t)nq * 4));
        CK(qlo.alloc((size_t)nq * 8));
        CK(qhi.alloc((size_t)nq * 8));
        if (n_upper) {
            CK(hipMemcpy(tid.p, h_tid, n_upper * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(pos.p, h_pos, n_upper * 4, hipMemcpyHostToDevice));
        }
        CK(hipMemcpy(qt.p, h_qt, (size_t)nq * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(qlo.p, h_qlo, (size_t)nq * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(qhi.p, h_qhi, (size_t)nq * 8, hipMemcpyHostToDevice));
        return 0;
    }
};

}  // namespace

extern "C" {

// the three-launch scan as K9 calls it; total: [columns] words, written on the phase-2 route only
int prims_scan3_u32(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t n_upper, uint32_t* total, uint32_t* flags) {
    return scan3<uint32_t>(in, out, n, n_upper, total, flags);
}
int prims_scan3_u4(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t n_upper, uint32_t* total, uint32_t* flags) {
    return scan3<U4>(in, out, n, n_upper, total, flags);
}

int prims_lb_state_new(uint32_t n_upper, int cols, void** out) {
    if ((cols != 1 && cols != 4) || n_upper > kLbMaxN) return (int)hipErrorInvalidValue;
    LbState* st = new (std::nothrow) LbState;
    if (!st) return (int)hipErrorOutOfMemory;
    st->cap_wg = scan_grid(n_upper, 1);
    st->cols = cols;
    const size_t bytes = (size_t)st->cap_wg * cols * 8;
    hipError_t e = hipMalloc((void**)&st->words, bytes);
    if (e == hipSuccess) e = hipMemset(st->words, 0, bytes);
    if (e != hipSuccess) { if (st->words) (void)hipFree(st->words); delete st; return (int)e; }
    *out = st;
    return 0;
}
// what next_lb_stamp does when its counter comes round: every word back to zero, and every stamp free again
int prims_lb_state_clear(void* state) {
    LbState* st = (LbState*)state;
    if (!st) return (int)hipErrorInvalidValue;
    CK(hipMemset(st->words, 0, (size_t)st->cap_wg * st->cols * 8));
    st->used.clear();
    return 0;
}
void prims_lb_state_free(void* state) {
    LbState* st = (LbState*)state;
    if (!st) return;
    (void)hipFree(st->words);
    delete st;
}

// the three instantiations of K3
int prims_scan_lb_u32_1(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t n_upper, void* state, uint32_t stamp, uint32_t* flags) {
    return scan_lb<uint32_t, 1>(in, out, n, n_upper, state, stamp, flags);
}
int prims_scan_lb_u4_1(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t n_upper, void* state, uint32_t stamp, uint32_t* flags) {
    return scan_lb<U4, 1>(in, out, n, n_upper, state, stamp, flags);
}
int prims_scan_lb_u4_2(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t n_upper, void* state, uint32_t stamp, uint32_t* flags) {
    return scan_lb<U4, 2>(in, out, n, n_upper, state, stamp, flags);
}

// tots: [scan_grid(n_upper, 1)] U4; carry_out: [scan_grid(n_upper, 1) * 256] U4, the carry every thread got
int prims_lb_head(const uint32_t* tots, uint32_t* carry_out, uint32_t n, uint32_t n_upper, void* state, uint32_t stamp) {
    LbState* st = (LbState*)state;
    if (const int rc = lb_admit(st, 4, n, n_upper, stamp)) return rc;
    const uint32_t g = scan_grid(n_upper, 1);
    DevBuf t, c, nn;
    CK(t.alloc((size_t)g * sizeof(U4)));
    CK(c.alloc((size_t)g * kScanBlock * sizeof(U4)));
    CK(nn.alloc(4));
    CK(hipMemcpy(t.p, tots, (size_t)g * sizeof(U4), hipMemcpyHostToDevice));
    CK(hipMemset(c.p, kFill, (size_t)g * kScanBlock * sizeof(U4)));
    CK(hipMemcpy(nn.p, &n, 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(head_kernel, dim3(g), dim3(kScanBlock), 0, nullptr, t.as<U4>(), nn.as<uint32_t>(), st->words, stamp, c.as<U4>());
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    CK(hipMemcpy(carry_out, c.p, (size_t)g * kScanBlock * sizeof(U4), hipMemcpyDeviceToHost));
    return 0;
}

// tid / pos: [n_upper] records sorted by (tid, pos), of which the first n are searched; out: [nq][64], the answer every lane got
int prims_search(const int32_t* tid, const int32_t* pos, uint64_t n, uint64_t n_upper, const int32_t* qt, const int64_t* qp, uint32_t nq, uint64_t* out) {
    if (n > n_upper) return (int)hipErrorInvalidValue;
    if (!nq) return 0;
    DevBuf dt, dp, dqt, dqp, dout;
    CK(dt.alloc(n_upper * 4));
    CK(dp.alloc(n_upper * 4));
    CK(dqt.alloc((size_t)nq * 4));
    CK(dqp.alloc((size_t)nq * 8));
    CK(dout.alloc((size_t)nq * 64 * 8));
    if (n_upper) {
        CK(hipMemcpy(dt.p, tid, n_upper * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dp.p, pos, n_upper * 4, hipMemcpyHostToDevice));
    }
    CK(hipMemcpy(dqt.p, qt, (size_t)nq * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dqp.p, qp, (size_t)nq * 8, hipMemcpyHostToDevice));
    CK(hipMemset(dout.p, kFill, (size_t)nq * 64 * 8));
    hipLaunchKernelGGL(search_kernel, dim3((nq + 3) / 4), dim3(256), 0, nullptr, dt.as<int32_t>(), dp.as<int32_t>(), n, dqt.as<int32_t>(), dqp.as<int64_t>(), nq,
                       dout.as<uint64_t>());
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    CK(hipMemcpy(out, dout.p, (size_t)nq * 64 * 8, hipMemcpyDeviceToHost));
    return 0;
}

// tid / pos: [n_upper] records sorted by (tid, pos), of which the first n are the store; visits: [nq][n_upper] (zero before the launch),
// steps, flags: [nq][64] (filled before the launch)
int prims_walk(const int32_t* tid, const int32_t* pos, uint64_t n, uint64_t n_upper, const int32_t* qt, const int64_t* qlo, const int64_t* qhi, uint32_t nq,
               uint32_t* visits, uint32_t* steps, uint32_t* flags) {
    if (n > n_upper) return (int)hipErrorInvalidValue;
    if (!nq) return 0;
    WalkBufs b;
    if (const int rc = b.open(tid, pos, n_upper, qt, qlo, qhi, nq)) return rc;
    DevBuf dv, ds, df;
    const size_t vbytes = (size_t)nq * n_upper * 4, lbytes = (size_t)nq * 64 * 4;
    CK(dv.alloc(vbytes));
    CK(ds.alloc(lbytes));
    CK(df.alloc(lbytes));
    if (vbytes) CK(hipMemset(dv.p, 0, vbytes));
    CK(hipMemset(ds.p, kFill, lbytes));
    CK(hipMemset(df.p, kFill, lbytes));
    hipLaunchKernelGGL(walk_kernel, dim3((nq + 3) / 4), dim3(256), 0, nullptr, b.tid.as<int32_t>(), b.pos.as<int32_t>(), n, n_upper, b.qt.as<int32_t>(),
                       b.qlo.as<int64_t>(), b.qhi.as<int64_t>(), nq, dv.as<uint32_t>(), ds.as<uint32_t>(), df.as<uint32_t>());
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    if (vbytes) CK(hipMemcpy(visits, dv.p, vbytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(steps, ds.p, lbytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(flags, df.p, lbytes, hipMemcpyDeviceToHost));
    return 0;
}

// hit / key: [n] bytes; counts: [rows][nkeys] with rows = nq rounded up to whole blocks of four, filled before the launch: the rows of
// the waves without a query come back as they went
int prims_key_counts(const int32_t* tid, const int32_t* pos, uint64_t n, const uint8_t* hit, const uint8_t* key, const int32_t* qt, const int64_t* qlo,
                     const int64_t* qhi, uint32_t nq, int nkeys, uint32_t* counts) {
    if (nkeys < 1 || nkeys > 255) return (int)hipErrorInvalidValue;
    if (!nq) return 0;
    WalkBufs b;
    if (const int rc = b.open(tid, pos, n, qt, qlo, qhi, nq)) return rc;
    DevBuf dh, dk, dc;
    const size_t cbytes = (size_t)((nq + 3) / 4 * 4) * nkeys * 4;
    CK(dh.alloc(n));
    CK(dk.alloc(n));
    CK(dc.alloc(cbytes));
    if (n) {
        CK(hipMemcpy(dh.p, hit, n, hipMemcpyHostToDevice));
        CK(hipMemcpy(dk.p, key, n, hipMemcpyHostToDevice));
    }
    CK(hipMemset(dc.p, kFill, cbytes));
    hipLaunchKernelGGL(count_kernel, dim3((nq + 3) / 4), dim3(256), nkeys > 1 ? (size_t)4 * nkeys * 4 : 0, nullptr, b.tid.as<int32_t>(), b.pos.as<int32_t>(), n,
                       dh.as<uint8_t>(), dk.as<uint8_t>(), b.qt.as<int32_t>(), b.qlo.as<int64_t>(), b.qhi.as<int64_t>(), nq, nkeys, dc.as<uint32_t>());
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    CK(hipMemcpy(counts, dc.p, cbytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// ---- K6's order-key insertion merge (csrc/bdx_insert.h) ---------------------------------------------------------------------

namespace {

constexpr size_t kInsGuard = 256;   // bytes of 0xA5 behind every array of the buffer set

struct PinBuf {
    void* p = nullptr;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes) { return hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault); }
    template <class T> T* as() const { return (T*)p; }
};

// One buffer set, kept from call to call as a context's is: the arrays of StageBufs::b_ins in size_k6's order (old_key [p2] u64 |
// hs_key_dev [sv] u64 | old_slot [p2] | ins_T, ins_src, ins_pre_l, ins_pre_c [sv + 1] each | sorted_key [nsort] u64 | sorted_slot
// [nsort] | rank_part [kK6RankSlices][nsort]), a guard behind each; the staging records, the counters, and the host's list in pinned memory
struct InsHandle {
    uint32_t sv_cap = 0, p2 = 0, nsort = 0, stage_n = 0;
    bool with_rank = false;
    DevBuf ins, stage, counts;
    PinBuf hs_key, hs_cnt;
    enum { kOldKey, kHsKeyDev, kOldSlot, kInsT, kInsSrc, kPreL, kPreC, kSortedKey, kSortedSlot, kRankPart, kArrays };
    size_t off[kArrays] = {}, bytes[kArrays] = {}, total = 0;
    template <class T> T* at(int i) const { return (T*)((char*)ins.p + off[i]); }
    void lay_out() {
        const size_t sv = sv_cap, each[kArrays] = {(size_t)p2 * 8, sv * 8, (size_t)p2 * 4, (sv + 1) * 4, (sv + 1) * 4, (sv + 1) * 4, (sv + 1) * 4,
                                                   (size_t)nsort * 8, (size_t)nsort * 4, with_rank ? (size_t)nsort * 4 * kK6RankSlices : 0};
        size_t o = 0;
        for (int i = 0; i < kArrays; ++i) {
            off[i] = o; bytes[i] = each[i];
            o = (o + each[i] + kInsGuard + 7) & ~(size_t)7;
        }
        total = o;
    }
    size_t guard_bytes(int i) const { return (i + 1 < kArrays ? off[i + 1] : total) - off[i] - bytes[i]; }
};

__global__ __launch_bounds__(256) void ins_bucket_kernel(const uint64_t* keys, uint32_t n, uint32_t n_regions, int period_arg, uint32_t* out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t period = (uint32_t)max(period_arg, 1);   // (as InsertJob reads K6Arrays::period)
    out[i] = ins_bucket_of(keys[i], period, ins_bucket_span(n_regions, period));
}

// the kernel's preconditions: keys of the device's list that differ, none sharing (T, own, start) with a key of the host's (a start vertex
// is walked by one side), the host's ascending, nothing beyond a capacity, counts that fit their 16 bits
bool ins_admits(const InsHandle* h, const uint64_t* old_key, const uint32_t* old_slot, const uint32_t* cnt_by_slot, uint32_t nd, const uint64_t* hs_key, uint32_t nh) {
    if (nd > h->p2 || nh > h->sv_cap) return false;
    // (the rank sort takes 2,049 ... kK6RankSortMax entries before anything looks at sv_cap, and rank_part is sized for min(sv_cap, kK6RankSortMax))
    if (h->with_rank && nd > kInsLds && nd <= kK6RankSortMax && nd > h->nsort) return false;
    for (uint32_t j = 1; j < nh; ++j)
        if (hs_key[j] < hs_key[j - 1]) return false;
    std::vector<uint64_t> k(old_key, old_key + nd);
    std::sort(k.begin(), k.end());
    for (uint32_t d = 1; d < nd; ++d)
        if (k[d] == k[d - 1]) return false;
    std::unordered_set<uint64_t> host;
    for (uint32_t j = 0; j < nh; ++j) host.insert(hs_key[j] >> kKeyShiftStart);
    for (uint32_t d = 0; d < nd; ++d) {
        if (host.count(old_key[d] >> kKeyShiftStart)) return false;
        if (old_slot[d] >= h->stage_n) return false;
        if (cnt_by_slot[2 * (size_t)old_slot[d]] >= 65536u || cnt_by_slot[2 * (size_t)old_slot[d] + 1] >= 65536u) return false;
    }
    return true;
}

}  // namespace

extern "C" {

// out: [11] kInsThreads, kInsLds, kInsBucketMax, kInsCntLds, kInsBuckets, kInsBucketDepth, kK6RankSortMax, kK6RankSlices, kRankGrid, kRankTile, kScanBlock
void prims_insert_constants(uint32_t* out) {
    const uint32_t v[11] = {kInsThreads, kInsLds, kInsBucketMax, kInsCntLds, kInsBuckets, kInsBucketDepth, kK6RankSortMax, kK6RankSlices, kRankGrid, kRankTile, (uint32_t)kScanBlock};
    memcpy(out, v, sizeof(v));
}

// the header's bucket function over an array, a lane per key
int prims_insert_bucket(const uint64_t* keys, uint32_t n, uint32_t n_regions, int period, uint32_t* out_bucket) {
    if (!n) return 0;
    DevBuf dk, db;
    CK(dk.alloc((size_t)n * 8));
    CK(db.alloc((size_t)n * 4));
    CK(hipMemcpy(dk.p, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    CK(hipMemset(db.p, kFill, (size_t)n * 4));
    hipLaunchKernelGGL(ins_bucket_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, dk.as<uint64_t>(), n, n_regions, period, db.as<uint32_t>());
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    CK(hipMemcpy(out_bucket, db.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// a buffer set for up to sv_cap merged entries; staging slots: 2 * sv_cap (a candidate consumes a read pair); everything starts out as 0xA5 bytes
int prims_insert_open(uint32_t sv_cap, int with_rank_part, void** out) {
    if (!sv_cap || sv_cap > (1u << 20)) return (int)hipErrorInvalidValue;
    InsHandle* h = new (std::nothrow) InsHandle;
    if (!h) return (int)hipErrorOutOfMemory;
    h->sv_cap = sv_cap;
    h->p2 = 1;
    while (h->p2 < sv_cap) h->p2 <<= 1;
    h->nsort = std::min(sv_cap, kK6RankSortMax);
    h->stage_n = 2 * sv_cap;
    h->with_rank = with_rank_part != 0;
    h->lay_out();
    hipError_t e = h->ins.alloc(h->total);
    if (e == hipSuccess) e = hipMemset(h->ins.p, kFill, h->total);
    if (e == hipSuccess) e = h->stage.alloc((size_t)h->stage_n * sizeof(SvOut));
    if (e == hipSuccess) e = hipMemset(h->stage.p, kFill, (size_t)h->stage_n * sizeof(SvOut));
    if (e == hipSuccess) e = h->counts.alloc(sizeof(StageCounts));
    if (e == hipSuccess) e = h->hs_key.alloc((size_t)sv_cap * 8);
    if (e == hipSuccess) e = h->hs_cnt.alloc((size_t)sv_cap * 4);
    if (e != hipSuccess) { delete h; return (int)e; }
    *out = h;
    return 0;
}
void prims_insert_close(void* handle) { delete (InsHandle*)handle; }

// old_key / old_slot: [nd] the device's list, any order; cnt_by_slot: [2 * sv_cap][2] lib_count, cn_count of the staging record of every slot;
// hs_key: [nh] ascending, hs_cnt: [nh] lib_count | cn_count << 16.  out_T / out_src / out_pre_l / out_pre_c: [sv_cap + 1] the four arrays as
// the launch left them (0xA5 bytes before it); out_counts: n_ins (0xA5A5A5A5 before the launch), overflow (0 before it), and 1 where a guard byte changed
int prims_insert_run(void* handle, const uint64_t* old_key, const uint32_t* old_slot, const uint32_t* cnt_by_slot, uint32_t nd, const uint64_t* hs_key,
                     const uint32_t* hs_cnt, uint32_t nh, uint32_t n_regions, int period, int ins_plain, uint32_t* out_T, uint32_t* out_src, uint32_t* out_pre_l,
                     uint32_t* out_pre_c, uint32_t* out_counts) {
    InsHandle* h = (InsHandle*)handle;
    if (!h || !ins_admits(h, old_key, old_slot, cnt_by_slot, nd, hs_key, nh)) return (int)hipErrorInvalidValue;
    const size_t sv1 = (size_t)h->sv_cap + 1;
    for (int i = 0; i < InsHandle::kArrays; ++i) CK(hipMemset((char*)h->ins.p + h->off[i] + h->bytes[i], kFill, h->guard_bytes(i)));
    for (int i = InsHandle::kInsT; i <= InsHandle::kPreC; ++i) CK(hipMemset((char*)h->ins.p + h->off[i], kFill, h->bytes[i]));
    if (nd) {
        CK(hipMemcpy(h->at<uint64_t>(InsHandle::kOldKey), old_key, (size_t)nd * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(h->at<uint32_t>(InsHandle::kOldSlot), old_slot, (size_t)nd * 4, hipMemcpyHostToDevice));
    }
    {
        std::vector<SvOut> st(h->stage_n);
        memset(st.data(), kFill, st.size() * sizeof(SvOut));
        for (uint32_t s = 0; s < h->stage_n; ++s) {
            st[s].sv.lib_count = (int32_t)std::min(cnt_by_slot[2 * (size_t)s], 65535u);   // (a slot no entry names may hold anything)
            st[s].sv.cn_count = (int32_t)std::min(cnt_by_slot[2 * (size_t)s + 1], 65535u);
        }
        CK(hipMemcpy(h->stage.p, st.data(), st.size() * sizeof(SvOut), hipMemcpyHostToDevice));
    }
    if (nh) {
        memcpy(h->hs_key.p, hs_key, (size_t)nh * 8);
        memcpy(h->hs_cnt.p, hs_cnt, (size_t)nh * 4);
    }
    StageCounts sc;
    memset(&sc, 0, sizeof(sc));
    sc.n_old = nd; sc.n_regions = n_regions; sc.n_ins = 0xA5A5A5A5u;
    CK(hipMemcpy(h->counts.p, &sc, sizeof(sc), hipMemcpyHostToDevice));
    K6Arrays a;
    memset(&a, 0, sizeof(a));
    a.sv_cap = h->sv_cap;
    a.old_key = h->at<uint64_t>(InsHandle::kOldKey); a.hs_key_dev = h->at<uint64_t>(InsHandle::kHsKeyDev); a.old_slot = h->at<uint32_t>(InsHandle::kOldSlot);
    a.ins_T = h->at<uint32_t>(InsHandle::kInsT); a.ins_src = h->at<uint32_t>(InsHandle::kInsSrc);
    a.ins_pre_l = h->at<uint32_t>(InsHandle::kPreL); a.ins_pre_c = h->at<uint32_t>(InsHandle::kPreC);
    a.sorted_key = h->at<uint64_t>(InsHandle::kSortedKey); a.sorted_slot = h->at<uint32_t>(InsHandle::kSortedSlot);
    a.rank_part = h->with_rank ? h->at<uint32_t>(InsHandle::kRankPart) : nullptr;
    a.sv_stage = h->stage.as<SvOut>();
    a.hs_key = h->hs_key.as<uint64_t>(); a.hs_cnt = h->hs_cnt.as<uint32_t>(); a.nh = nh;
    a.counts = h->counts.as<StageCounts>();
    a.period = period; a.ins_plain = ins_plain;
    if (a.rank_part) launch_k6_ranksort(a, nullptr);
    launch_k6_insert(a, nullptr);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(nullptr));
    CK(hipMemcpy(out_T, a.ins_T, sv1 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(out_src, a.ins_src, sv1 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(out_pre_l, a.ins_pre_l, sv1 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(out_pre_c, a.ins_pre_c, sv1 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&sc, h->counts.p, sizeof(sc), hipMemcpyDeviceToHost));
    out_counts[0] = sc.n_ins; out_counts[1] = sc.overflow; out_counts[2] = 0;
    std::vector<unsigned char> g;
    for (int i = 0; i < InsHandle::kArrays; ++i) {
        g.resize(h->guard_bytes(i));
        CK(hipMemcpy(g.data(), (char*)h->ins.p + h->off[i] + h->bytes[i], g.size(), hipMemcpyDeviceToHost));
        for (unsigned char b : g)
            if (b != kFill) out_counts[2] = 1;
    }
    return 0;
}

}  // extern "C"
