// KX -- the --exclude rule (bdx_exclude.h) over plain columns, one lane per record: the kernel-level entry point bdx_exclude_mask and
// what a caller of bdx_push / bdx_set_device_reads would filter its own columns with.  The decoder applies the same device function
// inside KB's record stage (kb_records.hip).  The table stays in HBM: records arrive position sorted, so neighbouring lanes' searches
// for their own positions walk the same nodes; the mates' do not.
#include <hip/hip_runtime.h>

#include "bdx_bam_dev.h"

namespace bdx {

namespace {

constexpr int kExcludeThreads = 256;

__global__ __launch_bounds__(kExcludeThreads) void kx_exclude_kernel(ExcludeMask m, const int32_t* __restrict__ tid, const int32_t* __restrict__ pos,
                                                                     const int32_t* __restrict__ mtid, const int32_t* __restrict__ mpos, uint64_t n,
                                                                     uint8_t* __restrict__ out, unsigned long long* n_dropped) {
    const uint64_t i = (uint64_t)blockIdx.x * kExcludeThreads + threadIdx.x;
    const bool drop = i < n && exclude_record(m, tid[i], pos[i], mtid[i], mpos[i]);
    if (i < n) out[i] = drop ? 1 : 0;
    // one atomic per wave
    const uint64_t b = __ballot(drop);
    if ((threadIdx.x & 63) == 0 && b && n_dropped) atomicAdd(n_dropped, (unsigned long long)__builtin_popcountll(b));
}

}  // namespace

void launch_kx_exclude(const ExcludeMask& m, const int32_t* tid, const int32_t* pos, const int32_t* mtid, const int32_t* mpos, uint64_t n, uint8_t* out,
                       unsigned long long* n_dropped, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(kx_exclude_kernel, dim3((unsigned)((n + kExcludeThreads - 1) / kExcludeThreads)), dim3(kExcludeThreads), 0, s, m, tid, pos, mtid, mpos, n,
                       out, n_dropped);
}

}  // namespace bdx

// (bdx_warm_up: the HIP runtime loads a translation unit's device code at the first launch of any of its kernels)
__global__ void kx_noop_kernel() {}
namespace bdx { void warm_kx(hipStream_t s) { hipLaunchKernelGGL(kx_noop_kernel, dim3(1), dim3(64), 0, s); } }
