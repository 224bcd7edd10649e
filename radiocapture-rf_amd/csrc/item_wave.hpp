// item_wave.hpp -- what the kernels in the slicer's layout share (slice.hip, tsbk.hip, edacs.hip, osw.hip, p25lc.hip): a WAVE is an
// item (a channel's stage), four items per workgroup, nothing shared between the waves.  Here are the 64-bit lane reads and
// the launcher; the walks are each kernel's own.
#pragma once
#include "rcf_internal.h"

namespace rcfx {

namespace {

constexpr int kItemWaves = 4;

__device__ __forceinline__ uint64_t rl_u64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int64_t rl_i64(int64_t v, int src) { return (int64_t)rl_u64((uint64_t)v, src); }

// one wave per record, kItemWaves to a workgroup (the records carry their rings' masks: no ring_mask)
template <class Rec>
void launch_item_waves(void (*kernel)(const Rec *, int), const Rec *d_items, int n_items, int max_n_k, hipStream_t s)
{
    if (n_items <= 0 || max_n_k <= 0) return;
    hipLaunchKernelGGL(kernel, dim3((n_items + kItemWaves - 1) / kItemWaves), dim3(64 * kItemWaves), 0, s, d_items, n_items);
}

}  // namespace

}  // namespace rcfx
