// loop_wave.hpp -- what the three symbol-loop kernels share (clock.hip, costas.hip, fsk4.hip): a wave owns 64 channels,
// one lane each; ring traffic goes through an LDS tile, a chunk of 64 new samples per channel at a time, the next chunk
// in flight while the current one is walked; the interpolator bank sits in LDS, and channels with a caller's bank of
// their own are walked in a pass of their own per distinct bank in the wave.  The recurrences, the state records and what
// a row holds in front of a chunk are each kernel's own.
//
// The bank's row pitch is 9 floats: a lane reads row imu, column 7 - j, with imu varying from lane to lane, and
// ds_read_b32 banks on (address / 4) mod 32 -- at the natural pitch of 8 the 129 rows fall on four bank offsets per column
// (an 8-way conflict on average), at 9 (odd) 32 consecutive rows cover all 32 banks.
//
// What is here is what the kernels can share with their instruction streams unchanged.  The bank load, the wave's n_k
// maximum and the row store stay written out in each kernel, and costas.hip keeps its own float2 prefetch: as functions
// they compile to other register allocations and schedules (compare `--cuda-device-only -S` before moving one here).
#pragma once
#include "rcf_internal.h"

namespace rcfx {

namespace {

constexpr int kChunk = 64;
constexpr int kTapRow = kClockTaps + 1;              // 9: see above
constexpr int kRows = kClockSteps + 1;

__device__ __forceinline__ int rl32(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ long long rl64(long long v, int src)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), src);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Samples i0 .. i0 + 63 of every channel's run into registers, one coalesced row per channel: pre[c] is this lane's sample
// of channel c (my_src, my_lo, my_nk: the lane's own ring, first index and count).  The arguments come by reference, as a
// lambda in the kernel would capture them: by value the kernels compile to other code.
__device__ __forceinline__ void prefetch_rows(float (&pre)[64], const long long &my_src, const long long &my_lo, const int &my_nk, const int &nc,
                                              int i0, const int &lane, const uint64_t &ring_mask)
{
#pragma unroll
    for (int c = 0; c < 64; ++c) {
        const int cc = c < nc ? c : nc - 1;
        const float *src = reinterpret_cast<const float *>((uintptr_t)rl64(my_src, cc));
        const int i = i0 + lane < rl32(my_nk, cc) ? i0 + lane : 0;
        pre[c] = src[(uint64_t)(rl64(my_lo, cc) + i) & ring_mask];
    }
}

// one workgroup of one wave per 64 records
template <class Rec>
void launch_loop(void (*kernel)(const Rec *, int, uint64_t), const Rec *d_items, int n_items, int max_n_k, uint64_t ring_mask, hipStream_t s)
{
    if (n_items <= 0 || max_n_k <= 0) return;
    hipLaunchKernelGGL(kernel, dim3((n_items + 63) / 64), dim3(64), 0, s, d_items, n_items, ring_mask);
}

}  // namespace

}  // namespace rcfx
