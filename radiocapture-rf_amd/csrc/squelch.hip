// squelch.hip -- carrier detect on the GPU (gfx950): GNU Radio's simple_squelch_cc, which the reference's conventional-channel
// ("scanner") system type hangs behind a 12.5 kHz channel and polls (scanning_receiver.py:53,112), behind a channel and on
// every bin of a filterbank.  Definition: include/rcf.h at rcf_chan_squelch; arithmetic: squelch_core.hpp.
//
// Two shapes of one recurrence, level = alpha |x|^2 + (1 - alpha) level in double.
//   squelch_kernel        behind a channel, exact: one lane per channel walks the block's new samples of the channel's IQ
//                         ring in order, in audio_gate_kernel's idiom (audio.hip) -- a wave owns 64 channels, ring traffic is
//                         staged through an LDS tile so that it stays coalesced.  It gates nothing and writes no samples: the
//                         level, the counters and the indices of the first and the last open sample.
//   pfb_squelch_z_kernel, pfb_squelch_walk_kernel      on every bin of a bank: lanes across bins (one 512-byte run of a
//                         frame-major ring per frame and wave), workgroups across segments of kSquelchSegment frames.  The
//                         recurrence is linear, so it is cut in time: pass 1 gives every whole segment its zero-state
//                         response z; pass 2 gives each (segment, bin) its entry level by walking the z of the segments before
//                         it with a^S, then walks the segment again from there and counts.  Two launches in stream order, no
//                         hand-over between the workgroups of a launch: nobody waits for anybody.
// Built with -ffp-contract=off (Makefile): the unfused float / double operations are the specified result.
// Every ring index is masked, every count that sizes a loop is clamped first, nothing is shared between waves.
#include "rcf_internal.h"
#include "squelch_core.hpp"

namespace rcfx {

namespace {

constexpr int kSeqChunk = 64;
constexpr int kSeqRow = kSeqChunk + 1;               // row stride in elements: spreads a column over the banks

// broadcast lane `src`'s value (src wave-uniform) through the scalar unit
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

// ---------------------------------------------------------------- behind a channel
// For a chunk of 64 samples the 64 lanes fetch channel 0's 64 samples (one 512-byte run), then channel 1's, ... into
// xs[channel][sample]; each lane then walks ITS channel's row.  The next chunk's loads are in flight meanwhile.
__global__ __launch_bounds__(64) void squelch_kernel(const SquelchLaunch *__restrict__ items, int n_items, uint64_t ring_mask)
{
    __shared__ float2 xs[64 * kSeqRow];
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * 64;
    const int nc = min(64, n_items - c0);
    const bool mine = lane < nc;
    const SquelchLaunch *it = items + c0 + (mine ? lane : 0);
    SquelchState *st = it->st;
    SquelchWalk w{st->level, st->n_open, st->first_open, st->last_open, st->unmuted};
    const double alpha = it->alpha, one_minus_alpha = 1.0 - it->alpha, thr = it->thr;
    // (a count that sizes a loop: clamped to what the ring holds)
    const int my_nk = mine ? (int)min((uint64_t)max(it->n_k, 0), ring_mask + 1) : 0;
    const long long my_src = (long long)(uintptr_t)it->iq_ring;
    const long long my_lo = it->n_lo;
    int max_nk = 0;
    for (int c = 0; c < nc; ++c) max_nk = max(max_nk, rl32(my_nk, c));
    float2 pre[64];
    auto prefetch = [&](int i0) {
#pragma unroll
        for (int c = 0; c < 64; ++c) {
            const int cc = c < nc ? c : nc - 1;
            const float2 *src = reinterpret_cast<const float2 *>((uintptr_t)rl64(my_src, cc));
            const int i = i0 + lane < rl32(my_nk, cc) ? i0 + lane : 0;
            pre[c] = src[(uint64_t)(rl64(my_lo, cc) + i) & ring_mask];
        }
    };
    prefetch(0);
    for (int i0 = 0; i0 < max_nk; i0 += kSeqChunk) {
#pragma unroll
        for (int c = 0; c < 64; ++c) xs[c * kSeqRow + lane] = pre[c];
        wave_lds_sync();
        if (i0 + kSeqChunk < max_nk) prefetch(i0 + kSeqChunk);
        // only two operations per sample sit on the recurrence; |x|^2 is done 16 samples at a time ahead of it
        const int n_here = min(kSeqChunk, my_nk - i0);
        for (int u0 = 0; u0 < n_here; u0 += 16) {
            float2 x[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) x[u] = xs[lane * kSeqRow + u0 + u];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (u0 + u < n_here) squelch_walk_step(w, alpha, one_minus_alpha, thr, x[u].x, x[u].y, my_lo + i0 + u0 + u);
        }
        wave_lds_sync();
    }
    if (mine) {
        st->level = w.level;
        st->n_seen += my_nk;
        st->n_open = w.n_open;
        st->first_open = w.first_open;
        st->last_open = w.last_open;
        st->unmuted = w.unmuted;
    }
}

// ---------------------------------------------------------------- on every bin of a bank
// sample of relative frame i (masked here) and bin k in the ring's layout
__device__ __forceinline__ float2 bin_sample(const PfbSquelchLaunch &p, int64_t i, int k)
{
    const uint64_t m = (uint64_t)i & p.ring_mask;
    const uint64_t at = p.frame_major ? m * (uint64_t)p.n_bins + (uint64_t)k
                                      : (m >> kPfbTileLog2) * (uint64_t)p.tile_pitch + ((uint64_t)k << kPfbTileLog2) + (m & ((1u << kPfbTileLog2) - 1));
    return p.bins_ring[at];
}

// the launch's frames, clamped to what the ring holds, and its segments
__device__ __forceinline__ int squelch_frames(const PfbSquelchLaunch &p) { return (int)min((uint64_t)max(p.n_frames, 0), p.ring_mask + 1); }

// Pass 1, one wave per (whole segment, 64 bins): the level the segment gives from 0
__global__ __launch_bounds__(64) void pfb_squelch_z_kernel(const PfbSquelchLaunch p)
{
    const int seg = blockIdx.x, k = blockIdx.y * 64 + threadIdx.x;
    const int kk = min(k, p.n_bins - 1);
    const int n = squelch_frames(p);
    if ((int64_t)(seg + 1) * kSquelchSegment > n) return;              // (the grid holds whole segments only)
    const double alpha = p.alpha, one_minus_alpha = 1.0 - p.alpha;
    const int64_t i0 = p.i_lo + (int64_t)seg * kSquelchSegment;
    double z = 0.0;
    for (int f0 = 0; f0 < kSquelchSegment; f0 += 16) {
        float2 x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = bin_sample(p, i0 + f0 + u, kk);
#pragma unroll
        for (int u = 0; u < 16; ++u) z = squelch_step(z, alpha, one_minus_alpha, squelch_power(x[u].x, x[u].y));
    }
    if (k < p.n_bins) p.z[(size_t)seg * p.n_bins + k] = z;
}

// Pass 2, one wave per (segment, 64 bins): the entry level from the bins' level before the launch and the z of the segments
// before this one, then the segment again from there.  Counts and last-open indices of a bin's segments meet in the bin's
// counters through one atomic add / max each (integers: any order gives the same result); the wave of the last segment
// stores the level -- into the OTHER of the state's two level arrays: its siblings may still be reading the one the launch
// started from -- and the bins' bits of the mask.
__global__ __launch_bounds__(64) void pfb_squelch_walk_kernel(const PfbSquelchLaunch p)
{
    const int seg = blockIdx.x, k = blockIdx.y * 64 + threadIdx.x;
    const bool mine = k < p.n_bins;
    const int kk = min(k, p.n_bins - 1);
    const int n = squelch_frames(p);
    const int f_lo = seg * kSquelchSegment;
    if (f_lo >= n) return;
    const int n_here = min(kSquelchSegment, n - f_lo);
    const bool last = f_lo + n_here == n;
    const double alpha = p.alpha, one_minus_alpha = 1.0 - p.alpha, thr = p.thr[kk];
    double level = p.level_in[kk];
    for (int j = 0; j < seg; ++j) level = squelch_enter(p.z[(size_t)j * p.n_bins + kk], level, p.a_pow_s, one_minus_alpha);
    SquelchWalk w{level, 0, -1, -1, 0};
    const int64_t i0 = p.i_lo + f_lo;
    for (int f0 = 0; f0 < n_here; f0 += 16) {
        float2 x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = bin_sample(p, i0 + min(f0 + u, n_here - 1), kk);
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (f0 + u < n_here) squelch_walk_step(w, alpha, one_minus_alpha, thr, x[u].x, x[u].y, i0 + f0 + u);
    }
    if (mine && w.n_open > 0) {
        __hip_atomic_fetch_add(&p.n_open[k], w.n_open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&p.last_open[k], w.last_open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (last) {
        if (mine) p.level_out[k] = w.level;
        const unsigned long long open = __ballot(mine && w.unmuted);
        if (threadIdx.x < 2) p.mask[blockIdx.y * 2 + threadIdx.x] = (uint32_t)(open >> (32 * threadIdx.x));
    }
}

}  // namespace

void launch_squelch(const SquelchLaunch *d_items, int n_items, int max_n_k, uint64_t ring_mask, hipStream_t s)
{
    if (n_items <= 0 || max_n_k <= 0) return;
    hipLaunchKernelGGL(squelch_kernel, dim3((n_items + 63) / 64), dim3(64), 0, s, d_items, n_items, ring_mask);
}

int pfb_squelch_segment() { return kSquelchSegment; }

void launch_pfb_squelch(const PfbSquelchLaunch &p, hipStream_t s)
{
    if (p.n_frames <= 0 || p.n_bins <= 0) return;
    const int whole = p.n_frames / kSquelchSegment, segs = (p.n_frames + kSquelchSegment - 1) / kSquelchSegment;
    const unsigned waves = (unsigned)((p.n_bins + 63) / 64);
    // (the z of the launch's last segment enters nothing)
    if (segs > 1) hipLaunchKernelGGL(pfb_squelch_z_kernel, dim3(std::min(whole, segs - 1), waves), dim3(64), 0, s, p);
    hipLaunchKernelGGL(pfb_squelch_walk_kernel, dim3(segs, waves), dim3(64), 0, s, p);
}

}  // namespace rcfx
