// capture.hip -- carrier-operated capture on the GPU (gfx950): the carrier detector of squelch.hip as a GATE with a lead-in
// and a hang time.  The reference's conventional-channel system type polls the detector and opens a logging_receiver, which
// stays hang_time behind the last activity (scanning_receiver.py:62-113) and has lost the head of the transmission by then;
// this stage turns a channel's IQ stream into the samples of its transmissions only, `pre` samples of lead-in included, and
// a record per transmission.  Definition: include/rcf.h at rcf_chan_capture; the per-sample step: capture_core.hpp.
//
//   capture_kernel        one lane per channel walks the block's new samples of the channel's IQ ring in order, in
//                         audio_gate_kernel's idiom (audio.hip) -- a wave owns 64 channels, ring traffic is staged through
//                         LDS so that it stays coalesced.  Two tiles per chunk of 64 samples: the DETECTOR's at index j (the
//                         loading lane computes |x|^2: a float per sample) and the WRITER's at j - pre (cf32, re-read from
//                         the channel's ring).  The lane parks the survivors in its row of the writer's tile; the rows are
//                         written out channel by channel, one run per channel and chunk.  Records are rare: a lane stores
//                         its own.
// LDS: 64 x 65 x (4 + 8) bytes = 49 920 per workgroup of one wave: three workgroups per CU of 160 KiB.
// Built with -ffp-contract=off (Makefile): the unfused float / double operations are the specified result.
// Every ring index is masked, every count that sizes a loop is clamped first, nothing is shared between waves.
#include "rcf_internal.h"
#include "capture_core.hpp"

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

// For a chunk of 64 samples the 64 lanes fetch channel 0's 64 detector samples and its 64 writer samples (two 512-byte runs),
// then channel 1's, ... into ps[channel][sample] and ws[channel][sample]; each lane then walks ITS channel's rows.  The next
// chunk's loads are in flight meanwhile.
__global__ __launch_bounds__(64) void capture_kernel(const CaptureLaunch *__restrict__ items, int n_items, uint64_t ring_mask)
{
    __shared__ float ps[64 * kSeqRow];
    __shared__ float2 ws[64 * kSeqRow];
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * 64;
    const int nc = min(64, n_items - c0);
    const bool mine = lane < nc;
    const CaptureLaunch *it = items + c0 + (mine ? lane : 0);
    CaptureState *st = it->st;
    CaptureWalk w{st->level, st->last_open, st->n_kept, st->n_records, st->n_windows, st->acc_open, st->acc_peak, st->in_window, st->unmuted};
    const double alpha = it->alpha, one_minus_alpha = 1.0 - it->alpha, thr = it->thr;
    // (a count that sizes a loop: clamped to what the ring holds)
    const int my_nk = mine ? (int)min((uint64_t)max(it->n_k, 0), ring_mask + 1) : 0;
    const long long my_src = (long long)(uintptr_t)it->iq_ring, my_dst = (long long)(uintptr_t)it->cap_ring;
    const long long my_lo = it->n_lo, my_a = it->a, my_hang = it->hang;
    const long long my_wlo = my_lo - (long long)it->pre;            // the writer's index at the detector's n_lo
    const int my_cap_mask = (int)it->cap_mask;
    uint32_t *const my_recs = it->rec_ring;
    const uint32_t my_rec_mask = it->rec_mask;
    int64_t decided = 0;
    int max_nk = 0;
    for (int c = 0; c < nc; ++c) max_nk = max(max_nk, rl32(my_nk, c));
    // (the detector's samples stay raw until they are staged: a power computed here would wait for its load before the walk
    // of the current chunk begins, and nothing would be in flight behind it)
    float2 pre_x[64], pre_w[64];
    auto prefetch = [&](int i0) {
#pragma unroll
        for (int c = 0; c < 64; ++c) {
            const int cc = c < nc ? c : nc - 1;
            const float2 *src = reinterpret_cast<const float2 *>((uintptr_t)rl64(my_src, cc));
            const int i = i0 + lane < rl32(my_nk, cc) ? i0 + lane : 0;
            pre_x[c] = src[(uint64_t)(rl64(my_lo, cc) + i) & ring_mask];
            pre_w[c] = src[(uint64_t)(rl64(my_wlo, cc) + i) & ring_mask];
        }
    };
    prefetch(0);
    for (int i0 = 0; i0 < max_nk; i0 += kSeqChunk) {
#pragma unroll
        for (int c = 0; c < 64; ++c) { ps[c * kSeqRow + lane] = squelch_power(pre_x[c].x, pre_x[c].y); ws[c * kSeqRow + lane] = pre_w[c]; }
        wave_lds_sync();
        if (i0 + kSeqChunk < max_nk) prefetch(i0 + kSeqChunk);
        int kept = 0;
        const long long kept0 = w.n_kept;
        const int n_here = min(kSeqChunk, my_nk - i0);
        for (int u0 = 0; u0 < n_here; u0 += 16) {
            float p[16];
            float2 x[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) { p[u] = ps[lane * kSeqRow + u0 + u]; x[u] = ws[lane * kSeqRow + u0 + u]; }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                if (u0 + u >= n_here) continue;
                const long long j = my_lo + i0 + u0 + u, s = my_wlo + i0 + u0 + u;
                capture_detect(w, alpha, one_minus_alpha, thr, p[u], j);
                if (s < my_a) continue;                                 // the lead-in is clipped at the attach point
                CaptureRec ev;
                const bool keep = capture_write(w, my_hang, s, &ev);
                decided += 1;
                if (keep) ws[lane * kSeqRow + kept] = x[u];             // kept <= u0 + u: never ahead of the reads
                kept += keep ? 1 : 0;
                if (ev.kind) {                                          // (rare)
                    uint32_t *r = my_recs + (size_t)((uint32_t)(w.n_records - 1) & my_rec_mask) * kCaptureRecWords;
                    r[0] = ev.kind; r[1] = ev.n_open;
                    r[2] = (uint32_t)(uint64_t)ev.sample; r[3] = (uint32_t)((uint64_t)ev.sample >> 32);
                    r[4] = (uint32_t)(uint64_t)ev.pos; r[5] = (uint32_t)((uint64_t)ev.pos >> 32);
                    r[6] = __float_as_uint(ev.peak); r[7] = 0u;
                }
            }
        }
        wave_lds_sync();
        for (int c = 0; c < nc; ++c) {                          // coalesced write-back of the survivors
            float2 *dst = reinterpret_cast<float2 *>((uintptr_t)rl64(my_dst, c));
            const uint64_t m = (uint64_t)(uint32_t)rl32(my_cap_mask, c);
            if (lane < rl32(kept, c)) dst[(uint64_t)(rl64(kept0, c) + lane) & m] = ws[c * kSeqRow + lane];
        }
        wave_lds_sync();
    }
    if (mine) {
        st->level = w.level;
        st->n_seen += my_nk;
        st->n_decided += decided;
        st->n_kept = w.n_kept;
        st->n_records = w.n_records;
        st->n_windows = w.n_windows;
        st->last_open = w.last_open;
        st->acc_open = w.acc_open;
        st->acc_peak = w.acc_peak;
        st->in_window = w.in_window;
        st->unmuted = w.unmuted;
    }
}

}  // namespace

void launch_capture(const CaptureLaunch *d_items, int n_items, int max_n_k, uint64_t ring_mask, hipStream_t s)
{
    if (n_items <= 0 || max_n_k <= 0) return;
    hipLaunchKernelGGL(capture_kernel, dim3((n_items + 63) / 64), dim3(64), 0, s, d_items, n_items, ring_mask);
}

}  // namespace rcfx
