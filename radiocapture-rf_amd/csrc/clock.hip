// clock.hip -- GNU Radio's clock_recovery_mm_ff behind a channel's discriminator (gfx950): the Mueller and Mueller symbol
// clock of the SmartNet and EDACS control demodulators (moto_control_demod.py:113, edacs_control_demod.py:85), every
// clocked channel of a block (or of a group's block) in one launch.
//
// Per channel, all in float, u[m] = gain * fm[m] (u = 0 before the stage's first input), T the interpolator bank:
//   imu  = (int)rintf(mu * 128)
//   y    = sum_{j = 0 .. 7, in that order} T[imu][7 - j] * u[p + j]
//   mm   = slice(last) * y - slice(y) * last                  slice(x) = x < 0 ? -1 : 1
//   last = y;   omega += gain_omega * mm
//   omega = omega_mid + 0.5 (|(omega - omega_mid) + omega_lim| - |(omega - omega_mid) - omega_lim|)
//   mu   = mu + omega + gain_mu * mm;   step = (int)floorf(mu);   mu -= floorf(mu);   p += step
//   out[k] = y
// with two guards GNU Radio does not have (both counted in ClockState::slips): a step < 1 advances by 1, a mu or omega
// that is not finite puts the loop back to (mu0, omega_mid, last = 0) and advances by ceil(omega_mid).  A step beyond
// the int range saturates.  Every product and sum is rounded on its own (no contraction): include/rcf.h has the
// definition, tests/mm_ref.py restates it operation for operation.
//
// The loop is a recurrence in time and independent between channels: a wave owns 64 channels, one lane each, as the
// voice chain's squelch does (audio.hip).  Ring traffic goes through an LDS tile so that it stays coalesced: for a chunk
// of 64 new samples the 64 lanes fetch channel 0's run, then channel 1's, ... into xs[channel][7 + sample]; columns 0 .. 6
// hold the seven samples before the chunk (a symbol's window reaches that far back: read from the ring before the first
// chunk, carried over from the row's end after that).  Each lane then walks ITS row: a `for` over the chunk's samples --
// the trip count is the block's, never the data's -- that produces a symbol when the window's last sample is the one it
// stands on, at most one per sample.  Symbols go to the channel's ring as they are produced.
// The bank sits in LDS, loaded once per workgroup, at a row pitch of 9 floats (loop_wave.hpp says why, and holds the wave's
// scaffolding that costas.hip and fsk4.hip share).  Channels with a caller's bank of their own are walked in a pass of
// their own per distinct bank in the wave.
#include "loop_wave.hpp"

namespace rcfx {

namespace {

constexpr int kBack = kClockTaps - 1;                // samples of look-back in front of a chunk
constexpr int kRow = kBack + kChunk;                 // 71: odd, spreads a column over the banks

__device__ __forceinline__ float slice(float x) { return x < 0.f ? -1.0f : 1.0f; }

__global__ __launch_bounds__(64) void clock_mm_kernel(const ClockLaunch *__restrict__ items, int n_items, uint64_t ring_mask)
{
#pragma clang fp contract(off)
    __shared__ float xs[64 * kRow];
    __shared__ float tab[kRows * kTapRow];
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * 64;
    const int nc = min(64, n_items - c0);
    const bool mine = lane < nc;
    const ClockLaunch L = items[c0 + (mine ? lane : 0)];
    ClockState s = *L.st;
    // the window's newest sample, counted from the launch's first new one: a symbol is due when the walk stands on it
    long long q = s.p + kBack - L.n_lo;
    const long long my_src = (long long)(uintptr_t)L.fm_ring, my_lo = L.n_lo, my_tab = (long long)(uintptr_t)L.taps;
    float *row = xs + lane * kRow;

    unsigned long long todo = __ballot(mine);
    while (todo) {                                   // one pass per distinct bank among the wave's channels (usually one)
        const long long t = rl64(my_tab, __ffsll(todo) - 1);
        const bool act = mine && my_tab == t;
        todo &= ~__ballot(act);
        wave_lds_sync();                             // (the pass before has finished with tab and xs)
        {
            const float *tp = reinterpret_cast<const float *>((uintptr_t)t);
            for (int i = lane; i < kRows * kClockTaps; i += 64) tab[(i >> 3) * kTapRow + (i & 7)] = tp[i];
        }
        const int my_nk = act ? L.n_k : 0;
        int max_nk = 0;
        for (int c = 0; c < nc; ++c) max_nk = max(max_nk, rl32(my_nk, c));
        // the seven samples before the launch's first new one (zero before the stage's start)
#pragma unroll
        for (int j = 0; j < kBack; ++j) {
            const long long m = L.n_lo - kBack + j;
            row[j] = (act && m >= L.n_first) ? L.fm_ring[(uint64_t)m & ring_mask] : 0.f;
        }
        // the whole next chunk (one coalesced 256-byte load per channel) is in flight while the current one is walked
        float pre[64];
        prefetch_rows(pre, my_src, my_lo, my_nk, nc, 0, lane, ring_mask);
        for (int i0 = 0; i0 < max_nk; i0 += kChunk) {
#pragma unroll
            for (int c = 0; c < 64; ++c) xs[c * kRow + kBack + lane] = pre[c];
            wave_lds_sync();
            if (i0 + kChunk < max_nk) prefetch_rows(pre, my_src, my_lo, my_nk, nc, i0 + kChunk, lane, ring_mask);
            const int n_here = min(kChunk, my_nk - i0);
            for (int i = 0; i < n_here; ++i) {
                if (q != i0 + i) continue;
                int imu = (int)rintf(__fmul_rn(s.mu, (float)kClockSteps));
                imu = min(max(imu, 0), kClockSteps);         // (mu is in [0, 1]: never taken; keeps the row inside tab whatever happens)
                const float *tr = tab + imu * kTapRow;
                const float *x = row + i;                    // u[p + j] = gain * x[j]
                float y = 0.f;
#pragma unroll
                for (int j = 0; j < kClockTaps; ++j) y = __fadd_rn(y, __fmul_rn(tr[kClockTaps - 1 - j], __fmul_rn(L.gain, x[j])));
                const float mm = __fsub_rn(__fmul_rn(slice(s.last), y), __fmul_rn(slice(y), s.last));
                s.last = y;
                float om = __fadd_rn(s.omega, __fmul_rn(L.gain_omega, mm));
                const float d = __fsub_rn(om, L.omega_mid);
                om = __fadd_rn(L.omega_mid, __fmul_rn(0.5f, __fsub_rn(fabsf(__fadd_rn(d, L.omega_lim)), fabsf(__fsub_rn(d, L.omega_lim)))));
                float mu = __fadd_rn(__fadd_rn(s.mu, om), __fmul_rn(L.gain_mu, mm));
                int adv;
                if (!isfinite(mu) || !isfinite(om)) {
                    mu = L.mu0; om = L.omega_mid; s.last = 0.f;
                    adv = L.adv0;
                    ++s.slips;
                } else {
                    const float fl = floorf(mu);
                    mu = __fsub_rn(mu, fl);
                    if (fl < 1.0f) { adv = 1; ++s.slips; }
                    else adv = fl >= 2147483648.0f ? 2147483647 : (int)fl;
                }
                s.mu = mu; s.omega = om;
                q += adv;
                L.sym_ring[(uint64_t)s.n_out & ring_mask] = y;
                ++s.n_out;
            }
            // the row's last seven samples are the next chunk's look-back (own row: no other lane touches these columns until the sync)
#pragma unroll
            for (int j = 0; j < kBack; ++j) row[j] = row[kChunk + j];
            wave_lds_sync();
        }
        if (act) {
            s.p = q - kBack + L.n_lo;
            *L.st = s;
        }
    }
}

}  // namespace

void launch_clock_mm(const ClockLaunch *d_items, int n_items, int max_n_k, uint64_t ring_mask, hipStream_t s)
{
    launch_loop(clock_mm_kernel, d_items, n_items, max_n_k, ring_mask, s);
}

}  // namespace rcfx
