// costas.hip -- the back half of the P25 CQPSK demodulators behind a channel's AGC (gfx950): the Gardner symbol clock and
// the Costas carrier loop of op25's gardner_costas_cc, then diff_phasor_cc -> complex_to_arg -> multiply_const_ff(4 / pi)
// (p25_control_demod.py:150-183, logging_receiver.py:282-332), every channel with the stage of a block (or of a group's
// block) in one launch.  op25's source is not in the reference tree: include/rcf.h at rcf_chan_costas DEFINES the stage
// (a restatement of the published algorithm, parity unpinned against any op25 build), tests/gc_ref.py restates it
// operation for operation.
//
// Per channel and AGC output x[m], all in float, T the interpolator bank, W[0 .. L-1] the last L derotated samples:
//   phase += freq (wrapped once);  push (cosf, sinf)(phase + pi/4) * x[m];  mu -= 1;  if mu > 1: next input
//   half = omega / 2;  hs = floor(half);  hm = mu + half - hs;  if hm > 1: hm -= 1, ++hs;  hs = min(hs, L - 8)
//   mid = I(W[0 .. 7], mu);  y = I(W[hs .. hs + 7], hm)         I(v, m) = sum_j T[rint(128 m)][7 - j] v[j]
//   e = clamp((last - y) . mid, +-1);  d = y conj(last);  last = y
//   omega += gain_omega e |y| (kept within omega_mid +- omega_limit);  mu += omega + gain_mu e
//   z = d (r + j r);  pe = the Costas error of z;  freq += beta pe |z|;  phase += freq + alpha pe |z|;  freq clamped
//   out[k] = atan2f(d.im, d.re) * 4 / pi
// and one guard (counted in CostasState::slips): a state that is not finite, or mu <= 1, after a symbol puts the loop back
// to its initial state.  Every product and sum is rounded on its own (no contraction).
//
// The layout is clock.hip's: the loop is a recurrence in time and independent between channels, so a wave owns 64
// channels, one lane each.  Ring traffic goes through an LDS tile: for a chunk of 64 new samples the 64 lanes fetch
// channel 0's run (one coalesced 512-byte row of float2), then channel 1's, ... into xs[channel][32 + sample], the next
// chunk in flight while the current one is walked.  Each lane walks ITS row -- a `for` over the chunk's samples, the trip
// count is the block's, never the data's -- and derotates in place as it passes, so that columns 0 .. 31 + i of a row are
// the derotated history and both interpolator windows are plain row reads; the row's last 32 samples move to the front
// for the next chunk, and come from / go to the state record at the launch's ends (no look-back into the AGC ring).  The
// row pitch is 97 float2 (odd: ds_read_b64 banks on the float2 index mod 32, the lanes of a half-wave cover all 32), the
// bank sits at a row pitch of 9 floats (loop_wave.hpp), and channels with a caller's bank of their own are walked in a
// pass of their own per distinct bank in the wave.
#include "loop_wave.hpp"

namespace rcfx {

namespace {

constexpr int kBack = kCostasHist;                   // 32 columns of derotated history in front of a chunk
constexpr int kRow = kBack + kChunk + 1;             // 97 float2: odd, spreads a column over the banks

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }
// v < lo ? lo : v > hi ? hi : v -- a NaN passes through (the guard then sees it)
__device__ __forceinline__ float clampf(float v, float lo, float hi) { v = lo > v ? lo : v; return hi < v ? hi : v; }
__device__ __forceinline__ float wrap(float ph, float two_pi)
{
    if (ph > two_pi) ph = sub(ph, two_pi);
    if (ph < -two_pi) ph = add(ph, two_pi);
    return ph;
}
__device__ __forceinline__ float mag(float2 v) { return __fsqrt_rn(add(mul(v.x, v.x), mul(v.y, v.y))); }

// I(v, m): the 8-tap interpolation of v[0 .. 7] at fraction m, real and imaginary part apart
__device__ __forceinline__ float2 interp(const float *tab, const float2 *v, float m)
{
    int im = (int)rintf(mul(m, (float)kClockSteps));
    im = min(max(im, 0), kClockSteps);
    const float *tr = tab + im * kTapRow;
    float2 a = make_float2(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < kClockTaps; ++j) {
        const float t = tr[kClockTaps - 1 - j];
        const float2 x = v[j];
        a.x = add(a.x, mul(t, x.x));
        a.y = add(a.y, mul(t, x.y));
    }
    return a;
}

__global__ __launch_bounds__(64) void costas_kernel(const CostasLaunch *__restrict__ items, int n_items, uint64_t ring_mask)
{
#pragma clang fp contract(off)
    __shared__ float2 xs[64 * kRow];
    __shared__ float tab[kRows * kTapRow];
    const float th = 0.78539816339744830962f, r = 0.70710678118654752f, two_pi = 6.28318530717958647692f;
    const float four_over_pi = 1.27323954473516268615f;
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * 64;
    const int nc = min(64, n_items - c0);
    const bool mine = lane < nc;
    const CostasLaunch L = items[c0 + (mine ? lane : 0)];
    const long long my_src = (long long)(uintptr_t)L.agc_ring, my_lo = L.n_lo, my_tab = (long long)(uintptr_t)L.taps;
    const int back = min(max(L.window, kClockTaps), kBack) - 1;        // W[0] is this many columns behind the newest sample
    float2 *row = xs + lane * kRow;

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
        // the state, read once: the loop's scalars into registers, the derotated history into the row's front
        float mu = 0.f, omega = 0.f, phase = 0.f, freq = 0.f;
        float2 last = make_float2(0.f, 0.f);
        long long n_out = 0, slips = 0;
        if (act) {
            const CostasState *st = L.st;
            mu = st->mu; omega = st->omega; phase = st->phase; freq = st->freq; last = st->last;
            n_out = st->n_out; slips = st->slips;
#pragma unroll
            for (int j = 0; j < kBack; ++j) row[j] = st->hist[j];
        }
        // the whole next chunk (one coalesced 512-byte load per channel) is in flight while the current one is walked
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
        for (int i0 = 0; i0 < max_nk; i0 += kChunk) {
#pragma unroll
            for (int c = 0; c < 64; ++c) xs[c * kRow + kBack + lane] = pre[c];
            wave_lds_sync();
            if (i0 + kChunk < max_nk) prefetch(i0 + kChunk);
            const int n_here = min(kChunk, max(my_nk - i0, 0));
            for (int i = 0; i < n_here; ++i) {
                // 1, 2: the NCO, and the sample derotated in place
                phase = wrap(add(phase, freq), two_pi);
                const float a = add(phase, th);
                const float c = cosf(a), s = sinf(a);
                const float2 x = row[kBack + i];
                row[kBack + i] = make_float2(sub(mul(c, x.x), mul(s, x.y)), add(mul(c, x.y), mul(s, x.x)));
                // 3
                mu = sub(mu, 1.0f);
                if (mu > 1.0f) continue;
                // 4: the symbol whose windows end at or before this sample
                const float half = mul(omega, 0.5f);
                const float fl = floorf(half);
                int hs = (int)fl;
                float hm = sub(add(mu, half), fl);
                if (hm > 1.0f) { hm = sub(hm, 1.0f); ++hs; }
                hs = min(max(hs, 0), back + 1 - kClockTaps);           // (max: never taken; keeps the window inside the row whatever happens)
                const float2 *W = row + kBack + i - back;
                const float2 mid = interp(tab, W, mu);
                const float2 y = interp(tab, W + hs, hm);
                float e = add(mul(sub(last.x, y.x), mid.x), mul(sub(last.y, y.y), mid.y));
                if (e != e) e = 0.f;
                e = clampf(e, -1.0f, 1.0f);
                const float2 d = make_float2(add(mul(y.x, last.x), mul(y.y, last.y)), sub(mul(y.y, last.x), mul(y.x, last.y)));
                last = y;
                const float om = add(omega, mul(mul(L.gain_omega, e), mag(y)));
                omega = add(L.omega_mid, clampf(sub(om, L.omega_mid), -L.omega_lim, L.omega_lim));
                mu = add(add(mu, omega), mul(L.gain_mu, e));
                const float2 z = make_float2(sub(mul(d.x, r), mul(d.y, r)), add(mul(d.x, r), mul(d.y, r)));
                const float pe = fabsf(z.x) > fabsf(z.y) ? (z.x > 0.f ? -z.y : z.y) : (z.y > 0.f ? z.x : -z.x);
                const float mz = mag(z);
                freq = add(freq, mul(mul(L.beta, pe), mz));
                phase = wrap(add(add(phase, freq), mul(mul(L.alpha, pe), mz)), two_pi);
                freq = clampf(freq, -L.max_freq, L.max_freq);
                L.sym_ring[(uint64_t)n_out & ring_mask] = mul(atan2f(d.y, d.x), four_over_pi);
                ++n_out;
                if (!(isfinite(mu) && isfinite(omega) && isfinite(phase) && isfinite(freq) && isfinite(last.x) && isfinite(last.y)) ||
                    mu <= 1.0f) {
                    mu = omega = L.omega_mid;
                    phase = freq = 0.f;
                    last = make_float2(0.f, 0.f);
                    ++slips;
                }
            }
            // the last 32 derotated samples are the next chunk's look-back (own row, ascending: a source column is never
            // behind its destination; no other lane touches these columns until the sync)
            for (int j = 0; j < kBack; ++j) row[j] = row[n_here + j];
            wave_lds_sync();
        }
        if (act) {
            CostasState *st = L.st;
            st->mu = mu; st->omega = omega; st->phase = phase; st->freq = freq; st->last = last;
            st->n_out = n_out; st->slips = slips;
#pragma unroll
            for (int j = 0; j < kBack; ++j) st->hist[j] = row[j];
        }
    }
}

}  // namespace

void launch_costas(const CostasLaunch *d_items, int n_items, int max_n_k, uint64_t ring_mask, hipStream_t s)
{
    launch_loop(costas_kernel, d_items, n_items, max_n_k, ring_mask, s);
}

}  // namespace rcfx
