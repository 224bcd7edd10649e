// fsk4.hip -- the back half of the P25 C4FM demodulators behind a channel's symbol filter (gfx950): the symbol-timing,
// deviation and offset tracking loop of op25's fsk4_demod_ff (p25_control_demod.py:118-135, logging_receiver.py:231-251),
// every channel with the stage of a block (or of a group's block) in one launch.  op25's source is not in the reference
// tree: include/rcf.h at rcf_chan_fsk4 DEFINES the stage (a restatement of the published algorithm, parity unpinned
// against any op25 build), tests/fsk4_ref.py restates it operation for operation.
//
// Per channel and symbol-filter output u[m], all state in double, T the interpolator bank, h[0 .. 7] the last 8 inputs:
//   clock += time;  push u[m];  if not (clock > 1): next input
//   clock -= 1;  imu = clamp(floor(0.5 + 128 (clock / time)), 0, 127)
//   a = sum_j (double)(T[imu][j] h[j]) - fine;  b = sum_j (double)(T[imu + 1][j] h[j]) - fine
//   out[k] = (float)(2 a / spread)
//   e = a minus the nearest of the levels -1.5, -0.5, 0.5, 1.5 spread;  spread -+= e k_spread (half of it at the outer levels)
//   clock +-= e k_timing (by the sign of b - a);  spread kept in spread_min .. spread_max
//   coarse += (fine - coarse) k_coarse;  fine += e k_fine
// and one guard (counted in Fsk4State::slips): a state that is not finite, or a clock outside -1 .. 2, after a symbol puts
// the loop back to its initial state.  Every product, sum and quotient is rounded on its own (no contraction).
//
// The layout is clock.hip's: the loop is a recurrence in time and independent between channels, so a wave owns 64
// channels, one lane each.  Ring traffic goes through an LDS tile: for a chunk of 64 new samples the 64 lanes fetch
// channel 0's run (one coalesced 256-byte row), then channel 1's, ... into xs[channel][8 + sample], the next chunk in
// flight while the current one is walked.  Each lane walks ITS row -- a `for` over the chunk's samples, the trip count is
// the lane's own n_k, never the data's and never the wave's maximum.  Every sample is stepped (the clock advances by
// `time` per input), so there is no data-dependent input position as in clock.hip; a symbol's window is the 8 columns that
// end at the sample the walk stands on.  Columns 0 .. 7 of a row are the 8 inputs before the chunk: they come from the
// state record at the launch's start, from the row's end after every chunk, and go back to the record at the launch's end
// (no look-back into the symbol-filter ring).  The row pitch is 73 floats (odd: a column spreads over the banks), the bank
// sits at a row pitch of 9 floats (loop_wave.hpp), and channels with a caller's bank of their own are walked in a pass of
// their own per distinct bank in the wave.
#include "loop_wave.hpp"

namespace rcfx {

namespace {

constexpr int kBack = kClockTaps;                    // 8 columns of history in front of a chunk
constexpr int kRow = kBack + kChunk + 1;             // 73 floats: odd, spreads a column over the banks

__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }

// sum over j = 0 .. 7, in that order, from 0.0, of (double)(row[j] * h[j]): float products, a double sum
__device__ __forceinline__ double window(const float *tr, const float *h)
{
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kClockTaps; ++j) s = add(s, (double)__fmul_rn(tr[j], h[j]));
    return s;
}

__global__ __launch_bounds__(64) void fsk4_kernel(const Fsk4Launch *__restrict__ items, int n_items, uint64_t ring_mask)
{
#pragma clang fp contract(off)
    __shared__ float xs[64 * kRow];
    __shared__ float tab[kRows * kTapRow];
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * 64;
    const int nc = min(64, n_items - c0);
    const bool mine = lane < nc;
    const Fsk4Launch L = items[c0 + (mine ? lane : 0)];
    const long long my_src = (long long)(uintptr_t)L.sym_ring, my_lo = L.n_lo, my_tab = (long long)(uintptr_t)L.taps;
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
        // the state, read once: the loop's scalars into registers, the 8 inputs before the launch into the row's front
        double clock = 0.0, spread = 2.0, fine = 0.0, coarse = 0.0;
        long long n_out = 0, slips = 0;
        if (act) {
            const Fsk4State *st = L.st;
            clock = st->clock; spread = st->spread; fine = st->fine; coarse = st->coarse;
            n_out = st->n_out; slips = st->slips;
#pragma unroll
            for (int j = 0; j < kBack; ++j) row[j] = st->hist[j];
        }
        // the whole next chunk (one coalesced 256-byte load per channel) is in flight while the current one is walked
        float pre[64];
        prefetch_rows(pre, my_src, my_lo, my_nk, nc, 0, lane, ring_mask);
        for (int i0 = 0; i0 < max_nk; i0 += kChunk) {
#pragma unroll
            for (int c = 0; c < 64; ++c) xs[c * kRow + kBack + lane] = pre[c];
            wave_lds_sync();
            if (i0 + kChunk < max_nk) prefetch_rows(pre, my_src, my_lo, my_nk, nc, i0 + kChunk, lane, ring_mask);
            const int n_here = min(kChunk, max(my_nk - i0, 0));
            for (int i = 0; i < n_here; ++i) {
                // 1, 2: the input is in the row already; h[0 .. 7] are the columns that end at it
                clock = add(clock, L.time);
                if (!(clock > 1.0)) continue;
                // 3
                clock = sub(clock, 1.0);
                const double v = floor(add(0.5, mul(128.0, __ddiv_rn(clock, L.time))));
                const int imu = !(v >= 0.0) ? 0 : v > 127.0 ? 127 : (int)v;
                const float *h = row + i + 1;                            // row[kBack + i] is the newest, h[7]
                const float *tr = tab + imu * kTapRow;
                const double a = sub(window(tr, h), fine);
                const double b = sub(window(tr + kTapRow, h), fine);
                L.out_ring[(uint64_t)n_out & ring_mask] = (float)__ddiv_rn(mul(2.0, a), spread);
                ++n_out;
                double e;
                if (a < -spread) {
                    e = add(a, mul(1.5, spread));
                    spread = sub(spread, mul(mul(e, 0.5), L.k_spread));
                } else if (a < 0.0) {
                    e = add(a, mul(0.5, spread));
                    spread = sub(spread, mul(e, L.k_spread));
                } else if (a < spread) {
                    e = sub(a, mul(0.5, spread));
                    spread = add(spread, mul(e, L.k_spread));
                } else {
                    e = sub(a, mul(1.5, spread));
                    spread = add(spread, mul(mul(e, 0.5), L.k_spread));
                }
                clock = b < a ? add(clock, mul(e, L.k_timing)) : sub(clock, mul(e, L.k_timing));
                spread = spread < L.spread_min ? L.spread_min : spread;  // (a NaN passes both)
                spread = spread > L.spread_max ? L.spread_max : spread;
                coarse = add(coarse, mul(sub(fine, coarse), L.k_coarse));
                fine = add(fine, mul(e, L.k_fine));
                if (!(isfinite(clock) && isfinite(spread) && isfinite(fine) && isfinite(coarse)) || clock < -1.0 || clock > 2.0) {
                    clock = 0.0; spread = 2.0; fine = 0.0; coarse = 0.0;
                    ++slips;
                }
            }
            // the last 8 inputs are the next chunk's look-back (own row, ascending: a source column is never behind its
            // destination; no other lane touches these columns until the sync)
#pragma unroll
            for (int j = 0; j < kBack; ++j) row[j] = row[n_here + j];
            wave_lds_sync();
        }
        if (act) {
            Fsk4State *st = L.st;
            st->clock = clock; st->spread = spread; st->fine = fine; st->coarse = coarse;
            st->n_out = n_out; st->slips = slips;
#pragma unroll
            for (int j = 0; j < kBack; ++j) st->hist[j] = row[j];
        }
    }
}

}  // namespace

void launch_fsk4(const Fsk4Launch *d_items, int n_items, int max_n_k, uint64_t ring_mask, hipStream_t s)
{
    launch_loop(fsk4_kernel, d_items, n_items, max_n_k, ring_mask, s);
}

}  // namespace rcfx
