"""numpy restatement of the C4FM symbol loop (rcf_chan_fsk4, include/rcf.h; csrc/fsk4.hip): the published tracking loop of
op25's fsk4_demod_ff, as the P25 C4FM demodulators run it behind the boxcar symbol filter (p25_control_demod.py:118-135,
logging_receiver.py:231-251) -- a scalar loop with every operation cast to `dtype`, operation for operation what the
header states (float64 is the definition; float32 state runs the same code and is the yardstick of the GPU test) --, a
C4FM modulator, and the cases the CPU and the GPU tests share.  The stage is unpinned against op25: its source is not in
the reference tree."""
import numpy as np

import gc_ref as R

NTAPS, NSTEPS = 8, 128
LEVEL_OF_DIBIT = (1.0, 3.0, -1.0, -3.0)      # dibit -> deviation in units of symbol_deviation
OP25 = dict(k_spread=0.01, k_timing=0.025, k_fine=0.125, k_coarse=0.00125, spread_min=1.6, spread_max=2.4)


class Fsk4:
    """the stage's state and loop; work(u) consumes symbol-filter outputs (float32) and returns the soft symbols they
    complete (float32, as the stage's ring holds them)"""

    def __init__(self, sample_rate, symbol_rate, k_spread, k_timing, k_fine, k_coarse, spread_min, spread_max, taps,
                 dtype=np.float64):
        f = self.f = dtype
        self.T = np.ascontiguousarray(taps, dtype=np.float32)
        assert self.T.shape == (NSTEPS + 1, NTAPS)
        self.time = f(float(symbol_rate) / float(sample_rate))                # one double division, then the state's type
        self.k_spread, self.k_timing, self.k_fine, self.k_coarse = f(k_spread), f(k_timing), f(k_fine), f(k_coarse)
        self.spread_min, self.spread_max = f(spread_min), f(spread_max)
        self.h = np.zeros(NTAPS, dtype=np.float32)                            # the last 8 inputs, newest last
        self.n_symbols = self.n_slips = 0
        self.imus = []                                                        # the bank row of every symbol
        self._reset()

    def _reset(self):
        f = self.f
        self.clock, self.spread, self.fine, self.coarse = f(0), f(2), f(0), f(0)

    def _window(self, row):
        f = self.f
        s = f(0)
        for j in range(NTAPS):
            s = f(s + f(np.float32(row[j] * self.h[j])))                      # float product, sum in the state's type
        return s

    def work(self, u):
        f = self.f
        u = np.asarray(u, dtype=np.float32)
        one, half, three_halves, two = f(1), f(0.5), f(1.5), f(2)
        out = []
        with np.errstate(all="ignore"):
            for m in range(len(u)):
                # 1
                self.clock = f(self.clock + self.time)
                self.h[:-1] = self.h[1:]
                self.h[-1] = u[m]
                # 2
                if not self.clock > one:
                    continue
                # 3
                self.clock = f(self.clock - one)
                v = np.floor(f(half + f(f(NSTEPS) * f(self.clock / self.time))))
                imu = 0 if not v >= 0 else 127 if v > 127 else int(v)
                self.imus.append(imu)
                a = f(self._window(self.T[imu]) - self.fine)
                b = f(self._window(self.T[imu + 1]) - self.fine)
                out.append(np.float32(f(f(two * a) / self.spread)))
                sp = self.spread
                if a < -sp:
                    e = f(a + f(three_halves * sp))
                    sp = f(sp - f(f(e * half) * self.k_spread))
                elif a < 0:
                    e = f(a + f(half * sp))
                    sp = f(sp - f(e * self.k_spread))
                elif a < sp:
                    e = f(a - f(half * sp))
                    sp = f(sp + f(e * self.k_spread))
                else:
                    e = f(a - f(three_halves * sp))
                    sp = f(sp + f(f(e * half) * self.k_spread))
                if b < a:
                    self.clock = f(self.clock + f(e * self.k_timing))
                else:
                    self.clock = f(self.clock - f(e * self.k_timing))
                sp = self.spread_min if sp < self.spread_min else sp
                sp = self.spread_max if sp > self.spread_max else sp
                self.spread = sp
                self.coarse = f(self.coarse + f(f(self.fine - self.coarse) * self.k_coarse))
                self.fine = f(self.fine + f(e * self.k_fine))
                self.n_symbols += 1
                # the guard
                ok = all(np.isfinite(x) for x in (self.clock, self.spread, self.fine, self.coarse))
                if not ok or self.clock < -1 or self.clock > 2:
                    self._reset()
                    self.n_slips += 1
        return np.array(out, dtype=np.float32)

    def state(self):
        """what rcf_chan_fsk4_state reports"""
        return dict(n_symbols=self.n_symbols, n_slips=self.n_slips, clock=float(self.clock), spread=float(self.spread),
                    fine=float(self.fine), coarse=float(self.coarse))


def fsk4_demod(u, params, taps, dtype=np.float64, cuts=None):
    """-> (soft symbols, stage) of the whole input u, fed in one piece or in the pieces [cuts[i], cuts[i + 1])"""
    st = Fsk4(taps=taps, dtype=dtype, **params)
    if cuts is None:
        cuts = [0, len(u)]
    parts = [st.work(u[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)), st


def fsk4_params(channel_rate, symbol_rate):
    """fsk4_demod_ff's two arguments at a channel of 2 channel_rate samples per second, and op25's constants"""
    return dict(sample_rate=2.0 * channel_rate, symbol_rate=float(symbol_rate), **OP25)


def distance(a, b, lo=0, hi=None, mask=None):
    """-> (rms, largest) |a - b| over the symbols [lo, hi) (hi None: the shorter length) that the boolean `mask` keeps; a
    non-finite symbol that is left in makes both NaN, which no comparison passes"""
    hi = min(len(a), len(b)) if hi is None else hi
    assert 0 <= lo < hi <= min(len(a), len(b)), (lo, hi, len(a), len(b))
    d = np.abs(np.asarray(a[lo:hi], dtype=np.float64) - np.asarray(b[lo:hi], dtype=np.float64))
    if mask is not None:
        d = d[np.asarray(mask[lo:hi], dtype=bool)]
    assert len(d) > 0
    return (float(np.sqrt(np.mean(d ** 2))), float(np.max(d))) if np.isfinite(d).all() else (float("nan"), float("nan"))


def c4fm_carrier(dibits, symbol_rate, fs, offset_hz, timing=0.0, deviation=600.0, amplitude=0.5, span=8, n_samples=None):
    """complex64 C4FM at offset_hz: symbol k (LEVEL_OF_DIBIT[dibit k] * deviation Hz) peaks at time (k + timing) /
    symbol_rate, raised-cosine pulses (alpha 0.2, as gc_ref.dqpsk_carrier makes them) cut at +-span symbols, evaluated
    at fs and frequency-modulated onto the carrier"""
    lv = np.asarray(LEVEL_OF_DIBIT, dtype=np.float64)[np.asarray(dibits, dtype=np.int64)]
    n = int(len(dibits) * fs / symbol_rate) if n_samples is None else int(n_samples)
    t = np.arange(n, dtype=np.float64) * (symbol_rate / fs) - timing         # in symbols
    k0 = np.floor(t).astype(np.int64)
    s = np.zeros(n, dtype=np.float64)
    for j in range(-span + 1, span + 1):
        k = k0 + j
        ok = (k >= 0) & (k < len(lv))
        s += np.where(ok, lv[np.clip(k, 0, len(lv) - 1)], 0.0) * R.raised_cosine(t - k)
    ph = 2 * np.pi * np.cumsum(offset_hz + deviation * s) / fs
    return (amplitude * np.exp(1j * ph)).astype(np.complex64)


slice_dibits = R.slice_dibits
decode_errors = R.decode_errors


def decode_errors_any_lag(soft, sent, skip, lags=range(-80, 32)):
    """-> (lag, errors): slice_dibits(soft[k]) against sent[k - lag] for k >= skip, the best lag of `lags` -- for a loop
    that has started over many times (each time costs a fraction of a symbol) and runs behind a chain of unknown delay"""
    got = slice_dibits(soft)[skip:]
    best = None
    for lag in lags:
        a = skip - lag
        if a < 0 or a + len(got) > len(sent) + 40:
            continue
        want = np.asarray(sent[a:a + len(got)], dtype=np.uint8)
        m = min(len(got), len(want))
        e = int(np.count_nonzero(got[:m] != want[:m]))
        if best is None or e < best[1]:
            best = (lag, e)
    return best


# ---- the test signals the CPU and the GPU tests share: 1500 symbols on a direct 12.5 kHz channel (25 kS/s) of a 400 kS/s
# front-end, pre-filter, discriminator at p25.fm_gain, boxcar symbol filter.  (baud, carrier offset in Hz, timing offset
# in symbols, deviation in Hz): both baud rates, both offset signs (tests/test_fsk4_cpu.py decides the list: the float64
# restatement must decode each without error after the first 500 symbols, without a slip).  Behind the two filters the
# boxcar-flattened levels keep `spread` near its lower limit at a deviation of 600 Hz, and the loop is choosier about the
# timing phase than on a bare discriminator: (4800, 0, 0.0, 600) locks half a symbol off (728 dibit errors) and was
# replaced by timing 0.4; (4800, -200, 0.3, 600) decodes in float64, but its float32-state run sits 0.65 away with a dibit
# error -- a marginal lock that measures the input, not the kernel -- and was replaced by timing 0.5; (6000, -150, 0.2, 600)
# was added so that both baud rates see both offset signs
FS, CHANNEL_RATE, CHANNEL_OFFSET, N_SYMBOLS, SKIP = 400e3, 12500, 50000.0, 1500, 500
CASES = [(4800, 0.0, 0.4, 600.0), (4800, 150.0, 0.5, 600.0), (4800, -200.0, 0.5, 600.0), (4800, -100.0, 0.8, 660.0),
         (6000, 100.0, 0.5, 600.0), (6000, -150.0, 0.2, 600.0)]
REJECTED = (4800, 0.0, 0.0, 600.0)           # does not decode behind the filters: tests/test_fsk4_cpu.py shows it


def case_signal(baud, cfo, timing, deviation, offset=CHANNEL_OFFSET, fs=FS, n_symbols=N_SYMBOLS):
    """-> (x complex64 at fs, the dibits sent): seeded by the case"""
    rng = np.random.default_rng([int(baud), int(cfo) + 10000, int(round(timing * 100)), int(deviation)])
    sent = rng.integers(0, 4, n_symbols).astype(np.uint8)
    return c4fm_carrier(sent, baud, fs, offset + cfo, timing, deviation), sent


def chain_delay(omega, chan_ntaps, decim, pre_ntaps=69, box=5):
    """whole symbols the chain in front of the loop is known to hold a symbol back: the group delays of the channel filter,
    the pre-filter and the boxcar, in channel samples, over omega, rounded down (the loop's own window adds up to one
    symbol more: decode_errors' lag search finds it)"""
    return int(((chan_ntaps - 1) / 2.0 / decim + (pre_ntaps - 1) / 2.0 + (box - 1) / 2.0) / omega)


def symbol_filter(fm, sps):
    """fir_filter_fff(1, (1/sps,)*sps) over the discriminator's output, zero history"""
    c = np.full(sps, 1.0 / sps, dtype=np.float32).astype(np.float64)
    return np.convolve(np.asarray(fm, dtype=np.float64), c)[:len(fm)].astype(np.float32)


# ---- non-finite bursts.  On the CPU (test_guard_brings_the_loop_back) a few samples of the loop's own input are
# overwritten; on the GPU (test_guard_next_to_a_clean_lane) a few front-end input samples of 2500-symbol signals are.
# (case of CASES, the value, the first overwritten front-end input, how many)
N_BURST_SYMBOLS = 2500
BURSTS = [(CASES[1], complex(float("nan"), float("nan")), 100003, 1), (CASES[4], complex(float("inf"), 0.0), 80005, 3)]
BURST_CLEAN = CASES[2]


def burst_signal(case, value=None, at=0, count=0):
    x, sent = case_signal(*case, n_symbols=N_BURST_SYMBOLS)
    if count:
        x = x.copy()
        x[at:at + count] = value
    return x, sent
