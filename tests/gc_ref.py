"""numpy restatement of the Gardner / Costas symbol recovery stage (rcf_chan_costas, include/rcf.h; csrc/costas.hip): the
published op25 gardner_costas_cc algorithm followed by diff_phasor_cc -> complex_to_arg -> multiply_const_ff(4 / pi), as
the P25 CQPSK demodulators run it behind feedforward_agc_cc (p25_control_demod.py:136-183, logging_receiver.py:278-332)
-- a scalar loop with every operation cast to `dtype`, operation for operation what the header states (float32; float64
runs the same code and is the yardstick of the GPU test) --, op25's fsk4_slicer_fb rule, and a pi/4-DQPSK modulator.
The stage is unpinned against op25: its source is not in the reference tree."""
import math

import numpy as np

NTAPS, NSTEPS, HIST = 8, 128, 32
LEVELS = (-2.0, 0.0, 2.0, 4.0)
STEP_OF_DIBIT = (1, 3, -1, -3)               # dibit -> phase step in units of pi / 4


def window_length(omega):
    """L = max(2 ceil(omega), floor(omega / 2) + 9): 12 at 25000 / 4800, 11 at 25000 / 6000"""
    om = float(np.float32(omega))
    return max(2 * int(math.ceil(om)), int(math.floor(om / 2)) + 9)


class GardnerCostas:
    """the stage's state and loop; work(x) consumes AGC outputs (complex) and returns the soft symbols they complete"""

    def __init__(self, omega, gain_mu, gain_omega, alpha, beta, max_freq, omega_limit, taps, dtype=np.float32):
        f = self.f = dtype
        self.T = np.ascontiguousarray(taps, dtype=np.float32).astype(f)       # the bank's float32 values in either run
        assert self.T.shape == (NSTEPS + 1, NTAPS)
        f32 = np.float32
        # the parameters are float32 in the ABI: both runs start from the same values
        self.omega_mid = f(f32(omega)); self.gain_mu = f(f32(gain_mu)); self.gain_omega = f(f32(gain_omega))
        self.alpha = f(f32(alpha)); self.beta = f(f32(beta)); self.max_freq = f(f32(max_freq)); self.omega_limit = f(f32(omega_limit))
        self.L = window_length(omega)
        assert self.L <= HIST
        self.th = f(f32(math.pi / 4)); self.r = f(f32(0.70710678118654752)); self.two_pi = f(f32(2 * math.pi))
        self.four_over_pi = f(f32(4 / math.pi))
        self.hr = np.zeros(HIST, dtype=f)                                     # the last 32 derotated samples, newest last
        self.hi = np.zeros(HIST, dtype=f)
        self.n_symbols = self.n_slips = 0
        self.n_clamped = 0                                                    # times hs exceeded L - 8 before the min
        self.clamped = []                                                     # ... and the indices of those symbols
        self._reset()

    def _reset(self):
        f = self.f
        self.mu = self.omega_mid; self.omega = self.omega_mid
        self.phase = f(0); self.freq = f(0); self.last_re = f(0); self.last_im = f(0)

    def _wrap(self, ph):
        if ph > self.two_pi:
            ph = self.f(ph - self.two_pi)
        if ph < -self.two_pi:
            ph = self.f(ph + self.two_pi)
        return ph

    def _interp(self, at, m):
        """I(v, m), v = W[at .. at + 7]"""
        f = self.f
        row = self.T[min(max(int(np.rint(f(m * f(NSTEPS)))), 0), NSTEPS)]
        base = HIST - self.L + at
        re, im = f(0), f(0)
        for j in range(NTAPS):
            t = row[NTAPS - 1 - j]
            re = f(re + f(t * self.hr[base + j]))
            im = f(im + f(t * self.hi[base + j]))
        return re, im

    def work(self, x):
        f = self.f
        x = np.asarray(x, dtype=np.complex64)
        xr = x.real.astype(f); xi = x.imag.astype(f)
        one, half = f(1), f(0.5)
        out = []
        with np.errstate(all="ignore"):
            for m in range(len(x)):
                # 1, 2: the NCO and the derotated sample
                self.phase = self._wrap(f(self.phase + self.freq))
                a = f(self.phase + self.th)
                c, s = f(np.cos(a)), f(np.sin(a))
                self.hr[:-1] = self.hr[1:]; self.hi[:-1] = self.hi[1:]
                self.hr[-1] = f(f(c * xr[m]) - f(s * xi[m]))
                self.hi[-1] = f(f(c * xi[m]) + f(s * xr[m]))
                # 3
                self.mu = f(self.mu - one)
                if self.mu > one:
                    continue
                # 4
                hf = f(self.omega * half)
                hs = int(np.floor(hf))
                hm = f(f(self.mu + hf) - f(hs))
                if hm > one:
                    hm = f(hm - one)
                    hs += 1
                if hs > self.L - NTAPS:
                    self.n_clamped += 1
                    self.clamped.append(self.n_symbols)
                hs = min(hs, self.L - NTAPS)
                mid_re, mid_im = self._interp(0, self.mu)
                y_re, y_im = self._interp(hs, hm)
                e = f(f(f(self.last_re - y_re) * mid_re) + f(f(self.last_im - y_im) * mid_im))
                if np.isnan(e):
                    e = f(0)
                e = min(max(e, f(-1)), one)
                d_re = f(f(y_re * self.last_re) + f(y_im * self.last_im))
                d_im = f(f(y_im * self.last_re) - f(y_re * self.last_im))
                self.last_re, self.last_im = y_re, y_im
                mag_y = f(np.sqrt(f(f(y_re * y_re) + f(y_im * y_im))))
                om = f(self.omega + f(f(self.gain_omega * e) * mag_y))
                dv = min(max(f(om - self.omega_mid), f(-self.omega_limit)), self.omega_limit)
                self.omega = f(self.omega_mid + dv)
                self.mu = f(f(self.mu + self.omega) + f(self.gain_mu * e))
                z_re = f(f(d_re * self.r) - f(d_im * self.r))
                z_im = f(f(d_re * self.r) + f(d_im * self.r))
                if abs(z_re) > abs(z_im):
                    pe = f(-z_im) if z_re > 0 else z_im
                else:
                    pe = z_re if z_im > 0 else f(-z_re)
                mag_z = f(np.sqrt(f(f(z_re * z_re) + f(z_im * z_im))))
                self.freq = f(self.freq + f(f(self.beta * pe) * mag_z))
                self.phase = self._wrap(f(f(self.phase + self.freq) + f(f(self.alpha * pe) * mag_z)))
                self.freq = min(max(self.freq, f(-self.max_freq)), self.max_freq)
                out.append(f(f(np.arctan2(d_im, d_re)) * self.four_over_pi))
                self.n_symbols += 1
                # the guard
                ok = all(np.isfinite(v) for v in (self.mu, self.omega, self.phase, self.freq, self.last_re, self.last_im))
                if not ok or self.mu <= one:
                    self._reset()
                    self.n_slips += 1
        return np.array(out, dtype=f)


def gardner_costas(x, params, taps, dtype=np.float32, cuts=None):
    """-> (soft symbols, stage) of the whole input x, fed in one piece or in the pieces [cuts[i], cuts[i + 1])"""
    gc = GardnerCostas(taps=taps, dtype=dtype, **params)
    if cuts is None:
        cuts = [0, len(x)]
    parts = [gc.work(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=dtype), gc


def costas_params(channel_rate, symbol_rate):
    """the values of p25_control_demod.py:150-160 at a channel of 2 channel_rate samples per second"""
    cr = 2.0 * channel_rate
    gain_mu, alpha = 0.025, 0.04
    return dict(omega=cr / symbol_rate, gain_mu=gain_mu, gain_omega=0.1 * gain_mu * gain_mu, alpha=alpha,
                beta=0.125 * alpha * alpha, max_freq=2 * math.pi * 1200.0 / cr, omega_limit=0.005)


def slice_dibits(soft, levels=LEVELS):
    """op25 fsk4_slicer_fb(levels): < l0 -> 3, < l1 -> 2, < l2 -> 0, else 1"""
    s = np.asarray(soft, dtype=np.float64)
    return np.where(s < levels[0], 3, np.where(s < levels[1], 2, np.where(s < levels[2], 0, 1))).astype(np.uint8)


def angle_diff_mod8(a, b):
    """a - b for soft symbols (angles in units of pi / 4, period 8), folded into [-4, 4)"""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return (d + 4.0) % 8.0 - 4.0


def distance(a, b, lo=0, hi=None, mask=None):
    """-> (rms, largest) absolute angle_diff_mod8(a, b) over the symbols [lo, hi) (hi None: the shorter length) that the
    boolean `mask` (indexed like a and b) keeps.  Non-finite symbols have to be masked out by the caller: one that is left
    in makes both measures NaN, which no comparison passes"""
    hi = min(len(a), len(b)) if hi is None else hi
    assert 0 <= lo < hi <= min(len(a), len(b)), (lo, hi, len(a), len(b))
    d = np.abs(angle_diff_mod8(a[lo:hi], b[lo:hi]))
    if mask is not None:
        d = d[np.asarray(mask[lo:hi], dtype=bool)]
    assert len(d) > 0
    return (float(np.sqrt(np.mean(d ** 2))), float(np.max(d))) if np.isfinite(d).all() else (float("nan"), float("nan"))


def raised_cosine(t, alpha=0.2):
    """the raised-cosine pulse h(t), t in symbols: sinc(t) cos(pi alpha t) / (1 - (2 alpha t)^2), closed form at the poles"""
    t = np.asarray(t, dtype=np.float64)
    den = 1.0 - (2.0 * alpha * t) ** 2
    pole = np.abs(den) < 1e-9
    h = np.sinc(t) * np.cos(np.pi * alpha * t) / np.where(pole, 1.0, den)
    return np.where(pole, np.pi / 4 * np.sinc(1.0 / (2 * alpha)), h)


def dqpsk_carrier(dibits, symbol_rate, fs, offset_hz, timing=0.0, amplitude=0.5, span=8, n_samples=None):
    """complex64 pi/4-DQPSK at offset_hz: symbol k (phase stepped by STEP_OF_DIBIT[dibit k] pi / 4) peaks at time
    (k + timing) / symbol_rate, raised-cosine pulses (alpha 0.2) cut at +-span symbols, evaluated at fs"""
    steps = np.asarray(STEP_OF_DIBIT, dtype=np.float64)[np.asarray(dibits, dtype=np.int64)]
    a = np.exp(1j * np.pi / 4 * np.cumsum(steps))
    n = int(len(dibits) * fs / symbol_rate) if n_samples is None else int(n_samples)
    t = np.arange(n, dtype=np.float64) * (symbol_rate / fs) - timing         # in symbols
    k0 = np.floor(t).astype(np.int64)
    s = np.zeros(n, dtype=np.complex128)
    for j in range(-span + 1, span + 1):
        k = k0 + j
        ok = (k >= 0) & (k < len(a))
        s += np.where(ok, a[np.clip(k, 0, len(a) - 1)], 0.0) * raised_cosine(t - k)
    ph = 2 * np.pi * offset_hz * np.arange(n, dtype=np.float64) / fs
    return (amplitude * s * np.exp(1j * ph)).astype(np.complex64)


def decode_errors(soft, sent, delay, skip=500, max_lag=8):
    """-> (lag, errors): slice_dibits(soft[k]) against sent[k - delay - lag] for k >= skip, the best lag of 0 .. max_lag.
    delay: the whole symbols the chain in front of the loop is known to hold back"""
    got = slice_dibits(soft)[skip:]
    best = None
    for lag in range(max_lag + 1):
        a = skip - delay - lag
        if a < 0:
            continue
        want = np.asarray(sent[a:a + len(got)], dtype=np.uint8)
        m = min(len(got), len(want))
        if m < len(got) - max_lag - 1:
            continue
        e = int(np.count_nonzero(got[:m] != want[:m]))
        if best is None or e < best[1]:
            best = (lag, e)
    return best


# ---- the test signals the CPU and the GPU tests share: 1500 symbols on a direct 12.5 kHz channel (25 kS/s) of a 400 kS/s
# front-end, pre-filter, feedforward_agc_cc(1024, 1.0).  (baud, carrier offset in Hz, timing offset in symbols): both baud
# rates, both offset signs, timing phases away from the Gardner detector's unstable point (tests/test_costas_cpu.py
# decides the list: the restatement must decode each without error after the first 500 symbols)
FS, CHANNEL_RATE, CHANNEL_OFFSET, N_SYMBOLS, SKIP, AGC_N = 400e3, 12500, 50000.0, 1500, 500, 1024
CASES = [(4800, 100.0, 0.5), (4800, -150.0, 0.61), (4800, 250.0, 0.3), (6000, 250.0, 0.5), (6000, -200.0, 0.61)]


def case_signal(baud, cfo, timing, offset=CHANNEL_OFFSET, fs=FS, n_symbols=N_SYMBOLS):
    """-> (x complex64 at fs, the dibits sent): seeded by the case"""
    rng = np.random.default_rng([int(baud), int(cfo) + 10000, int(round(timing * 100))])
    sent = rng.integers(0, 4, n_symbols).astype(np.uint8)
    return dqpsk_carrier(sent, baud, fs, offset + cfo, timing), sent


def chain_delay(omega, chan_ntaps, decim, pre_ntaps=69, agc_n=AGC_N):
    """whole symbols the chain in front of the loop holds a symbol back: the channel filter's and the pre-filter's group
    delays and the AGC's N - 1 samples, in channel samples, over omega, rounded down"""
    return int(((chan_ntaps - 1) / 2.0 / decim + (pre_ntaps - 1) / 2.0 + (agc_n - 1)) / omega)


# ---- mixed rates and the omega range in one wave (test_mixed_rates_and_omega_range_in_one_wave): eight direct channels
# of one 400 kS/s front-end, feedforward_agc_cc(64, 1.0) and the loop on each, six blocks of 16000 inputs, so that n_k is
# 500, 1000 or 2000 and the lanes leave the kernel's chunk loop at different trips.  The rates interleave across the lanes.
# (chan_open's rate, baud, channel offset, carrier offset, timing, the block the loop is attached before, a caller's
#  bank, decodes after `skip` symbols or None: tests/test_costas_cpu.py decides the last column)
MIXED_BLK, MIXED_BLOCKS, MIXED_AGC_N = 16000, 6, 64
MIXED = [
    (25000, 9600, -130000.0, 80.0, 0.5, 2, False, 500),       # omega 5.2083 at 50 kS/s, two blocks late
    (6250, 2400, 20000.0, 60.0, 0.5, 0, False, 200),          # omega 5.2083 at 12.5 kS/s
    (12500, 3125, -75000.0, 100.0, 0.5, 0, False, 500),       # omega 8, L = 16
    (25000, 3125, 150000.0, 70.0, 0.5, 0, False, 200),        # omega 16, L = 32: the window is the whole history
    (6250, 6000, 50000.0, 90.0, 0.5, 0, False, None),         # omega 2.0833, L = 10: too narrow a channel to decode
    (12500, 4800, -25000.0, 100.0, 0.5, 0, False, 300),       # the P25 shape
    (12500, 6000, 90000.0, -80.0, 0.5, 0, True, None),        # a caller's bank (linear): a second pass in the wave
    (6250, 2400, -190000.0, -60.0, 0.4, 0, False, 200),
]


def mixed_signal():
    """-> (x complex64 of MIXED_BLOCKS blocks, per channel the dibits sent): the eight carriers over weak noise"""
    n = MIXED_BLK * MIXED_BLOCKS
    rng = np.random.default_rng(816)
    x = 0.002 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    sent = []
    for cr, baud, off, cfo, timing, _, _, _ in MIXED:
        d = rng.integers(0, 4, n * baud // int(FS) + 2).astype(np.uint8)
        x = x + dqpsk_carrier(d, baud, FS, off + cfo, timing, amplitude=0.1, n_samples=n)
        sent.append(d)
    return x.astype(np.complex64), sent


def comparable_prefix(s_a, gc_a, s_b, gc_b, tol=0.05):
    """-> (P, the clamp hits inside it): the longest prefix of symbols over which two runs of the restatement on one input
    are the same loop up to rounding: every symbol k < P differs by less than tol (a run that was one symbol ahead of the
    other would not), and both runs took the window clamp at the same symbols k < P"""
    n = min(len(s_a), len(s_b))
    far = np.flatnonzero(~(np.abs(angle_diff_mod8(s_a[:n], s_b[:n])) < tol))
    P = int(far[0]) if len(far) else n
    odd = sorted(set(gc_a.clamped) ^ set(gc_b.clamped))
    if odd and odd[0] < P:
        P = odd[0]
    return P, [k for k in gc_a.clamped if k < P]


# ---- non-finite bursts (test_coming_back_from_non_finite_input): standard-chain signals of 2500 symbols with a few
# front-end input samples overwritten.  (case of CASES, the value, the first overwritten input, how many, the dibit
# errors of the restatement later than SKIP symbols after the burst: tests/test_costas_cpu.py decides the last column)
N_BURST_SYMBOLS = 2500
BURSTS = [(CASES[0], complex(float("nan"), float("nan")), 100003, 1, 0), (CASES[3], complex(float("inf"), 0.0), 80005, 3, 0)]
BURST_CLEAN = CASES[1]


def burst_signal(case, value=None, at=0, count=0):
    x, sent = case_signal(*case, n_symbols=N_BURST_SYMBOLS)
    if count:
        x = x.copy()
        x[at:at + count] = value
    return x, sent


def burst_span(agc, omega):
    """-> (first, last) symbol index a burst can have touched directly: the AGC outputs that are not finite or exactly
    zero (a gain of 1 / inf) in the middle half of the stream, over omega, widened by 8 symbols either way (the loop's
    omega stays within 0.1 % of the nominal one, every slip moves the count by less than one symbol)"""
    n = len(agc)
    bad = np.flatnonzero(~np.isfinite(agc) | (agc == 0))
    bad = bad[(bad > n // 4) & (bad < 3 * n // 4)]
    assert len(bad) > 0
    return int(bad[0] / omega) - 8, int(bad[-1] / omega) + 8


def symbols_before_first_slip(x, params, taps, dtype=np.float32):
    """the number of symbols the restatement has produced when its guard first fires (None: it never does)"""
    gc = GardnerCostas(taps=taps, dtype=dtype, **params)
    for m in range(len(x)):
        gc.work(x[m:m + 1])
        if gc.n_slips:
            return gc.n_symbols
    return None


# ---- the window clamp (test_window_clamp): a 6250-baud carrier in the standard chain and a loop whose negative gain_omega
# pins omega at its upper limit, 4.15 > 4: hs reaches 3 > L - 8 = 2.  Such a loop is chaotic; only a prefix is comparable
CLAMP_CASE = (6250, 100.0, 0.5)
CLAMP_PARAMS = dict(omega=3.95, omega_limit=0.2, gain_omega=-1e-2)

# ---- the guard's mu <= 1 arm (test_guard_through_mu): CASES[0] cut to 600 symbols on a direct channel with
# feedforward_agc_cc(64, 1.0), and a gain_mu that throws mu below 1 (-40) or far away (-3e38: the loop sleeps)
MU_SYMBOLS, MU_AGC_N, MU_GAINS = 600, 64, (-40.0, -3e38)
