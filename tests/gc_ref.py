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
