"""numpy restatement of the symbol clock stage (rcf_chan_clock_mm, include/rcf.h; csrc/clock.hip): GNU Radio's
digital.clock_recovery_mm_ff(omega, gain_omega, mu, gain_mu, omega_relative_limit) behind quadrature_demod_cf(gain), as the
SmartNet and EDACS control demodulators run it (moto_control_demod.py:113, edacs_control_demod.py:85) -- a scalar loop
with every operation cast to float32, operation for operation what the header states -- and an independent float64 solve
of the interpolator bank's normal equations (rcf_design_mmse_interpolator)."""
import numpy as np

f32 = np.float32
NTAPS, NSTEPS = 8, 128
INT_MAX = 2147483647


def mmse_bank(ntaps=NTAPS, nsteps=NSTEPS, bw=0.25):
    """[nsteps + 1, ntaps] float64: row s solves R h = r for mu = s / nsteps,
    R[j][l] = 2 bw sinc(2 bw (j - l)),  r[j] = 2 bw sinc(2 bw (j - ntaps / 2 + mu))   (numpy's sinc is sin(pi x) / (pi x))"""
    j = np.arange(ntaps, dtype=np.float64)
    R = 2 * bw * np.sinc(2 * bw * (j[:, None] - j[None, :]))
    out = np.empty((nsteps + 1, ntaps))
    for s in range(nsteps + 1):
        r = 2 * bw * np.sinc(2 * bw * (j - ntaps // 2 + s / nsteps))
        out[s] = np.linalg.solve(R, r)
    return out


def linear_bank():
    """T[s] = {0, 0, 0, s / 128, 1 - s / 128, 0, 0, 0}: linear interpolation between the two middle samples"""
    T = np.zeros((NSTEPS + 1, NTAPS), dtype=f32)
    s = np.arange(NSTEPS + 1, dtype=np.float64) / NSTEPS
    T[:, 3] = s
    T[:, 4] = 1 - s
    return T


def _slice(x):
    return f32(-1.0) if x < 0 else f32(1.0)


def clock_recovery_mm(fm, omega, gain_omega=1.4395919, mu=0.5, gain_mu=0.05, omega_relative_limit=0.005, gain=5.0,
                      taps=None, unit_gain_input=True):
    """-> (soft symbols float32, slips).  fm: the stage's whole input from its first sample on -- the unit-gain
    discriminator stream (u = gain * fm, one float32 product) or, unit_gain_input=False, u itself
    (chan_read_fm(cid, gain) delivers that product).  taps: the [129, 8] float32 bank."""
    T = np.ascontiguousarray(taps, dtype=f32)
    assert T.shape == (NSTEPS + 1, NTAPS)
    x = np.asarray(fm, dtype=f32)
    u = (f32(gain) * x).astype(f32) if unit_gain_input else x
    u = np.concatenate([np.zeros(NTAPS - 1, dtype=f32), u])      # zero history: u[m] = 0 before the first input
    n = len(u)
    omega_mid = f32(omega)
    omega_lim = f32(omega_mid * f32(omega_relative_limit))
    g_om, g_mu, mu0 = f32(gain_omega), f32(gain_mu), f32(mu)
    adv0 = int(np.ceil(omega_mid))
    mu_, om, last = mu0, omega_mid, f32(0)
    p = 0                                                        # index into the padded stream: the stage's p + 7
    out, slips = [], 0
    half, steps = f32(0.5), f32(NSTEPS)
    with np.errstate(all="ignore"):
        while p + NTAPS <= n:
            imu = int(np.rint(f32(mu_ * steps)))
            row = T[imu]
            y = f32(0)
            for j in range(NTAPS):
                y = f32(y + f32(row[NTAPS - 1 - j] * u[p + j]))
            mm = f32(f32(_slice(last) * y) - f32(_slice(y) * last))
            last = y
            om = f32(om + f32(g_om * mm))
            d = f32(om - omega_mid)
            om = f32(omega_mid + f32(half * f32(np.abs(f32(d + omega_lim)) - np.abs(f32(d - omega_lim)))))
            mu_ = f32(f32(mu_ + om) + f32(g_mu * mm))
            if not (np.isfinite(mu_) and np.isfinite(om)):       # guard 2
                mu_, om, last = mu0, omega_mid, f32(0)
                step = adv0
                slips += 1
            else:
                fl = np.floor(mu_)
                mu_ = f32(mu_ - fl)
                if fl < 1:                                       # guard 1
                    step = 1
                    slips += 1
                else:
                    step = INT_MAX if fl >= 2147483648.0 else int(fl)
            p += step
            out.append(y)
    return np.array(out, dtype=f32), slips


def fsk2_baseband(bits, sps):
    """+-1 rectangular pulses, `sps` samples per symbol (any real number): sample n carries bit floor(n / sps)"""
    n = int(np.floor(len(bits) * sps))
    k = np.minimum((np.arange(n) / sps).astype(np.int64), len(bits) - 1)
    return (2.0 * np.asarray(bits, dtype=np.float64)[k] - 1.0).astype(f32)


def fsk2_carrier(bits, symbol_rate, fs, offset_hz, deviation_hz, rng, noise=0.01):
    """complex64 2-FSK carrier at offset_hz: rectangular symbols, bit b -> offset_hz +- deviation_hz, unit amplitude, plus
    a little white noise from rng"""
    n = int(len(bits) * fs / symbol_rate)
    k = np.minimum((np.arange(n) * (symbol_rate / fs)).astype(np.int64), len(bits) - 1)
    f = offset_hz + deviation_hz * (2.0 * np.asarray(bits, dtype=np.float64)[k] - 1.0)
    ph = 2 * np.pi * np.cumsum(f) / fs
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return (np.exp(1j * ph) + noise * w).astype(np.complex64)


def align_bits(got, sent, skip=100, max_offset=8):
    """-> (offset, errors) of the best contiguous alignment got[skip + i] == sent[skip + i + offset]"""
    best = None
    g = np.asarray(got[skip:], dtype=np.uint8)
    for off in range(-max_offset, max_offset + 1):
        a = skip + off
        if a < 0:
            continue
        s = np.asarray(sent[a:a + len(g)], dtype=np.uint8)
        m = min(len(s), len(g))
        if m < len(g) - max_offset - 1:
            continue
        e = int(np.count_nonzero(g[:m] != s[:m]))
        if best is None or e < best[1]:
            best = (off, e)
    return best
