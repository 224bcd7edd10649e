"""numpy restatement of GNU Radio 3.8 analog.feedforward_agc_cc(nsamples, reference) (feedforward_agc_cc_impl), the AGC of
the P25 CQPSK front half (p25_control_demod.py:149, logging_receiver.py:281).  The block has set_history(N): its input
starts with N - 1 zeros, the output count equals the input count, and

    env(z)  = float(|re| > |im| ? (double)|re| + 0.4 (double)|im| : (double)|im| + 0.4 (double)|re|)
    M[n]    = max(1e-4f, max_{m = n-N+1 .. n} env(x[m]))
    out[n]  = (R / M[n]) * x[n - N + 1]            (float division, then one float product per component)

Every step is exactly rounded, so the vectorised form below and the naive loop give the same bits."""
import numpy as np

f32 = np.float32
MAX_ENV_FLOOR = f32(1e-4)


def envelope(x):
    """env() of every sample of a complex64 array: the double arithmetic of GNU Radio's envelope(), one rounding to float"""
    x = np.asarray(x, dtype=np.complex64)
    r = np.abs(x.real).astype(np.float64)
    i = np.abs(x.imag).astype(np.float64)
    return np.where(r > i, r + 0.4 * i, i + 0.4 * r).astype(f32)


def window_max(env, nsamples):
    """M[n] = max(1e-4f, max env[n-N+1 .. n]) with env = 0 before the start"""
    env = np.asarray(env, dtype=f32)
    padded = np.concatenate([np.zeros(nsamples - 1, dtype=f32), env])
    out = np.empty(len(env), dtype=f32)
    step = max(1, (1 << 24) // max(nsamples, 1))          # bounded temporaries for long windows
    for a in range(0, len(env), step):
        b = min(len(env), a + step)
        w = np.lib.stride_tricks.sliding_window_view(padded[a:b + nsamples - 1], nsamples)
        out[a:b] = w.max(axis=1)
    return np.maximum(MAX_ENV_FLOOR, out)


def feedforward_agc(x, nsamples=1024, reference=1.0):
    """feedforward_agc_cc(nsamples, reference) over x (complex64), the stream starting with zero history"""
    x = np.asarray(x, dtype=np.complex64)
    N = int(nsamples)
    assert 1 <= N
    g = f32(reference) / window_max(envelope(x), N)          # float32 / float32: one rounding
    xd = np.concatenate([np.zeros(N - 1, dtype=np.complex64), x])[: len(x)]
    out = np.empty(len(x), dtype=np.complex64)
    out.real = xd.real.astype(f32) * g                        # complex<float> * float: two float products
    out.imag = xd.imag.astype(f32) * g
    return out


def feedforward_agc_naive(x, nsamples=1024, reference=1.0):
    """GNU Radio's work() loop, literally (slow: small inputs only)"""
    x = np.asarray(x, dtype=np.complex64)
    N = int(nsamples)
    hist = np.concatenate([np.zeros(N - 1, dtype=np.complex64), x])
    out = np.empty(len(x), dtype=np.complex64)
    for i in range(len(x)):
        max_env = MAX_ENV_FLOOR
        for j in range(N):
            z = hist[i + j]
            r, im = abs(float(z.real)), abs(float(z.imag))
            e = f32(r + 0.4 * im if r > im else im + 0.4 * r)
            max_env = max(max_env, e)
        gain = f32(f32(reference) / max_env)
        z = hist[i]
        out[i] = complex(f32(z.real) * gain, f32(z.imag) * gain)
    return out
