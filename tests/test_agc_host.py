"""The P25 CQPSK front half without a GPU: the feedforward_agc_cc restatement's known answers (tests/agc_ref.py), the
pre-filter rcf.p25 derives, and the batched readers' "agc" stream in the binding."""
import numpy as np
import pytest

import agc_ref as A

f32 = np.float32


def _rng_iq(rng, n, scale=1.0):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


@pytest.mark.parametrize("N", [1, 2, 7, 64])
def test_first_outputs_are_zero_and_the_rest_is_the_delayed_input(N):
    rng = np.random.default_rng(11 + N)
    x = _rng_iq(rng, 400)
    y = A.feedforward_agc(x, N, 1.0)
    assert len(y) == len(x)
    assert np.all(y[: N - 1] == 0)
    # out[n] is x[n - N + 1] times one real gain
    g = y[N - 1:] / x[: len(x) - N + 1]
    np.testing.assert_allclose(g.imag, 0, atol=1e-5 * np.abs(g).max())


@pytest.mark.parametrize("N,R", [(1, 1.0), (2, 1.0), (7, 0.37), (33, -2.5), (64, 1.0)])
def test_vectorised_restatement_equals_the_naive_loop(N, R):
    rng = np.random.default_rng(100 + N)
    x = _rng_iq(rng, 300, 0.5)
    x[50:60] = 0                                   # envelope below the floor inside the stream
    x[120] = complex(0.25, -0.25)                  # |re| == |im|
    x[121] = complex(-3.0, 0.0)
    a = A.feedforward_agc(x, N, R)
    b = A.feedforward_agc_naive(x, N, R)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_gain_changes_n_minus_1_samples_before_a_step_reaches_the_output():
    N, s, n = 64, 500, 1200
    z = np.complex64(np.exp(0.3j))
    amp = np.where(np.arange(n) < s, f32(0.1), f32(1.0)).astype(f32)
    x = (amp * z).astype(np.complex64)
    y = A.feedforward_agc(x, N, 1.0)
    g_lo = f32(1.0) / A.envelope(np.array([x[0]]))[0]          # before the step: 1 / env(0.1 z)
    g_hi = f32(1.0) / A.envelope(np.array([x[-1]]))[0]         # once the step is in the window: 1 / env(z)
    gain = (np.abs(y[N - 1:]) / np.abs(x[: n - N + 1])).astype(np.float64)
    idx = np.arange(N - 1, n)
    np.testing.assert_allclose(gain[idx < s], g_lo, rtol=1e-6)
    np.testing.assert_allclose(gain[idx >= s], g_hi, rtol=1e-6)
    # the gain drops at n = s; the step itself reaches the output N - 1 samples later
    mag = np.abs(y)
    assert np.all(mag[N - 1:s] > 0.5) and np.all(mag[s:s + N - 1] < 0.2) and np.all(mag[s + N - 1:] > 0.5)
    assert abs(float(mag[s - 1]) - float(mag[s])) > 0.5 and abs(float(mag[s + N - 2]) - float(mag[s + N - 1])) > 0.5


def test_input_below_the_floor_is_held_at_gain_r_times_1e4():
    rng = np.random.default_rng(5)
    x = _rng_iq(rng, 500, 1e-6)                               # every envelope < 1e-4
    assert A.envelope(x).max() < 1e-4
    for R in (1.0, 0.5, -3.0):
        y = A.feedforward_agc(x, 16, R)
        g = f32(R) / f32(1e-4)
        assert abs(float(g) - R * 1e4) <= abs(R) * 1e4 * 1e-6
        want = np.empty(len(x) - 15, dtype=np.complex64)
        want.real = x.real[:-15] * g
        want.imag = x.imag[:-15] * g
        np.testing.assert_array_equal(y[15:].view(np.uint32), want.view(np.uint32))


def test_envelope_is_one_rounding_of_the_float64_evaluation():
    rng = np.random.default_rng(9)
    vals = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-30, 30, 2000),
                           [0.0, -0.0, 1e-45, -1e-45, 3.4e38, 1.0, -1.0, 0.4, 2.5]]).astype(f32)
    re = vals
    im = np.roll(vals, 7)
    im[:9] = re[:9]                                           # |re| == |im| takes the second branch
    x = (re + 1j * im.astype(np.complex64)).astype(np.complex64)
    got = A.envelope(x)
    for k in range(len(x)):
        r, i = abs(float(re[k])), abs(float(im[k]))
        want = f32(r + 0.4 * i) if r > i else f32(i + 0.4 * r)
        assert got[k].view(np.uint32) == want.view(np.uint32), (k, re[k], im[k])


def test_envelope_rounds_once_not_twice():
    # a value where rounding 0.4 |im| to float first would give a different float: the double path must be taken
    rng = np.random.default_rng(3)
    re = rng.uniform(1.0, 2.0, 20000).astype(f32)
    im = rng.uniform(0.0, 1.0, 20000).astype(f32)
    x = (re + 1j * im).astype(np.complex64)
    got = A.envelope(x)
    twice = (re + f32(0.4) * im).astype(f32)
    once = (re.astype(np.float64) + 0.4 * im.astype(np.float64)).astype(f32)
    np.testing.assert_array_equal(got, once)
    assert np.any(got != twice)


def test_p25_prefilter_taps_equal_the_oracle():
    from rcf import p25
    from oracle import grspec as G
    taps = p25.prefilter_taps(12500)
    want = G.low_pass_2(1.0, 25000, 6250, 500, 30, G.WIN_BLACKMAN)
    assert len(taps) == 69
    np.testing.assert_array_equal(taps, want)
    assert p25.fm_gain(12500) == G.p25_fm_gain(25000.0)
    assert p25.symbol_taps(12500) == [0.2] * 5


def test_p25_front_halves_pick_by_modulation():
    from rcf import p25
    calls = []

    class FakeFrontend:
        def chan_open_taps(self, src, decim, taps, offset_hz):
            calls.append(("open", src, decim, len(taps), offset_hz))
            return 77

        def chan_agc(self, cid, nsamples, reference):
            calls.append(("agc", cid, nsamples, reference))

        def chan_fm_filter(self, cid, gain, taps):
            calls.append(("sym", cid, round(gain, 6), list(taps)))

    fe = FakeFrontend()
    assert p25.front_half(fe, 5, 12500, "CQPSK") == 77
    assert calls == [("open", 5, 1, 69, 0.0), ("agc", 77, 1024, 1.0)]
    calls.clear()
    assert p25.front_half(fe, 5, 12500, "C4FM") == 77
    assert calls == [("open", 5, 1, 69, 0.0), ("sym", 77, round(25000 / (2 * np.pi * 600), 6), [0.2] * 5)]
    with pytest.raises(ValueError):
        p25.front_half(fe, 5, 12500, "FM")


def test_binding_maps_the_agc_stream_explicitly():
    from rcf import native
    assert native.READ_AGC == 2
    for s in ("rcf_chan_agc", "rcf_chan_read_agc", "rcf_chan_agc_ring"):
        assert s in native.SYMBOLS and hasattr(native.lib(), s)
    assert native._read_what("iq") == native.READ_IQ
    assert native._read_what("agc") == native.READ_AGC
    for other in ("fm", "FM", "sym", None):                   # anything else stays the discriminator, as before
        assert native._read_what(other) == native.READ_FM
    assert native._read_dtype("agc") == np.complex64 and native._read_dtype("fm") == np.float32
