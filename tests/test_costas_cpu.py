"""The Gardner / Costas stage without a GPU (rcf_chan_costas, rcf/p25.py, tests/gc_ref.py): the binding's names and
argument checks, the reference's loop parameters, the slicer rule, and the restatement of the stage's definition fed by
the oracle chain (xlating_fir_ccc twice, feedforward_agc): it decodes what was sent, does not depend on how its input is
cut, and its float32 and float64 runs stay within rounding noise of each other -- the distance the GPU test
(tests/test_gpu_costas.py) takes as its yardstick.  The stage is defined by include/rcf.h and unpinned against op25."""
import math

import numpy as np
import pytest

import agc_ref as A
import gc_ref as R
from oracle import grspec as G
from rcf import native, p25

f32 = np.float32


@pytest.fixture(scope="module")
def bank():
    return native.design_mmse_interpolator()


@pytest.fixture(scope="module")
def chain(bank):
    """per case: the AGC output of the oracle chain, the dibits sent, the float32 and float64 runs of the restatement"""
    D, taps = G.channel_params(R.FS, R.CHANNEL_RATE)
    pre = G.low_pass_2(1.0, 2 * R.CHANNEL_RATE, R.CHANNEL_RATE / 2, 500, 30, G.WIN_BLACKMAN)
    out = {}
    for case in R.CASES:
        baud, cfo, timing = case
        x, sent = R.case_signal(baud, cfo, timing)
        y1 = G.xlating_fir_ccc(x, D, taps, R.CHANNEL_OFFSET, R.FS)
        y2 = G.xlating_fir_ccc(y1, 1, pre, 0.0, 2.0 * R.CHANNEL_RATE)
        agc = A.feedforward_agc(y2, R.AGC_N, 1.0)
        params = p25.costas_params(R.CHANNEL_RATE, baud)
        s32, g32 = R.gardner_costas(agc, params, bank)
        s64, g64 = R.gardner_costas(agc, params, bank, dtype=np.float64)
        out[case] = dict(agc=agc, sent=sent, params=params, s32=s32, g32=g32, s64=s64, g64=g64,
                         delay=R.chain_delay(params["omega"], len(taps), D, len(pre)))
    return out


def test_names_and_argument_checks():
    assert native.T_COSTAS == 11
    for s in ("rcf_chan_costas", "rcf_chan_costas_state", "rcf_chan_read_costas", "rcf_chan_costas_ring"):
        assert s in native.SYMBOLS and hasattr(native.lib(), s)
    for m in ("chan_costas", "chan_costas_state", "chan_read_costas", "chan_costas_ring"):
        assert callable(getattr(native.Frontend, m))
    p, keep = native.costas_params_struct(25000 / 4800, 0.025, 6.25e-5, 0.04, 2e-4, 0.3, 0.005)
    assert keep is None and not p.interp_taps and p.omega == f32(25000 / 4800) and p.omega_limit == f32(0.005)
    T = np.zeros((129, 8), dtype=np.float32)
    p, keep = native.costas_params_struct(5.0, 0.025, 6.25e-5, 0.04, 2e-4, 0.3, 0.005, T)
    assert keep is not None and bool(p.interp_taps)
    with pytest.raises(ValueError):
        native.costas_params_struct(5.0, 0.025, 6.25e-5, 0.04, 2e-4, 0.3, 0.005, np.zeros((128, 8), dtype=np.float32))
    # the ABI refuses a null handle before it touches anything
    assert native.lib().rcf_chan_costas(None, 1, None) == native.RCF_EINVAL
    assert native.lib().rcf_chan_costas_state(None, 1, None) == native.RCF_EINVAL
    assert native.lib().rcf_chan_read_costas(None, 1, None, 0) == native.RCF_EINVAL
    assert native.lib().rcf_chan_costas_ring(None, 1, None, None) == native.RCF_EINVAL


@pytest.mark.parametrize("symbol_rate,omega,window", [(4800, 25000 / 4800, 12), (6000, 25000 / 6000, 11)])
def test_costas_params_are_the_references(symbol_rate, omega, window):
    p = p25.costas_params(12500, symbol_rate)
    assert p == R.costas_params(12500, symbol_rate)
    assert p["omega"] == omega and p["gain_mu"] == 0.025 and p["gain_omega"] == 0.1 * 0.025 * 0.025
    assert abs(p["gain_omega"] - 6.25e-5) < 1e-18
    assert p["alpha"] == 0.04 and p["beta"] == 0.125 * 0.04 * 0.04
    assert p["max_freq"] == 2 * math.pi * 1200 / 25000.0 and p["omega_limit"] == 0.005
    assert R.window_length(omega) == window
    assert p["omega"] - p["omega_limit"] - p["gain_mu"] >= 2 and p["max_freq"] < math.pi


def test_slice_dibits_on_the_level_edges():
    below = np.nextafter(f32(0), f32(-1))
    soft = np.array([-3.0, -2.0, np.nextafter(f32(-2), f32(-3)), -1.0, below, 0.0, 1.0, np.nextafter(f32(2), f32(0)), 2.0, 3.0, 4.0, 5.0,
                     -4.0, 3.999], dtype=f32)
    want = [3, 2, 3, 2, 2, 0, 0, 0, 1, 1, 1, 1, 3, 1]
    assert p25.slice_dibits(soft).tolist() == want
    assert R.slice_dibits(soft).tolist() == want
    assert p25.slice_dibits(soft).dtype == np.uint8
    assert p25.slice_dibits([0.5, 1.5], levels=(-1.0, 0.0, 1.0, 2.0)).tolist() == [0, 1]
    # the modulator's dibits come back through a perfect differential detector
    steps = np.asarray(R.STEP_OF_DIBIT, dtype=f32)
    assert p25.slice_dibits(steps).tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_decodes_the_sent_dibits(chain, case):
    c = chain[case]
    assert len(R.CASES) >= 3 and {b for b, _, _ in R.CASES} == {4800, 6000}
    assert any(f > 0 for _, f, _ in R.CASES) and any(f < 0 for _, f, _ in R.CASES)
    assert abs(len(c["s32"]) - R.N_SYMBOLS) <= 2
    lag, errs = R.decode_errors(c["s32"], c["sent"], c["delay"], skip=R.SKIP)
    print("%s: %d symbols, chain delay %d + lag %d, %d errors after the first %d, slips %d, freq %.5f rad/sample"
          % (case, len(c["s32"]), c["delay"], lag, errs, R.SKIP, c["g32"].n_slips, c["g32"].freq))
    assert errs == 0
    assert c["g32"].n_slips == 0
    assert c["g32"].freq * case[1] < 0                        # the carrier estimate opposes the offset
    assert R.decode_errors(c["s64"], c["sent"], c["delay"], skip=R.SKIP)[1] == 0


def test_restatement_does_not_depend_on_the_cuts(chain, bank):
    case = R.CASES[0]
    c = chain[case]
    n = len(c["agc"])
    rng = np.random.default_rng(5)
    cuts = sorted({0, n} | {int(v) for v in rng.integers(1, n, 40)} | {3000 + k for k in range(12)} | {5000 + 3 * k for k in range(8)})
    s, g = R.gardner_costas(c["agc"], c["params"], bank, cuts=cuts)
    assert s.tobytes() == c["s32"].tobytes()
    assert (g.n_symbols, g.n_slips, g.mu, g.omega, g.freq, g.phase) == \
        (c["g32"].n_symbols, c["g32"].n_slips, c["g32"].mu, c["g32"].omega, c["g32"].freq, c["g32"].phase)


@pytest.mark.parametrize("case", R.CASES)
def test_float32_and_float64_runs_differ_by_rounding_noise(chain, case):
    """the yardstick of the GPU parity test, recorded here: rms distance of the two runs after the first 500 symbols"""
    c = chain[case]
    n = min(len(c["s32"]), len(c["s64"]))
    assert abs(len(c["s32"]) - len(c["s64"])) <= 1
    rms = float(np.sqrt(np.mean(R.angle_diff_mod8(c["s32"][R.SKIP:n], c["s64"][R.SKIP:n]) ** 2)))
    print("%s: float32 against float64 restatement: rms %.3e soft-symbol units over %d symbols" % (case, rms, n - R.SKIP))
    # both are the same loop on the same input: far below the 1.0 that separates a symbol from the slicer's levels
    assert 0 < rms < 0.05
