"""The Gardner / Costas stage without a GPU (rcf_chan_costas, rcf/p25.py, tests/gc_ref.py): the binding's names and
argument checks, the reference's loop parameters, the slicer rule, and the restatement of the stage's definition fed by
the oracle chain (xlating_fir_ccc twice, feedforward_agc): it decodes what was sent, does not depend on how its input is
cut, and its float32 and float64 runs stay within rounding noise of each other -- the distance the GPU test
(tests/test_gpu_costas.py) takes as its yardstick.  The stage is defined by include/rcf.h and unpinned against op25."""
import hashlib
import math

import numpy as np
import pytest

import agc_ref as A
import gc_ref as R
import mm_ref as M
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


# ---- the inputs of the GPU tests beyond the P25 operating point: each case is decided here, on the oracle chain, by the
# conditions its test names; the yardsticks printed are those of the oracle chain's stream (the GPU tests take theirs from
# the GPU's own AGC stream)

CASES_F32_SHA256 = "2073803575fac8fe94791b88a04b7687848831646eca818786dcda26fa764562"


def test_float32_outputs_on_the_cases_are_the_recorded_bits(chain):
    """the restatement counts the window clamp and nothing else about it has changed: the float32 soft symbols of the
    five CASES, concatenated, hash to what they did before the counter went in"""
    h = hashlib.sha256()
    for case in R.CASES:
        h.update(np.ascontiguousarray(chain[case]["s32"], dtype=f32).tobytes())
        assert chain[case]["g32"].n_clamped == 0 and chain[case]["g32"].clamped == []
    assert h.hexdigest() == CASES_F32_SHA256


def _standard_chain(x):
    """the channel filter and the pre-filter of the standard chain -> what the AGC reads, and the channel samples the chain
    with its AGC holds a symbol back"""
    D, taps = G.channel_params(R.FS, R.CHANNEL_RATE)
    pre = G.low_pass_2(1.0, 2 * R.CHANNEL_RATE, R.CHANNEL_RATE / 2, 500, 30, G.WIN_BLACKMAN)
    with np.errstate(all="ignore"):
        y1 = G.xlating_fir_ccc(x, D, taps, R.CHANNEL_OFFSET, R.FS)
        return G.xlating_fir_ccc(y1, 1, pre, 0.0, 2.0 * R.CHANNEL_RATE), R.chain_delay(1.0, len(taps), D, len(pre))


def _agc_dropping_nan(y, n):
    """feedforward_agc_cc as GNU Radio's loop and the GPU's fmaxf run it on non-finite input: a NaN envelope never wins
    the window's maximum (agc_ref.feedforward_agc_naive does the same; numpy's max in feedforward_agc would spread it)"""
    env = A.envelope(y)
    g = f32(1.0) / A.window_max(np.where(np.isnan(env), f32(0), env), n)
    yd = np.concatenate([np.zeros(n - 1, dtype=np.complex64), y])[:len(y)]
    out = np.empty(len(y), dtype=np.complex64)
    with np.errstate(all="ignore"):
        out.real = yd.real * g
        out.imag = yd.imag * g
    return out


@pytest.mark.parametrize("case", R.CASES)
def test_the_start_has_a_yardstick_too(chain, case):
    """symbols [0, SKIP) and the first 16, which the GPU parity test compares as well.  The AGC of 1024 delivers zeros for
    its first 1023 outputs, about 196 symbols: the first 16 are 0 in both runs, and what that range checks is that a loop
    fed zeros puts out zeros.  Symbols that follow a start on a live signal are those of the AGC-64 cases (the mixed-rate
    lanes, the lanes of the 130-channel test, gain_mu -40), compared from symbol 0"""
    c = chain[case]
    rms, mx = R.distance(c["s32"], c["s64"], 0, R.SKIP)
    _, mx16 = R.distance(c["s32"], c["s64"], 0, 16)
    print("%s: float32 against float64 restatement over [0, %d): rms %.3e, max %.3e; max over the first 16: %.3e"
          % (case, R.SKIP, rms, mx, mx16))
    assert 0 < rms < 0.05 and mx16 <= mx < 0.05


@pytest.fixture(scope="module")
def mixed(bank):
    x, sent = R.mixed_signal()
    out = []
    for k, (cr, baud, off, cfo, timing, late, own, skip) in enumerate(R.MIXED):
        D, taps = G.channel_params(R.FS, cr)
        agc = A.feedforward_agc(G.xlating_fir_ccc(x, D, taps, off, R.FS), R.MIXED_AGC_N, 1.0)
        a = agc[late * R.MIXED_BLK // D:]                     # the loop starts at the channel's next output
        params = p25.costas_params(cr, baud)
        T = M.linear_bank() if own else bank
        s32, g32 = R.gardner_costas(a, params, T)
        s64, g64 = R.gardner_costas(a, params, T, dtype=np.float64)
        out.append(dict(n_in=len(a), params=params, s32=s32, g32=g32, s64=s64, g64=g64,
                        sent=sent[k][late * R.MIXED_BLK * baud // int(R.FS):],
                        delay=R.chain_delay(params["omega"], len(taps), D, pre_ntaps=1, agc_n=R.MIXED_AGC_N)))
    return out


def test_mixed_rate_cases_meet_their_conditions(mixed):
    rows = R.MIXED
    assert len(rows) <= 8 and {2 * r[0] for r in rows} == {12500, 25000, 50000}
    assert [r[0] for r in rows[:3]] == [25000, 6250, 12500]   # the rates interleave across the lanes
    assert sum(r[5] > 0 for r in rows) == 1 and sum(r[6] for r in rows) == 1
    for a in rows:
        for b in rows:                                        # 50 kS/s neighbours at least 50 kHz apart
            assert a is b or 25000 not in (a[0], b[0]) or abs(a[2] - b[2]) >= 50000.0
    seen = set()
    for k, (row, m) in enumerate(zip(rows, mixed)):
        cr, baud, off, cfo, timing, late, own, skip = row
        omega, L = m["params"]["omega"], m["g32"].L
        seen.add((2 * cr, baud))
        assert m["n_in"] == (R.MIXED_BLOCKS - late) * R.MIXED_BLK * 2 * cr // int(R.FS)
        rms, mx = R.distance(m["s32"], m["s64"])
        errs = None if skip is None else R.decode_errors(m["s32"], m["sent"], m["delay"], skip=skip)
        print("mixed %d: %d S/s, %d baud, omega %.4f, L %d, %d symbols in both runs, slips %d, clamped %d; float32 against "
              "float64 from symbol 0: rms %.3e, max %.3e; (lag, dibit errors) after %s: %s"
              % (k, 2 * cr, baud, omega, L, len(m["s32"]), m["g32"].n_slips, m["g32"].n_clamped, rms, mx, skip, errs))
        assert len(m["s32"]) == len(m["s64"]) <= 2500
        assert m["g32"].n_slips == m["g64"].n_slips == 0
        assert 0 < rms < 0.05
        if skip is not None:
            assert errs[1] == 0 and R.decode_errors(m["s64"], m["sent"], m["delay"], skip=skip)[1] == 0
            assert len(m["s32"]) - skip >= 70
    # the table's rows and the P25 shape
    assert {(12500, 2400), (25000, 3125), (50000, 9600), (50000, 3125), (12500, 6000), (25000, 4800)} <= seen
    assert mixed[3]["params"]["omega"] == 16.0 and mixed[3]["g32"].L == 32
    assert abs(mixed[4]["params"]["omega"] - 2.0833) < 1e-4 and mixed[4]["g32"].L == 10
    assert mixed[2]["g32"].L == 16 and mixed[0]["g32"].L == mixed[1]["g32"].L == 12


def test_window_clamp_case_is_comparable_over_a_prefix(bank):
    x, _ = R.case_signal(*R.CLAMP_CASE)
    y, _ = _standard_chain(x)
    agc = A.feedforward_agc(y, R.AGC_N, 1.0)
    params = dict(p25.costas_params(R.CHANNEL_RATE, R.CLAMP_CASE[0]), **R.CLAMP_PARAMS)
    s32, g32 = R.gardner_costas(agc, params, bank)
    s64, g64 = R.gardner_costas(agc, params, bank, dtype=np.float64)
    P, hits = R.comparable_prefix(s32, g32, s64, g64)
    _, mx = R.distance(s32, s64, 0, P)
    print("window clamp %s %s: L %d, %d / %d symbols, clamp taken %d / %d times; comparable prefix P = %d with %d hits, "
          "the first at %s; float32 against float64 over [0, P): max %.3e"
          % (R.CLAMP_CASE, R.CLAMP_PARAMS, g32.L, len(s32), len(s64), g32.n_clamped, g64.n_clamped, P, len(hits), hits[:3], mx))
    assert g32.L - R.NTAPS == 2 and params["omega"] - params["omega_limit"] - params["gain_mu"] >= 2
    assert P >= 64 and len(hits) >= 3 and mx < 0.05
    assert abs(len(s32) - len(s64)) <= 2 and np.isfinite(s32).all() and g32.n_slips == 0
    assert abs(float(g32.omega) - float(g32.omega_mid)) <= float(g32.omega_limit) * (1 + 1e-6)


@pytest.mark.parametrize("k", range(len(R.BURSTS)))
def test_burst_cases_come_back_alike_in_both_runs(bank, k):
    case, value, at, count, tail_errors = R.BURSTS[k]
    x, sent = R.burst_signal(case, value, at, count)
    y, delay1 = _standard_chain(x)
    params = p25.costas_params(R.CHANNEL_RATE, case[0])
    delay = int(delay1 / params["omega"])
    assert 0 < (~np.isfinite(y)).sum() < 100
    # the oracle's FIR (complex128 products) turns inf + 0j into NaN, which the AGC drops; a filter that keeps an Inf
    # zeroes the AGC's gain for the window in front of it instead.  Both are run: the drop-out is the second
    streams = [y] + ([np.where(np.isfinite(y), y, np.complex64(complex(np.inf, 0.0)))] if np.isinf(value.real) else [])
    assert any(np.isinf(b[1].real) for b in R.BURSTS) and any(np.isnan(b[1].real) for b in R.BURSTS)
    for y in streams:
        agc = _agc_dropping_nan(y, R.AGC_N)
        s32, g32 = R.gardner_costas(agc, params, bank)
        s64, g64 = R.gardner_costas(agc, params, bank, dtype=np.float64)
        bad32, bad64 = np.flatnonzero(~np.isfinite(s32)), np.flatnonzero(~np.isfinite(s64))
        a, b = R.burst_span(agc, params["omega"])
        assert len(s32) == len(s64) and g32.n_slips == g64.n_slips > 0
        assert np.array_equal(bad32, bad64) and 0 < len(bad32) < 0.02 * len(s32) and a <= bad32[0] and bad32[-1] <= b
        fin = np.isfinite(s32)
        before, after = R.distance(s32, s64, 0, a, fin), R.distance(s32, s64, b + R.SKIP, None, fin)
        lag, errs = R.decode_errors(s32, sent, delay, skip=b + R.SKIP)
        print("burst %s, %d x %s at input %d (%d AGC outputs zeroed): %d symbols, %d slips, %d non-finite symbols in %d .. %d "
              "in both runs; float32 against float64 before symbol %d: rms %.3e, max %.3e; after symbol %d: rms %.3e; "
              "lag %d, %d dibit errors in the tail of %d"
              % (case, count, value, at, int((agc[len(agc) // 4:] == 0).sum()), len(s32), g32.n_slips, len(bad32), bad32[0], bad32[-1],
                 a, before[0], before[1], b + R.SKIP, after[0], lag, errs, len(s32) - b - R.SKIP))
        assert a > 1000 and len(s32) - b - R.SKIP > 200
        assert 0 < before[0] < 0.05 and 0 < after[0] < 0.05
        assert errs == tail_errors and R.decode_errors(s64, sent, delay, skip=b + R.SKIP)[1] == tail_errors
        assert all(np.isfinite(v) for v in (g32.mu, g32.omega, g32.phase, g32.freq))
    assert any(b[4] == 0 for b in R.BURSTS)


@pytest.mark.parametrize("gain_mu", R.MU_GAINS)
def test_mu_guard_cases_agree_in_both_runs(bank, gain_mu):
    x, _ = R.case_signal(*R.CASES[0], n_symbols=R.MU_SYMBOLS)
    D, taps = G.channel_params(R.FS, R.CHANNEL_RATE)
    agc = A.feedforward_agc(G.xlating_fir_ccc(x, D, taps, R.CHANNEL_OFFSET, R.FS), R.MU_AGC_N, 1.0)
    params = dict(p25.costas_params(R.CHANNEL_RATE, R.CASES[0][0]), gain_mu=gain_mu)
    s32, g32 = R.gardner_costas(agc, params, bank)
    s64, g64 = R.gardner_costas(agc, params, bank, dtype=np.float64)
    first = R.symbols_before_first_slip(agc, params, bank)
    print("gain_mu %g: %d / %d symbols of %d sent, %d / %d slips, the first after symbol %s; mu at the end %g"
          % (gain_mu, len(s32), len(s64), R.MU_SYMBOLS, g32.n_slips, g64.n_slips, first, g32.mu))
    assert len(s32) == len(s64) and g32.n_slips == g64.n_slips and np.isfinite(s32).all()
    assert first == R.symbols_before_first_slip(agc, params, bank, dtype=np.float64)
    if gain_mu == -40.0:
        assert g32.n_slips > 0 and 16 <= first < len(s32) < R.MU_SYMBOLS
        _, mx = R.distance(s32, s64, 0, first)
        print("    float32 against float64 over the %d symbols before the first slip: max %.3e" % (first, mx))
        assert 0 < mx < 0.05
    else:                                                     # one huge step of mu, and no input brings it back
        assert g32.n_slips == 0 and first is None and len(s32) < 32 and g32.mu > 1e30
        again, g = R.gardner_costas(np.concatenate([agc, agc]), params, bank)
        assert len(again) == len(s32) and g.n_slips == 0
