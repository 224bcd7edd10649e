"""The C4FM symbol loop without a GPU (rcf_chan_fsk4, rcf/p25.py, tests/fsk4_ref.py): the binding's names and argument
checks, op25's loop constants, and the restatement of the stage's definition fed by the oracle chain (xlating_fir_ccc
twice, quadrature_demod_cf at p25.fm_gain, the boxcar).  This test decides the inputs of the GPU test
(tests/test_gpu_fsk4.py): a case is kept if the float64 restatement -- the definition -- decodes it without a dibit error
after the first 500 of 1500 symbols and without a slip.  It also shows that the restatement does not depend on how its
input is cut, that the guard brings the loop back after NaN, Inf and 1e30, that `fine` and `coarse` take the sign of the
carrier's offset, and records the distance between the float32-state and the float64 run, the GPU test's yardstick.  The
stage is defined by include/rcf.h and unpinned against op25.

Of the candidates (baud, offset, timing, deviation) that decoded on a bare discriminator, (4800, 0, 0.0, 600) does not
behind the filters (728 dibit errors: a lock half a symbol off) and (4800, -200, 0.3, 600) only just (its float32-state run
has a dibit error); timings 0.4 and 0.5 replace them, and (6000, -150, 0.2, 600) was added."""
import numpy as np
import pytest

import fsk4_ref as F
from oracle import grspec as G
from rcf import native, p25

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def bank():
    return native.design_mmse_interpolator()


def _oracle_chain(x, baud):
    """-> (the symbol filter's output of the oracle chain, whole symbols the chain holds a symbol back)"""
    D, taps = G.channel_params(F.FS, F.CHANNEL_RATE)
    pre = G.low_pass_2(1.0, 2 * F.CHANNEL_RATE, F.CHANNEL_RATE / 2, 500, 30, G.WIN_BLACKMAN)
    y1 = G.xlating_fir_ccc(x, D, taps, F.CHANNEL_OFFSET, F.FS)
    y2 = G.xlating_fir_ccc(y1, 1, pre, 0.0, 2.0 * F.CHANNEL_RATE)
    fm = G.quadrature_demod_cf(y2, np.float32(p25.fm_gain(F.CHANNEL_RATE)))
    sps = len(p25.symbol_taps(F.CHANNEL_RATE, baud))
    return F.symbol_filter(fm, sps), F.chain_delay(2.0 * F.CHANNEL_RATE / baud, len(taps), D, len(pre), sps)


def _run(case, bank):
    x, sent = F.case_signal(*case)
    u, delay = _oracle_chain(x, case[0])
    params = p25.fsk4_params(F.CHANNEL_RATE, case[0])
    s64, g64 = F.fsk4_demod(u, params, bank)
    s32, g32 = F.fsk4_demod(u, params, bank, dtype=np.float32)
    return dict(u=u, sent=sent, params=params, s64=s64, g64=g64, s32=s32, g32=g32, delay=delay)


@pytest.fixture(scope="module")
def chain(bank):
    return {case: _run(case, bank) for case in F.CASES}


def test_names_and_argument_checks():
    assert native.T_FSK4 == 12
    for s in ("rcf_chan_fsk4", "rcf_chan_fsk4_state", "rcf_chan_read_fsk4", "rcf_chan_fsk4_ring"):
        assert s in native.SYMBOLS and hasattr(native.lib(), s)
    for m in ("chan_fsk4", "chan_fsk4_state", "chan_read_fsk4", "chan_fsk4_ring"):
        assert callable(getattr(native.Frontend, m))
    p, keep = native.fsk4_params_struct(25000.0, 4800.0, 0.01, 0.025, 0.125, 0.00125, 1.6, 2.4)
    assert keep is None and not p.interp_taps and p.sample_rate == 25000.0 and p.k_coarse == 0.00125 and p.spread_max == 2.4
    p, keep = native.fsk4_params_struct(25000.0, 4800.0, 0.01, 0.025, 0.125, 0.00125, 1.6, 2.4, np.zeros((129, 8), dtype=np.float32))
    assert keep is not None and bool(p.interp_taps)
    with pytest.raises(ValueError):
        native.fsk4_params_struct(25000.0, 4800.0, 0.01, 0.025, 0.125, 0.00125, 1.6, 2.4, np.zeros((128, 8), dtype=np.float32))
    # the ABI refuses a null handle before it touches anything
    assert native.lib().rcf_chan_fsk4(None, 1, None) == native.RCF_EINVAL
    assert native.lib().rcf_chan_fsk4_state(None, 1, None) == native.RCF_EINVAL
    assert native.lib().rcf_chan_read_fsk4(None, 1, None, 0) == native.RCF_EINVAL
    assert native.lib().rcf_chan_fsk4_ring(None, 1, None, None) == native.RCF_EINVAL


@pytest.mark.parametrize("symbol_rate", [4800, 6000])
def test_fsk4_params_are_op25s(symbol_rate):
    p = p25.fsk4_params(12500, symbol_rate)
    assert p == F.fsk4_params(12500, symbol_rate)
    assert p == dict(sample_rate=25000.0, symbol_rate=float(symbol_rate), k_spread=0.01, k_timing=0.025, k_fine=0.125,
                     k_coarse=0.00125, spread_min=1.6, spread_max=2.4)
    assert p25.fsk4_params(12500)["symbol_rate"] == 4800.0
    assert 2 <= p["sample_rate"] / p["symbol_rate"] <= 4096 and 0 < p["spread_min"] <= 2 <= p["spread_max"]


def test_modulator_levels_and_slicer_agree():
    # a held dibit deviates by LEVEL_OF_DIBIT * deviation: the discriminator at p25.fm_gain reads +1, +3, -1, -3
    for dibit, level in enumerate(F.LEVEL_OF_DIBIT):
        x = F.c4fm_carrier(np.full(40, dibit), 4800, 48000.0, 0.0, deviation=600.0)
        fm = G.quadrature_demod_cf(x, np.float32(48000.0 / (2 * np.pi * 600.0)))
        assert abs(float(np.mean(fm[150:250])) - level) < 2e-2, (dibit, float(np.mean(fm[150:250])))
    assert p25.slice_dibits(np.asarray(F.LEVEL_OF_DIBIT, dtype=np.float32)).tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("case", F.CASES)
def test_restatement_decodes_the_sent_dibits(chain, case):
    c = chain[case]
    assert len(F.CASES) >= 4 and {k[0] for k in F.CASES} == {4800, 6000}
    for baud in (4800, 6000):                                 # both offset signs at both baud rates
        assert any(k[1] > 0 for k in F.CASES if k[0] == baud) and any(k[1] < 0 for k in F.CASES if k[0] == baud)
    assert abs(len(c["s64"]) - F.N_SYMBOLS) <= 2 and c["g64"].n_symbols == len(c["s64"])
    lag, errs = F.decode_errors(c["s64"], c["sent"], c["delay"], skip=F.SKIP)
    st = c["g64"].state()
    print("%s: %d symbols, chain delay %d + lag %d, %d errors after the first %d, slips %d, spread %.4f, fine %.4f, coarse %.4f"
          % (case, len(c["s64"]), c["delay"], lag, errs, F.SKIP, st["n_slips"], st["spread"], st["fine"], st["coarse"]))
    assert errs == 0 and st["n_slips"] == 0
    assert np.isfinite(c["s64"]).all() and 1.6 < st["spread"] < 2.4
    if case[1]:
        assert st["fine"] * case[1] > 0 and st["coarse"] * case[1] > 0        # both take the sign of the carrier's offset
        # ... and coarse its size, in level steps of `deviation` Hz at p25.fm_gain's 600: within 0.1 of a level step
        assert abs(st["coarse"] - case[1] / 600.0) < 0.1


def test_the_rejected_candidate_does_not_decode(bank):
    c = _run(F.REJECTED, bank)
    _, errs = F.decode_errors(c["s64"], c["sent"], c["delay"], skip=F.SKIP)
    print("%s: %d dibit errors after the first %d, slips %d" % (F.REJECTED, errs, F.SKIP, c["g64"].n_slips))
    assert errs > 100


def test_restatement_does_not_depend_on_the_cuts(chain, bank):
    case = F.CASES[1]
    c = chain[case]
    n = len(c["u"])
    rng = np.random.default_rng(5)
    cuts = sorted({0, n} | {int(v) for v in rng.integers(1, n, 40)} | {3000 + k for k in range(12)} | {5000 + 3 * k for k in range(8)})
    for dtype, s, g in ((np.float64, c["s64"], c["g64"]), (np.float32, c["s32"], c["g32"])):
        s2, g2 = F.fsk4_demod(c["u"], c["params"], bank, dtype=dtype, cuts=cuts)
        assert s2.tobytes() == s.tobytes() and g2.state() == g.state() and g2.imus == g.imus


@pytest.mark.parametrize("case", F.CASES)
def test_float32_state_and_float64_runs_differ_by_rounding_noise(chain, case):
    """the yardstick of the GPU parity test, recorded here.  The two runs round clock / time apart by ~1e-7 of a step, so
    that now and then floor() picks neighbouring rows of the bank: a row apart is 1 / 128 of a sample, about 1e-2 in a
    soft symbol at the steepest part of a transition"""
    c = chain[case]
    assert len(c["s32"]) == len(c["s64"])
    flips = sum(a != b for a, b in zip(c["g32"].imus, c["g64"].imus))
    for lo, hi in ((F.SKIP, None), (0, F.SKIP)):
        rms, mx = F.distance(c["s32"], c["s64"], lo, hi)
        print("%s: float32-state against float64 restatement over [%d, %s): rms %.3e, max %.3e; %d of %d symbols on another row"
              % (case, lo, hi, rms, mx, flips, len(c["s64"])))
        # the same loop on the same input: far below the 1.0 that separates a level from the slicer's thresholds
        assert 0 < rms <= mx < 0.05
    assert F.decode_errors(c["s32"], c["sent"], c["delay"], skip=F.SKIP)[1] == 0


@pytest.mark.parametrize("value", [NAN, INF, 1e30])
def test_guard_brings_the_loop_back(chain, bank, value):
    """a burst in the loop's own input: op25's loop would stay NaN for good; this one starts over and decodes again"""
    case = F.CASES[1]
    c = chain[case]
    at, count = 3000, 3                                       # symbol ~576: 74 locked symbols before it, 420 after the 500 that follow
    u = c["u"].copy()
    u[at:at + count] = value
    omega = c["params"]["sample_rate"] / c["params"]["symbol_rate"]
    hit = int(at / omega)
    for dtype in (np.float64, np.float32):
        s, g = F.fsk4_demod(u, c["params"], bank, dtype=dtype)
        lag, errs = F.decode_errors(s, c["sent"], c["delay"], skip=hit + F.SKIP)
        before = F.decode_errors(s[:hit - 2], c["sent"], c["delay"], skip=F.SKIP)[1]
        print("burst of %d x %s at input %d (symbol %d), %s state: %d symbols, %d slips, %d dibit errors later than %d symbols after it"
              % (count, value, at, hit, dtype.__name__, len(s), g.n_slips, errs, F.SKIP))
        # the guard fires at most once per symbol, and only while the burst is among the 8 inputs of the window (or, after
        # 1e30, in the symbol that follows): (3 + 7) inputs are two or three symbols
        assert 1 <= g.n_slips <= int((count + F.NTAPS) / omega) + 2
        assert errs == 0 and before == 0 and abs(len(s) - len(c["s64"])) <= 2
        assert all(np.isfinite(v) for v in g.state().values())
        assert np.isfinite(s[hit + 8:]).all()
        if dtype is np.float64:
            np.testing.assert_array_equal(s[:hit - 2], c["s64"][:hit - 2])

