"""-m gpu: what a second call means for a channel's optional stages, and that every stage's reader has a cursor of its own.

  stage           ring on re-call       from           read cursor
  symbol filter   kept                  kept           kept            (test 1: only the taps and the gain change)
  AGC             kept                  `produced`     `produced`      (test 2)
  symbol clock    new ring and state    `produced`     0               (test 2)
  voice chain     new                   `produced`     0               (test_gpu_audio.py)

Small rings (out_capacity 4096) and ragged pushes throughout: every stream that is compared wraps or is cut at odd places."""
import numpy as np
import pytest

import mm_ref as M
from oracle import grspec as G
from rcf import audio as host_audio
from rcf import synth

pytestmark = pytest.mark.gpu

CAP = 4096
BAR = 1e-4                    # rms bar of the symbol filter's stream (test_gpu_parity.py)


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _same_bits(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32),
                                  err_msg=str(what))


def _cuts(pieces):
    """input cuts of pushes that yield about `pieces` channel samples each (one per 96 inputs), ending at odd places"""
    at, cuts = 0, [0]
    for j, p in enumerate(pieces):
        at += 96 * p + (17 * (j + 1)) % 96
        cuts.append(at)
    return cuts


# ---------------------------------------------------------------------------------------------------------------- 1
PIECES1 = (1500, 2100, 1300, 1700, 2000, 2300, 1400)          # 12300 channel samples: three rings
GAIN_A, TAPS_A = 5.0, np.full(5, 0.2, dtype=np.float32)
GAIN_B, TAPS_B = 2.5, np.array([1.0, -1.0, 0.5], dtype=np.float32)


def _run1(nat, x, meta, recall):
    """-> (sym_from, produced at the re-call, produced at the end, fm x 1 from output 0 on, sym reads concatenated)"""
    cuts = _cuts(PIECES1)
    pre = G.low_pass_2(1.0, 25000.0, 6250.0, 500.0, 30.0, G.WIN_BLACKMAN)
    fm, sym = [], []
    with nat.Frontend(meta["fs"], device=0, block_capacity=96 * 2400, out_capacity=CAP) as fe:
        c1 = fe.chan_open(12500, meta["offset"] + 40.0)
        c2 = fe.chan_open_taps(c1, 1, pre, 0.0)
        sym_from = n_switch = None
        for j, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]), start=1):
            fe.push(x[a:b])
            fm.append(fe.chan_read_fm(c2, 1.0))
            if j == 2:
                sym_from = fe.chan_produced(c2)
                fe.chan_fm_filter(c2, GAIN_A, TAPS_A)
            if j == 3 or j >= 5:
                sym.append(fe.chan_read_sym(c2))
            if j == 4:
                n_switch = fe.chan_produced(c2)
                if recall:
                    fe.chan_fm_filter(c2, GAIN_B, TAPS_B)
        produced = fe.chan_produced(c2)
    return sym_from, n_switch, produced, np.concatenate(fm), np.concatenate(sym)


def _filtered(fm, sym_from, gain, taps):
    """sym[n] = sum_i taps[i] * gain * fm[n - i] for n >= sym_from, fm[m] = 0 for m < sym_from, in float64"""
    u = float(np.float32(gain)) * fm[sym_from:].astype(np.float64)
    return np.convolve(u, taps.astype(np.float64))[: len(u)]


def test_fm_filter_recall_keeps_ring_from_and_cursor_new_taps_apply_from_produced_on(gpu_required):
    """rcf_chan_fm_filter called a second time: the reader loses nothing and sees nothing twice, outputs up to the call keep
    the first taps (bit for bit those of a run that never re-calls), outputs from `produced` on use the new taps and gain
    over the discriminator history the ring kept."""
    nat = gpu_required
    n_in = _cuts(PIECES1)[-1]
    x, meta = synth.cfg1(seconds=n_in / 2.4e6, seed=2121)
    sym_from, n_switch, produced, fm, sym = _run1(nat, x, meta, recall=True)
    assert 0 < sym_from < n_switch < produced and produced > 3 * CAP - 96
    assert len(fm) == produced
    assert len(sym) == produced - sym_from                       # nothing lost, nothing repeated across the re-call
    a, b = _filtered(fm, sym_from, GAIN_A, TAPS_A), _filtered(fm, sym_from, GAIN_B, TAPS_B)
    n = np.arange(sym_from, produced)
    ref = np.where(n < n_switch, a, b)
    e = rms(sym, ref)
    # ... and the 16 outputs around the call on their own: there a switch that is one output early or late stands out
    k = n_switch - sym_from
    w = slice(k - 8, k + 8)
    e_w = rms(sym[w], ref[w])
    early, late = rms(np.where(n < n_switch - 1, a, b)[w], ref[w]), rms(np.where(n < n_switch + 1, a, b)[w], ref[w])
    print("sym after a re-call: %d items, rms error %.3e (around the call %.3e); the switch one output early %.3e, late %.3e"
          % (len(sym), e, e_w, early, late))
    assert min(early, late) > 10 * BAR                           # the two tap sets differ by far more than the bar
    assert e < BAR and e_w < BAR
    # the same cuts without the second call: equal up to the call, bit for bit
    f2, s2, p2, _, plain = _run1(nat, x, meta, recall=False)
    assert (f2, s2, p2) == (sym_from, n_switch, produced) and len(plain) == len(sym)
    _same_bits(sym[:k], plain[:k], "before the re-call")
    assert rms(plain, a) < BAR and rms(sym[k:], plain[k:]) > 10 * BAR


# ---------------------------------------------------------------------------------------------------------------- 2
PIECES2 = (1100, 1400, 1200, 900, 1300)                       # 5900 channel samples; the stages see the last 3400
OMEGA = 25000 / 3600.0                                        # the SmartNet clock (test_gpu_clock_mm.py)
KINDS = ("iq", "fm", "sym", "agc", "clock", "audio")


def _read(fe, c, kind):
    return {"iq": lambda: fe.chan_read_iq(c), "fm": lambda: fe.chan_read_fm(c, 1.0), "sym": lambda: fe.chan_read_sym(c),
            "agc": lambda: fe.chan_read_agc(c), "clock": lambda: fe.chan_read_clock(c), "audio": lambda: fe.chan_read_audio(c)}[kind]()


def _open2(nat, meta):
    fe = nat.Frontend(meta["fs"], device=0, block_capacity=96 * 2200, out_capacity=CAP)
    return fe, fe.chan_open(12500, meta["offset"])


def _attach2(fe, c):
    fe.chan_fm_filter(c, GAIN_A, TAPS_A)
    fe.chan_agc(c)
    fe.chan_clock_mm(c, OMEGA)
    host_audio.open_analog_voice(fe, c, 25000)


def test_six_readers_on_one_channel_each_with_its_own_cursor(gpu_required):
    """symbol filter, AGC, symbol clock and voice chain on one channel, attached after the second push; the six streams read
    after every push in another order each time are what one read at the end gives (IQ and discriminator: the ring's worth
    that is left of them).  Then the AGC's and the clock's rows of the re-call table."""
    nat = gpu_required
    cuts = _cuts(PIECES2 + (500,))
    x, meta = synth.cfg1(seconds=cuts[-1] / 2.4e6, seed=77)
    got = {k: [] for k in KINDS}
    fe, c = _open2(nat, meta)
    with fe:
        for j, (a, b) in enumerate(zip(cuts[:-2], cuts[1:-1])):
            fe.push(x[a:b])
            order = KINDS[j:] + KINDS[:j] if j % 2 == 0 else (KINDS[j:] + KINDS[:j])[::-1]
            for k in order:
                if j >= 2 or k in ("iq", "fm"):
                    got[k].append(_read(fe, c, k))
            if j == 1:
                attached = fe.chan_produced(c)
                _attach2(fe, c)
        produced = fe.chan_produced(c)
        # AGC off and on again, the clock restarted: both start over at `produced`
        fe.chan_agc(c, 0)
        fe.chan_agc(c)
        fe.chan_clock_mm(c, OMEGA)
        fe.push(x[cuts[-2]:])
        fresh = fe.chan_produced(c) - produced
        agc2, clk2, fm2 = fe.chan_read_agc(c), fe.chan_read_clock(c), fe.chan_read_fm(c, 5.0)
        n_clk2, _ = fe.chan_clock_produced(c)
        bank = nat.design_mmse_interpolator()
    got = {k: np.concatenate(v) for k, v in got.items()}
    once = {}
    fe, c = _open2(nat, meta)
    with fe:
        for j, (a, b) in enumerate(zip(cuts[:-2], cuts[1:-1])):
            fe.push(x[a:b])
            if j == 1:
                assert fe.chan_produced(c) == attached
                _attach2(fe, c)
        for k in KINDS[::-1]:
            once[k] = _read(fe, c, k)
    assert CAP < produced and produced - attached < CAP
    for k in KINDS:
        print("%s: %d items read in pieces, %d at once" % (k, len(got[k]), len(once[k])))
        assert len(once[k]) == min(len(got[k]), CAP) and len(once[k]) > 0, k
        assert (len(got[k]) > CAP) == (k in ("iq", "fm")), k
        _same_bits(got[k][-len(once[k]):].view(np.float32), once[k].view(np.float32), k)
    assert len(got["iq"]) == len(got["fm"]) == produced
    assert len(got["sym"]) == len(got["agc"]) == produced - attached
    # the AGC's reader starts at the new `produced`, the clock's at symbol 0 of a new clock_recovery_mm_ff
    assert 0 < fresh == len(fm2) == len(agc2)
    want, _ = M.clock_recovery_mm(fm2, OMEGA, taps=bank, unit_gain_input=False)
    assert n_clk2 == len(want) > 0
    _same_bits(clk2, want, "restarted clock")
