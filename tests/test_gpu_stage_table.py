"""Every tail stage together (symbol filter, AGC, symbol clock, Gardner / Costas loop, C4FM loop): what the per-stage tests
do not cover in one place.  A group block that carries records of all five, with a loop attached inside a running group,
gives each member the bits it gives alone; and a symbol clock or a C4FM chain behind a stage-2 channel of a 256-bin bank
gives the same bits with the stage-2 lag on and off (a block with any tail record must not lag: the tail reads rings the
lagged launch has not written)."""
import numpy as np
import pytest

import fsk4_ref as F
import gc_ref as R
import mm_ref as M
from oracle import grspec as G
from rcf import control, p25, synth

pytestmark = pytest.mark.gpu

FS, CR = F.FS, F.CHANNEL_RATE
BLK, K = 16 * 1000, 5                                         # 1000 channel samples a block
N = BLK * K
LATE = 3                                                      # member 1's clock is attached before this block


def _same_bits(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    np.testing.assert_array_equal(np.ascontiguousarray(got, dtype=np.float32).view(np.uint32),
                                  np.ascontiguousarray(want, dtype=np.float32).view(np.uint32), err_msg=str(what))


def _same_iq(got, want, what=""):
    _same_bits(np.ascontiguousarray(got, dtype=np.complex64).view(np.float32),
               np.ascontiguousarray(want, dtype=np.complex64).view(np.float32), what)


# per member: (kind, channel offset) of its carriers, 100 kHz and more apart
CARRIERS = [
    [("c4fm", -140000.0), ("plain", 60000.0)],
    [("cqpsk", -150000.0), ("late clock", 120000.0)],
    [("c4fm", -160000.0), ("cqpsk", -20000.0), ("clock", 130000.0)],
]


def _signal(m):
    rng = np.random.default_rng(500 + m)
    x = np.zeros(N, dtype=np.complex128)
    for kind, off in CARRIERS[m]:
        if kind in ("c4fm", "plain"):
            x += F.c4fm_carrier(rng.integers(0, 4, N * 4800 // int(FS) + 2), 4800, FS, off + 80.0, 0.45, amplitude=0.3, n_samples=N)
        elif kind == "cqpsk":
            x += R.dqpsk_carrier(rng.integers(0, 4, N * 4800 // int(FS) + 2), 4800, FS, off + 100.0, 0.5, amplitude=0.3, n_samples=N)
        else:
            sent = rng.integers(0, 2, N * 9600 // int(FS) + 2)
            x += 0.3 * M.fsk2_carrier(sent, 9600.0, FS, off, 1200.0, rng)[:N]
    return x.astype(np.complex64)


def _setup(fe, m):
    """member m's channels and stages -> {name: channel id}; the late clock's channel is open, its clock comes later"""
    ids = {}
    for kind, off in CARRIERS[m]:
        c = fe.chan_open(CR, off)
        if kind == "c4fm":
            ids["fsk4"] = p25.c4fm_demod(fe, c, CR, 4800)
        elif kind == "cqpsk":
            ids["costas"] = p25.cqpsk_demod(fe, c, CR, 4800)
        elif kind == "clock":
            fe.chan_clock_mm(c, 25000 / 9600.0, interp_taps=M.linear_bank())      # a caller's bank
            ids["clock"] = c
        elif kind == "late clock":
            ids["clock"] = c
        else:
            ids["plain"] = c
    return ids


def _before_block(fe, m, ids, b):
    if m == 1 and b == LATE:
        control.edacs_clock(fe, ids["clock"])


def _read_all(fe, ids):
    out = {}
    if "fsk4" in ids:
        c = ids["fsk4"]
        out["fsk4"] = (fe.chan_read_fsk4(c), fe.chan_fsk4_state(c), fe.chan_read_sym(c))
    if "costas" in ids:
        c = ids["costas"]
        out["costas"] = (fe.chan_read_costas(c), fe.chan_costas_state(c), fe.chan_read_agc(c))
    if "clock" in ids:
        c = ids["clock"]
        out["clock"] = (fe.chan_read_clock(c), fe.chan_clock_produced(c), fe.chan_read_fm(c, 5.0))
    if "plain" in ids:
        out["plain"] = (fe.chan_read_fm(ids["plain"], 1.0), fe.chan_read_iq(ids["plain"]))
    return out


def test_every_tail_stage_in_one_group_block(gpu_required):
    nat = gpu_required
    xs = [_signal(m) for m in range(3)]
    loops = (nat.T_CLOCK, nat.T_COSTAS, nat.T_FSK4)
    fes = [nat.Frontend(FS, device=0, block_capacity=BLK) for _ in range(3)]
    try:
        ids = [_setup(fe, m) for m, fe in enumerate(fes)]
        fes[0].timing_enable(True, classes=list(loops))
        with nat.Group(fes) as g:
            for b in range(K):
                for m, fe in enumerate(fes):
                    _before_block(fe, m, ids[m], b)
                g.push([x[b * BLK:(b + 1) * BLK] for x in xs])
            g.sync()
            # merged launches are timed on the first member: one per group block in which any member had records
            # (member 2 carries all three loops from block 0)
            assert [fes[0].timing_read(t)[1] for t in loops] == [K, K, K]
            grouped = [_read_all(fe, ids[m]) for m, fe in enumerate(fes)]
    finally:
        for fe in fes:
            fe.close()
    assert [sorted(r) for r in grouped] == [["fsk4", "plain"], ["clock", "costas"], ["clock", "costas", "fsk4"]]
    for m in range(3):
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            own = _setup(fe, m)
            for b in range(K):
                _before_block(fe, m, own, b)
                fe.push(xs[m][b * BLK:(b + 1) * BLK])
            alone = _read_all(fe, own)
        got = grouped[m]
        for name in ("fsk4", "costas"):
            if name not in got:
                continue
            (soft, st, feed), (soft1, st1, feed1) = got[name], alone[name]
            print("member %d %s: %d symbols, %s" % (m, name, len(soft), st))
            _same_bits(soft, soft1, (m, name))
            assert st == st1 and st["n_symbols"] == len(soft), (m, name, st, st1)
            (_same_iq if name == "costas" else _same_bits)(feed, feed1, (m, name, "the stream it reads"))
            assert len(feed) == N // 16
            assert len(soft) > 500 and st["n_slips"] == 0, (m, name, len(soft), st)
        if "clock" in got:
            (sym, cnt, fm), (sym1, cnt1, fm1) = got["clock"], alone["clock"]
            print("member %d clock: %d symbols, %d slips" % (m, cnt[0], cnt[1]))
            _same_bits(sym, sym1, (m, "clock"))
            assert cnt == cnt1 and cnt[0] == len(sym), (m, cnt, cnt1)
            _same_bits(fm, fm1, (m, "clock fm"))
            assert len(sym) > 500 and cnt[1] == 0, (m, len(sym), cnt)
            # a late `from`: the clock attached inside the running group saw the last K - LATE blocks only
            n_in = (K - LATE if m == 1 else K) * BLK // 16
            assert abs(len(sym) - n_in * 9600 / 25000.0) <= 4, (m, len(sym), n_in)
        if "plain" in got:
            _same_bits(got["plain"][0], alone["plain"][0], (m, "plain fm"))
            _same_iq(got["plain"][1], alone["plain"][1], (m, "plain iq"))


S2_BLK, S2_BLOCKS = 256 * 16 * 40, 8


def _stage2(nat, x, lag, at, bank):
    """the shape of test_gpu_cqpsk._stage2: seven stage-2 channels on a 256-bin bank; before block `at` channel 2 gets a
    symbol clock, channel 4 a symbol filter and the C4FM loop; channel 3 stays as it is"""
    fs, nb = 20e6, 256
    bw = fs / nb
    proto = G.low_pass_2(1.0, fs, bw * 0.4, bw * 0.2, 60.0, G.WIN_BLACKMAN_HARRIS)
    with nat.Frontend(fs, 0.0, device=0, block_capacity=S2_BLK, hist_capacity=1 << 14, out_capacity=1 << 13) as fe:
        fe.set_stage2_lag(lag)
        fe.pfb_open(nb, nb, proto)
        ids = [fe.pfb_chan_open((5 + 17 * i) % nb, 12500, 12500.0 * ((i % 5) - 2)) for i in range(7)]
        omega = fe.chan_info(ids[2])["out_rate"] / 9600.0
        from_ = None
        for b in range(len(x) // S2_BLK):
            if b == at:
                from_ = (fe.chan_produced(ids[2]), fe.chan_produced(ids[4]))
                fe.chan_clock_mm(ids[2], omega)
                fe.chan_fm_filter(ids[4], p25.fm_gain(CR), p25.symbol_taps(CR))
                fe.chan_fsk4(ids[4], **p25.fsk4_params(CR))
            fe.push(x[b * S2_BLK:(b + 1) * S2_BLK])
        return dict(clock=fe.chan_read_clock(ids[2]), clock_n=fe.chan_clock_produced(ids[2]), clock_fm=fe.chan_read_fm(ids[2], 5.0),
                    fsk4=fe.chan_read_fsk4(ids[4]), fsk4_st=fe.chan_fsk4_state(ids[4]), sym=fe.chan_read_sym(ids[4]),
                    iq=fe.chan_read_iq(ids[4]), near_iq=fe.chan_read_iq(ids[3]), near_fm=fe.chan_read_fm(ids[3], 5.0),
                    omega=omega, from_=from_)


def test_clock_and_c4fm_behind_a_stage2_channel_do_not_lag(gpu_required):
    nat = gpu_required
    bank = nat.design_mmse_interpolator()
    x, _ = synth.cfg2(n=S2_BLOCKS * S2_BLK, seed=2300)
    for at in (0, 3):                                         # from the start, and attached while a launch lags
        on, off = _stage2(nat, x, True, at, bank), _stage2(nat, x, False, at, bank)
        assert on["from_"] == off["from_"] and on["clock_n"] == off["clock_n"] and on["fsk4_st"] == off["fsk4_st"], at
        for name in ("clock", "clock_fm", "fsk4", "sym", "near_fm"):
            _same_bits(on[name], off[name], ("lag", at, name))
        for name in ("iq", "near_iq"):
            _same_iq(on[name], off[name], ("lag", at, name))
        f_clock, f_sym = on["from_"]
        assert len(on["sym"]) == len(on["iq"]) - f_sym and len(on["sym"]) > 500
        assert on["fsk4_st"]["n_symbols"] == len(on["fsk4"]) > 0
        # the clock's symbols are the restatement of the discriminator stream that was read back, from its start on
        want, wslips = M.clock_recovery_mm(on["clock_fm"][f_clock:], on["omega"], taps=bank, unit_gain_input=False)
        print("attached before block %d: %d inputs, %d symbols (restatement %d), slips %d (%d)"
              % (at, len(on["clock_fm"]) - f_clock, on["clock_n"][0], len(want), on["clock_n"][1], wslips))
        assert on["clock_n"][0] == len(want) > 100
        _same_bits(on["clock"], want, ("restatement", at))
        assert on["clock_n"][1] == wslips
