"""The SmartNet / EDACS symbol clock on the GPU (rcf_chan_clock_mm; moto_control_demod.py:113, edacs_control_demod.py:85):
clock_recovery_mm_ff behind a channel's discriminator.  Its soft symbols are, bit for bit, the restatement
(tests/mm_ref.py) of the same channel's chan_read_fm(cid, 5.0) -- on every channel kind, however the stream is cut and
however many channels and front-ends share its launch -- and its bits are the bits that were sent."""
import ctypes

import numpy as np
import pytest

import mm_ref as M
from oracle import grspec as G
from rcf import control, p25, synth

pytestmark = pytest.mark.gpu

FS = 2.4e6
DEV = 1200.0


@pytest.fixture(scope="module")
def bank(gpu_required):
    return gpu_required.design_mmse_interpolator()


def _same_bits(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    np.testing.assert_array_equal(np.ascontiguousarray(got, dtype=np.float32).view(np.uint32),
                                  np.ascontiguousarray(want, dtype=np.float32).view(np.uint32), err_msg=str(what))


def _push_blocks(fe, x, blk):
    for a in range(0, len(x), blk):
        fe.push(x[a:a + blk])


def _carrier(rng, rate, n_samples, off, fs=FS):
    """(a 2-FSK carrier of n_samples at `off`, the bits it carries)"""
    sent = rng.integers(0, 2, int(np.ceil(n_samples * rate / fs)) + 2)
    return M.fsk2_carrier(sent, rate, fs, off, DEV, rng)[:n_samples], sent


def _check_clock(fe, cid, omega, T, what="", fm_from=0, fm=None, **kw):
    """the channel's soft symbols against the restatement of its own discriminator stream from output fm_from on"""
    sym = fe.chan_read_clock(cid)
    n, slips = fe.chan_clock_produced(cid)
    if fm is None:
        fm = fe.chan_read_fm(cid, kw.get("gain", 5.0))
    want, wslips = M.clock_recovery_mm(fm[fm_from:], omega, taps=T, unit_gain_input=False, **{k: v for k, v in kw.items() if k != "gain"})
    print("%s: %d inputs, %d symbols (restatement %d), slips %d (%d)" % (what, len(fm) - fm_from, n, len(want), slips, wslips))
    assert n == len(want), (what, n, len(want))
    _same_bits(sym, want, what)
    assert slips == wslips, (what, slips, wslips)
    return sym, slips, fm


@pytest.mark.parametrize("system", ["smartnet", "edacs"])
def test_soft_symbols_are_the_restatement_and_the_bits_are_the_sent_bits(gpu_required, bank, system):
    nat = gpu_required
    rate, n_bits, setup = {"smartnet": (3600.0, 1200, control.smartnet_clock), "edacs": (9600.0, 3800, control.edacs_clock)}[system]
    rng = np.random.default_rng(int(rate))
    sent = rng.integers(0, 2, n_bits)
    off = 150000.0
    x = M.fsk2_carrier(sent, rate, FS, off, DEV, rng)
    with nat.Frontend(FS, device=0, block_capacity=48000) as fe:
        c = fe.chan_open(12500, off)
        setup(fe, c)
        _push_blocks(fe, x, 48000)
        sym, slips, fm = _check_clock(fe, c, 25000 / rate, bank, system)
    assert len(fm) == -(-len(x) // 96)                        # outputs at inputs 0, 96, 192, ...
    assert slips == 0
    assert abs(len(sym) - n_bits) <= 4
    o, errs = M.align_bits(sym >= 0, sent, skip=100)
    print("%s: alignment offset %d, %d bit errors after the first 100 symbols" % (system, o, errs))
    assert errs == 0


def test_symbols_do_not_depend_on_the_cuts(gpu_required, bank):
    nat = gpu_required
    rate = 3600.0
    rng = np.random.default_rng(77)
    sent = rng.integers(0, 2, 1080)
    x = M.fsk2_carrier(sent, rate, FS, -200000.0, DEV, rng)
    # ~100 pieces: random ones, a run of pieces shorter than one channel sample, and two runs of pieces of exactly one
    # channel sample (96 inputs) -- blocks that end 0, 1, 2, ... samples after a symbol's window was completed, so that
    # the next symbol's window straddles one to seven block boundaries
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 45)}
    cuts |= {96 * 1000 + 17 * k for k in range(1, 12)}
    cuts |= {96 * (2500 + k) + 5 for k in range(22)} | {96 * (6000 + k) for k in range(22)}
    cuts = sorted(cuts)
    assert 95 <= len(cuts) <= 110 and sum(b - a < 96 * 7 for a, b in zip(cuts[:-1], cuts[1:])) > 40

    def run(pieces):
        with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
            c = fe.chan_open(12500, -200000.0)
            control.smartnet_clock(fe, c)
            for a, b in zip(pieces[:-1], pieces[1:]):
                fe.push(x[a:b])
            return fe.chan_read_clock(c), fe.chan_clock_produced(c), fe.chan_read_fm(c, 5.0)

    s1, n1, fm1 = run([0, len(x)])
    s2, n2, fm2 = run(cuts)
    assert fm1.tobytes() == fm2.tobytes()
    assert n1 == n2 and n1[0] == len(s1) and n1[1] == 0
    _same_bits(s2, s1, "cuts")
    want, _ = M.clock_recovery_mm(fm1, 25000 / rate, taps=bank, unit_gain_input=False)
    _same_bits(s1, want, "restatement")
    assert M.align_bits(s1 >= 0, sent, skip=100)[1] == 0


def test_chained_channel_and_discriminator_only_filterbank_tap(gpu_required, bank):
    nat = gpu_required
    rng = np.random.default_rng(31)
    sent = rng.integers(0, 2, 600)
    # a chained pre-filter channel (the P25 demods' 69-tap filter: any chained channel), both it and its source clocked
    x = M.fsk2_carrier(sent, 3600.0, FS, 300000.0, DEV, rng)
    with nat.Frontend(FS, device=0, block_capacity=48000) as fe:
        c1 = fe.chan_open(12500, 300000.0)
        c2 = fe.chan_open_taps(c1, 1, p25.prefilter_taps(12500), 0.0)
        control.smartnet_clock(fe, c2)
        control.edacs_clock(fe, c1)
        _push_blocks(fe, x, 48000)
        s2, slips, _ = _check_clock(fe, c2, 25000 / 3600.0, bank, "chained")
        _check_clock(fe, c1, 25000 / 9600.0, bank, "its source")
    assert slips == 0 and M.align_bits(s2 >= 0, sent, skip=100)[1] == 0
    # a tap of a 400-bin bank at 5 Msps that exposes its discriminator only
    fs = 5e6
    D, taps = G.channel_params(fs, 12500)
    sent = rng.integers(0, 2, 1300)
    x = M.fsk2_carrier(sent, 9600.0, fs, 7 * fs / 400, DEV, rng)
    with nat.Frontend(fs, 0.0, device=0, block_capacity=D * 1000, hist_capacity=1 << 14, out_capacity=1 << 12) as fe:
        fe.pfb_open(2 * D, D, taps)
        tap = fe.pfb_tap_open(7, gr_phase=True)
        fe.chan_set_fm_only(tap, True)
        control.edacs_clock(fe, tap, receive_rate=fs / D)
        _push_blocks(fe, x, D * 1000)
        st, slips, fm = _check_clock(fe, tap, 25000 / 9600.0, bank, "fm-only tap")
    assert abs(len(fm) - len(x) / D) <= 1 and slips == 0
    assert M.align_bits(st >= 0, sent, skip=100)[1] == 0


def test_130_channels_three_waves_one_launch_per_block(gpu_required, bank):
    nat = gpu_required
    blk, K = 24000, 6
    rng = np.random.default_rng(130)
    offs = [-1.1e6 + 16900.0 * k for k in range(130)]
    x = (0.05 * synth.awgn(rng, blk * K) + _carrier(rng, 3600.0, blk * K, offs[5])[0]
         + _carrier(rng, 9600.0, blk * K, offs[70])[0]).astype(np.complex64)
    omega_of = lambda k: 25000 / (3600.0 if k % 2 else 9600.0)       # noqa: E731
    late = lambda k: k % 3 == 1                                      # noqa: E731
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [fe.chan_open(12500, f) for f in offs]
        fe.timing_enable(True, classes=[nat.T_CLOCK])
        for k, c in enumerate(cids):
            if not late(k):
                fe.chan_clock_mm(c, omega_of(k))
        _push_blocks(fe, x[:3 * blk], blk)
        f_late = fe.chan_produced(cids[0])
        for k, c in enumerate(cids):
            if late(k):
                fe.chan_clock_mm(c, omega_of(k))
        _push_blocks(fe, x[3 * blk:], blk)
        assert fe.timing_read(nat.T_CLOCK)[1] == K                   # one launch per block carries all 130
        assert f_late == 3 * blk // 96
        slips = 0
        for k, c in enumerate(cids):
            slips += _check_clock(fe, c, omega_of(k), bank, k, fm_from=f_late if late(k) else 0)[1]
    assert slips == 0


def test_two_front_ends_in_a_group_share_the_launch(gpu_required, bank):
    nat = gpu_required
    blk, K = 48000, 5
    rng = np.random.default_rng(2)
    offs = [(-250000.0, 410000.0), (90000.0, -610000.0)]
    rates = [(3600.0, 9600.0), (9600.0, 3600.0)]
    parts = [[_carrier(rng, rates[m][j], blk * K, offs[m][j]) for j in range(2)] for m in range(2)]
    xs = [(parts[m][0][0] + parts[m][1][0]).astype(np.complex64) for m in range(2)]
    fes = [nat.Frontend(FS, device=0, block_capacity=blk) for _ in range(2)]
    try:
        ids = [[fe.chan_open(12500, f) for f in offs[m]] for m, fe in enumerate(fes)]
        for m, fe in enumerate(fes):
            for j, c in enumerate(ids[m]):
                fe.chan_clock_mm(c, 25000 / rates[m][j])
        fes[0].timing_enable(True, classes=[nat.T_CLOCK])
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * blk:(b + 1) * blk] for xm in xs])
            g.sync()
            assert fes[0].timing_read(nat.T_CLOCK)[1] == K           # one launch per group block for both members
            for m, fe in enumerate(fes):
                for j, c in enumerate(ids[m]):
                    sym, slips, _ = _check_clock(fe, c, 25000 / rates[m][j], bank, ("group", m, j))
                    assert slips == 0
                    assert M.align_bits(sym >= 0, parts[m][j][1], skip=100)[1] == 0
    finally:
        for fe in fes:
            fe.close()


def _read_device(ptr, n_floats):
    """copy device memory to the host with the HIP runtime librcf itself loaded"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(n_floats, dtype=np.float32)
    assert hip.hipMemcpy(out.ctypes.data, ptr, n_floats * 4, 2) == 0      # hipMemcpyDeviceToHost
    return out


def test_lifecycle_restart_retune_off_close_and_a_callers_bank(gpu_required, bank):
    nat = gpu_required
    blk = 48000
    rng = np.random.default_rng(4)
    sent = rng.integers(0, 2, 1300)
    off = 123000.0
    x = (M.fsk2_carrier(sent, 3600.0, FS, off, DEV, rng) + M.fsk2_carrier(sent, 3600.0, FS, -400000.0, DEV, rng)).astype(np.complex64)
    om = 25000 / 3600.0
    lin = M.linear_bank()

    def code(fn, *a):
        with pytest.raises(nat.RcfError) as e:
            fn(*a)
        return e.value.code

    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c1 = fe.chan_open(12500, off)
        c3 = fe.chan_open(12500, -400000.0)
        control.smartnet_clock(fe, c1)
        control.smartnet_clock(fe, c3)
        _push_blocks(fe, x[:3 * blk], blk)
        first = fe.chan_read_clock(c1)
        assert len(first) > 150
        # enabled again mid-stream: zero history from this output on, symbol 0 is the first of the call
        f1 = fe.chan_produced(c1)
        control.smartnet_clock(fe, c1)
        assert fe.chan_clock_produced(c1) == (0, 0)
        _push_blocks(fe, x[3 * blk:6 * blk], blk)
        # the zero-copy ring holds the same symbols
        fe.sync()
        ptr, cap = fe.chan_clock_ring(c1)
        assert cap == 1 << 16
        n1 = fe.chan_clock_produced(c1)[0]
        ring = _read_device(ptr, n1)
        a = fe.chan_read_clock(c1)
        _same_bits(ring, a, "ring")
        # a retune keeps it
        fe.chan_set_offset(c1, off + 40.0)
        _push_blocks(fe, x[6 * blk:9 * blk], blk)
        b = fe.chan_read_clock(c1)
        fm1 = fe.chan_read_fm(c1, 5.0)
        want, _ = M.clock_recovery_mm(fm1[f1:], om, taps=bank, unit_gain_input=False)
        _same_bits(np.concatenate([a, b]), want, "restart + retune")
        assert len(b) > 150 and fe.chan_clock_produced(c1) == (len(want), 0)
        w0, _ = M.clock_recovery_mm(fm1[:3 * blk // 96], om, taps=bank, unit_gain_input=False)
        _same_bits(first, w0, "before the restart")
        # off: the reads are refused; off twice: nothing to do
        fe.chan_clock_mm(c1, None)
        fe.chan_clock_mm(c1, None)
        assert code(fe.chan_read_clock, c1) == nat.RCF_ESTATE
        assert code(fe.chan_clock_produced, c1) == nat.RCF_ESTATE
        assert code(fe.chan_clock_ring, c1) == nat.RCF_ESTATE
        # closed while enabled, another channel opened: its stream is its own; a caller's bank beside the default one
        fe.chan_close(c3)
        assert code(fe.chan_read_clock, c3) == nat.RCF_ENOCHAN
        c4 = fe.chan_open(12500, -400000.0)
        fe.chan_clock_mm(c4, om, interp_taps=lin)
        f1b = fe.chan_produced(c1)
        control.smartnet_clock(fe, c1)
        _push_blocks(fe, x[9 * blk:14 * blk], blk)
        s4, slips4, fm4 = _check_clock(fe, c4, om, lin, "linear bank")
        s1, _, _ = _check_clock(fe, c1, om, bank, "default bank beside it")      # (its unread fm starts at f1b)
    assert slips4 == 0 and len(fm4) == 5 * blk // 96
    wd, _ = M.clock_recovery_mm(fm4, om, taps=bank, unit_gain_input=False)
    assert s4.tobytes() != wd[: len(s4)].tobytes()                 # the two banks do differ
    assert len(s1) > 250 and f1b == 9 * blk // 96


def test_default_bank_beside_a_callers_bank_in_one_wave(gpu_required, bank):
    nat = gpu_required
    blk = 48000
    rng = np.random.default_rng(9)
    sent = rng.integers(0, 2, 500)
    x = M.fsk2_carrier(sent, 3600.0, FS, 50000.0, DEV, rng)[: 6 * blk]
    lin = M.linear_bank()
    om = 25000 / 3600.0
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [fe.chan_open(12500, 50000.0 + 3000.0 * k) for k in range(5)]
        for k, c in enumerate(cids):
            fe.chan_clock_mm(c, om, interp_taps=lin if k % 2 else None)
        _push_blocks(fe, x, blk)
        for k, c in enumerate(cids):
            _check_clock(fe, c, om, lin if k % 2 else bank, ("bank", k))


def test_refusals(gpu_required):
    nat = gpu_required

    def code(fn, *a, **kw):
        with pytest.raises(nat.RcfError) as e:
            fn(*a, **kw)
        return e.value.code

    nan, inf = float("nan"), float("inf")
    with nat.Frontend(FS, device=0, block_capacity=48000) as fe:
        c = fe.chan_open(12500, 0.0)
        for name in ("omega", "gain_omega", "mu", "gain_mu", "omega_relative_limit", "gain"):
            for bad in (nan, inf, -inf):
                kw = {"omega": 6.9, name: bad}
                assert code(fe.chan_clock_mm, c, **kw) == nat.RCF_EINVAL, (name, bad)
        assert code(fe.chan_clock_mm, c, 2.0) == nat.RCF_EINVAL                 # 2.0 * (1 - 0.005) < 2
        assert code(fe.chan_clock_mm, c, 1.0) == nat.RCF_EINVAL
        assert code(fe.chan_clock_mm, c, 2.5, omega_relative_limit=0.3) == nat.RCF_EINVAL
        assert code(fe.chan_clock_mm, c, 4097.0) == nat.RCF_EINVAL
        assert code(fe.chan_clock_mm, c, 6.9, mu=1.5) == nat.RCF_EINVAL          # mu selects a row of the bank
        assert code(fe.chan_clock_mm, c, 6.9, mu=-0.1) == nat.RCF_EINVAL
        assert code(fe.chan_clock_mm, 999, 6.9) == nat.RCF_ENOCHAN
        assert code(fe.chan_read_clock, 999) == nat.RCF_ENOCHAN
        assert code(fe.chan_read_clock, c) == nat.RCF_ESTATE                     # no clock yet
        assert code(fe.chan_clock_produced, c) == nat.RCF_ESTATE
        assert code(fe.chan_clock_ring, c) == nat.RCF_ESTATE
        fe.chan_clock_mm(c, 2.02)                                                # 2.02 * 0.995 >= 2
        fe.chan_clock_mm(c, 4096.0)
        fe.chan_clock_mm(c, None)
        with pytest.raises(ValueError):
            fe.chan_clock_mm(c, 6.9, interp_taps=np.zeros((128, 8), dtype=np.float32))
    # a ring that cannot hold the window
    with nat.Frontend(FS, device=0, block_capacity=48000, out_capacity=8) as fe:
        c = fe.chan_open(12500, 0.0)
        assert code(fe.chan_clock_mm, c, 6.9) == nat.RCF_ECAP
    # ... and a block that yields more than the ring holds beside the seven samples of look-back: refused, nothing queued
    rng = np.random.default_rng(1)
    x = (0.1 * synth.awgn(rng, 96 * 3100)).astype(np.complex64)
    with nat.Frontend(FS, device=0, block_capacity=96 * 1100, out_capacity=1 << 10) as fe:
        c, plain = fe.chan_open(12500, 0.0), None
        fe.chan_clock_mm(c, 6.9)
        fe.push(x[:96 * 1000])                                                   # 1000 + 7 <= 1024
        T = nat.design_mmse_interpolator()
        s0, _, fm0 = _check_clock(fe, c, 6.9, T, "first block")
        assert code(fe.push, x[96 * 1000:96 * 2020]) == nat.RCF_ECAP             # 1020 + 7 > 1024
        assert fe.chan_produced(c) == 1000
        fe.push(x[96 * 1000:96 * 2017])                                          # 1017 + 7 == 1024
        s1 = fe.chan_read_clock(c)
        fm1 = fe.chan_read_fm(c, 5.0)
        want, _ = M.clock_recovery_mm(np.concatenate([fm0, fm1]), 6.9, taps=T, unit_gain_input=False)
        _same_bits(np.concatenate([s0, s1]), want, "after the refusal")
        fe.chan_clock_mm(c, None)
        fe.push(x[96 * 2017:96 * 3037])                                          # without the clock 1020 + 1 fit
        assert fe.chan_produced(c) == 3037 and plain is None


def test_bounded_on_hostile_input(gpu_required, bank):
    """2000 channel samples of wideband noise at amplitude 1e6: the call returns (the kernel's loop is over the block's
    samples), at most one symbol per sample, the guards fire where the loop gains let them, and symbols, count and slips
    are the restatement's (which has the two guards)"""
    nat = gpu_required
    rng = np.random.default_rng(666)
    x = (1e6 * synth.awgn(rng, 96 * 2000)).astype(np.complex64)
    shapes = [dict(omega=25000 / 9600.0),                                        # the EDACS loop as it is
              dict(omega=2.6, gain_mu=1.0),                                      # steps < 1
              dict(omega=2.6, gain_omega=3e38),                                  # omega overflows: the loop starts over
              dict(omega=6.9, gain_omega=3e38, gain_mu=40.0),                    # both, and steps of hundreds of inputs
              dict(omega=2.6, gain_mu=3e38)]                                     # mu overflows, or a step saturates: past any block
    with nat.Frontend(FS, device=0, block_capacity=96 * 500) as fe:
        cids = [fe.chan_open(12500, 100000.0 * k - 200000.0) for k in range(len(shapes))]
        for c, kw in zip(cids, shapes):
            fe.chan_clock_mm(c, gain=5.0, **kw)
        _push_blocks(fe, x, 96 * 500)
        for k, (c, kw) in enumerate(zip(cids, shapes)):
            kw = dict(kw)
            om = kw.pop("omega")
            sym, slips, fm = _check_clock(fe, c, om, bank, ("hostile", k), **kw)
            assert len(fm) == 2000 and len(sym) <= 2000
            assert np.isfinite(sym).all()
            if k in (1, 2, 3):
                assert slips > 0, k


def test_mixed_channel_rates_in_one_wave(gpu_required, bank):
    """six clocked channels at 12.5, 25 and 50 kS/s in one wave: n_k = 250, 500 and 1000 per block, so the lanes leave the
    chunk loop at different trips, each with its own omega; one is enabled two blocks late"""
    nat = gpu_required
    blk, K = 48000, 6
    rng = np.random.default_rng(6)
    # (chan_open's channel rate, baud, offset): omega = 2 * channel rate / baud = 3.47, 6.94, 2.60, 5.21, 13.9, 3.47
    shapes = [(6250, 3600.0, -700000.0), (12500, 3600.0, -400000.0), (12500, 9600.0, -100000.0),
              (25000, 9600.0, 200000.0), (25000, 3600.0, 500000.0), (6250, 3600.0, 800000.0)]
    sent = {k: _carrier(rng, shapes[k][1], blk * K, shapes[k][2]) for k in (1, 3)}
    x = (0.05 * synth.awgn(rng, blk * K) + sent[1][0] + sent[3][0]).astype(np.complex64)
    omega = [2 * cr / baud for cr, baud, _ in shapes]
    late = 4
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [fe.chan_open(cr, off) for cr, _, off in shapes]
        fe.timing_enable(True, classes=[nat.T_CLOCK])
        for k, c in enumerate(cids):
            if k != late:
                fe.chan_clock_mm(c, omega[k])
        _push_blocks(fe, x[:2 * blk], blk)
        f_late = fe.chan_produced(cids[late])
        fe.chan_clock_mm(cids[late], omega[late])
        _push_blocks(fe, x[2 * blk:], blk)
        assert fe.timing_read(nat.T_CLOCK)[1] == K                   # one launch per block carries all six
        assert f_late == 2 * blk // 48
        for k, c in enumerate(cids):
            sym, slips, fm = _check_clock(fe, c, omega[k], bank, ("mixed rates", k), fm_from=f_late if k == late else 0)
            assert len(fm) == K * blk * 2 * shapes[k][0] // int(FS)
            if k in sent:
                assert slips == 0 and M.align_bits(sym >= 0, sent[k][1], skip=100)[1] == 0


def test_symbol_ring_wraps(gpu_required, bank):
    """out_capacity 1024 and more than 2500 symbols: the soft-symbol ring (and the discriminator ring it reads) wraps at
    least twice; read after every push, the concatenation is the restatement of the concatenated discriminator stream"""
    nat = gpu_required
    blk, K = 96 * 1000, 7                                            # 1000 channel samples a block: 1000 + 7 <= 1024
    omega = 25000 / 9600.0
    rng = np.random.default_rng(1024)
    car, sent = _carrier(rng, 9600.0, blk * K, 250000.0)
    x = (0.05 * synth.awgn(rng, blk * K) + car).astype(np.complex64)
    syms, fms = [], []
    with nat.Frontend(FS, device=0, block_capacity=96 * 1100, out_capacity=1 << 10) as fe:
        c = fe.chan_open(12500, 250000.0)
        fe.chan_clock_mm(c, omega)
        assert fe.chan_clock_ring(c)[1] == 1024
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk])
            fms.append(fe.chan_read_fm(c, 5.0))
            syms.append(fe.chan_read_clock(c))
        n, slips = fe.chan_clock_produced(c)
    fm, sym = np.concatenate(fms), np.concatenate(syms)
    want, wslips = M.clock_recovery_mm(fm, omega, taps=bank, unit_gain_input=False)
    print("wrapped ring: %d inputs, %d symbols (restatement %d), slips %d (%d)" % (len(fm), n, len(want), slips, wslips))
    assert len(fm) == K * 1000 and len(want) > 2500 and all(0 < len(s) < 1024 for s in syms)
    assert n == len(want) == len(sym)
    _same_bits(sym, want, "wrapped ring")
    assert slips == wslips == 0
    assert M.align_bits(sym >= 0, sent, skip=100)[1] == 0
