"""The P25 CQPSK front half on the GPU (p25_control_demod.py:136-161; rcf_chan_agc): a channel, the chained 69-tap
pre-filter, analog.feedforward_agc_cc(1024, 1.0).  The AGC is bit-identical to the restatement (tests/agc_ref.py) of
the same channel's IQ, on every channel kind, however the stream is cut and however many channels and front-ends share
its launch."""
import ctypes
import numpy as np
import pytest

import agc_ref as A
from oracle import grspec as G
from rcf import p25, synth

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.complex64).view(np.uint32)


def _assert_same_bits(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(what))


def _fades(x, fs, period_s=0.04):
    """20 dB amplitude steps: the stream alternates between full level and a tenth of it every period_s"""
    k = (np.arange(len(x)) // int(fs * period_s)) % 2
    return (x * np.where(k == 0, 1.0, 0.1).astype(np.float32)).astype(np.complex64)


def _push_blocks(fe, x, blk):
    for a in range(0, len(x), blk):
        fe.push(x[a:a + blk])


@pytest.mark.parametrize("fades,N", [(False, 1024), (True, 1024), (False, 1), (True, 7), (True, 4096)])
def test_cqpsk_front_half_is_the_restatement_of_its_channel_bit_for_bit(gpu_required, fades, N):
    nat = gpu_required
    x, meta = synth.cfg1(seconds=0.5)
    fs = meta["fs"]
    if fades:
        x = _fades(x, fs)
    with nat.Frontend(fs, meta["center_freq"], device=0, block_capacity=48000) as fe:
        c1 = fe.chan_open(12500, meta["offset"])
        c2 = p25.cqpsk_front_half(fe, c1, 12500) if N == 1024 else fe.chan_open_taps(c1, 1, p25.prefilter_taps(12500), 0.0)
        if N != 1024:
            fe.chan_agc(c2, N, 1.0)
        _push_blocks(fe, x, 48000)
        agc = fe.chan_read_agc(c2)
        iq = fe.chan_read_iq(c2)
    assert len(agc) == len(iq) == len(x) // 96
    _assert_same_bits(agc, A.feedforward_agc(iq, N, 1.0), (fades, N))
    # ... and against the oracle chain: xlating_fir_ccc twice (channel, pre-filter), then the restatement
    D, taps = G.channel_params(fs, 12500)
    y1 = G.xlating_fir_ccc(x, D, taps, meta["offset"], fs)
    y2 = G.xlating_fir_ccc(y1, 1, G.low_pass_2(1.0, 25000, 6250, 500, 30, G.WIN_BLACKMAN), 0.0, 25000.0)
    want = A.feedforward_agc(y2[: len(agc)], N, 1.0)
    err = float(np.sqrt(np.mean(np.abs(agc.astype(np.complex128) - want) ** 2)))
    assert err <= 1e-5, (fades, N, err)
    assert float(np.abs(agc).max()) > 0.5                     # a real signal, normalised to about 1


@pytest.mark.parametrize("N", [1024, 4096])
def test_agc_bits_do_not_depend_on_the_cuts(gpu_required, N):
    nat = gpu_required
    x, meta = synth.cfg1(seconds=0.3, seed=7)
    x = _fades(x, meta["fs"], 0.03)
    rng = np.random.default_rng(N)
    # random pieces, many of them shorter than N - 1 outputs (96 input samples per output)
    cuts = sorted({0, len(x)} | {int(v) for v in rng.integers(1, len(x), 60)} | {96 * 5 * k + 3 for k in range(1, 40)})

    def run(pieces):
        with nat.Frontend(meta["fs"], device=0, block_capacity=len(x)) as fe:
            c1 = fe.chan_open(12500, meta["offset"])
            c2 = p25.cqpsk_front_half(fe, c1, 12500, nsamples=N)
            for a, b in zip(pieces[:-1], pieces[1:]):
                fe.push(x[a:b])
            return fe.chan_read_agc(c2), fe.chan_read_iq(c2)

    agc1, iq1 = run([0, len(x)])
    agc2, iq2 = run(cuts)
    _assert_same_bits(iq2, iq1, "iq")
    _assert_same_bits(agc2, agc1, "agc")
    _assert_same_bits(agc1, A.feedforward_agc(iq1, N, 1.0), "restatement")


def _many_channels(nat, x, fs, n_chans, agc_of, blocks_plain, blocks_agc, blk, timing=False):
    """n_chans direct channels; blocks_plain blocks without AGCs, then AGCs (agc_of(k) -> (N, R) or None) and
    blocks_agc blocks more.  Returns per channel (agc, iq, first AGC output index) and the T_DISC launch counts."""
    with nat.Frontend(fs, device=0, block_capacity=blk) as fe:
        cids = [fe.chan_open(12500, -1.1e6 + 4300.0 * k) for k in range(n_chans)]
        if timing:
            fe.timing_enable(True, classes=[nat.T_DISC])
        at = 0
        for _ in range(blocks_plain):
            fe.push(x[at:at + blk])
            at += blk
        n_plain = fe.timing_read(nat.T_DISC)[1] if timing else 0
        from_ = fe.chan_produced(cids[0])
        for k, c in enumerate(cids):
            if agc_of(k):
                fe.chan_agc(c, *agc_of(k))
        for _ in range(blocks_agc):
            fe.push(x[at:at + blk])
            at += blk
        n_agc = fe.timing_read(nat.T_DISC)[1] if timing else 0
        out = []
        for k, c in enumerate(cids):
            out.append((fe.chan_read_agc(c) if agc_of(k) else None, fe.chan_read_iq(c), from_))
    return out, n_plain, n_agc


def test_512_agc_channels_one_launch_per_block_same_bits_as_alone(gpu_required):
    nat = gpu_required
    fs, blk, K = 2.4e6, 48000, 4
    rng = np.random.default_rng(512)
    x = (synth.awgn(rng, blk * 2 * K) * np.repeat(rng.uniform(0.05, 2.0, 2 * K * 8), blk // 8)).astype(np.complex64)
    shapes = [(1, 1.0), (7, 0.5), (100, 2.0), (1024, 1.0), (4096, -1.5)]
    agc_of = lambda k: shapes[k % len(shapes)]               # noqa: E731
    many, n_plain, n_agc = _many_channels(nat, x, fs, 512, agc_of, K, K, blk, timing=True)
    assert n_plain > 0 and n_agc - n_plain == K, (n_plain, n_agc)      # T_DISC: exactly one launch more per block
    for k, (agc, iq, f) in enumerate(many):
        N, R = agc_of(k)
        assert f > 0 and len(agc) == len(iq) - f
        _assert_same_bits(agc, A.feedforward_agc(iq[f:], N, R), k)
    # each channel alone in its launch: the same bits (the IQ is the same: the channel set and the blocks are)
    for k in (3, 4, 5):
        alone, _, _ = _many_channels(nat, x, fs, 512, lambda j, k=k: agc_of(j) if j == k else None, K, K, blk)
        _assert_same_bits(alone[k][1], many[k][1], ("iq", k))
        _assert_same_bits(alone[k][0], many[k][0], ("agc", k))


def _member_setup(fe, m, agc=True):
    c1 = fe.chan_open(12500, -62500.0 + 25000.0 * m)
    c2 = p25.cqpsk_front_half(fe, c1, 12500, nsamples=(1024, 64, 2048)[m]) if agc else \
        fe.chan_open_taps(c1, 1, p25.prefilter_taps(12500), 0.0)
    c3 = fe.chan_open(12500, 300000.0 - 12500.0 * m)
    if agc:
        fe.chan_agc(c3, 200 + m, 0.75)
    return [c1, c2, c3]


def test_group_push_same_bits_as_members_alone_and_one_launch_per_block(gpu_required):
    nat = gpu_required
    fs, blk, K = 2.4e6, 48000, 8
    xs = [synth.cfg1(seconds=blk * K / fs, seed=40 + m)[0] for m in range(3)]
    for m in range(3):
        xs[m] = _fades(xs[m], fs, 0.025 + 0.01 * m)

    def grouped(agc):
        fes = [nat.Frontend(fs, device=0, block_capacity=blk) for _ in range(3)]
        try:
            ids = [_member_setup(fe, m, agc) for m, fe in enumerate(fes)]
            fes[0].timing_enable(True, classes=[nat.T_DISC])
            with nat.Group(fes) as g:
                for b in range(K):
                    g.push([xm[b * blk:(b + 1) * blk] for xm in xs])
                g.sync()
                n = fes[0].timing_read(nat.T_DISC)[1]
                out = [[(fe.chan_read_agc(c) if agc and c != ids[m][0] else None, fe.chan_read_iq(c)) for c in ids[m]]
                       for m, fe in enumerate(fes)]
                rows = g.read_many([(m, ids[m][1]) for m in range(3)], what="agc") if agc else None
        finally:
            for fe in fes:
                fe.close()
        return out, n, rows

    out, n_agc, rows = grouped(True)
    _, n_plain, _ = grouped(False)
    assert n_agc - n_plain == K, (n_plain, n_agc)            # the group's AGCs: one launch per group block
    for m in range(3):
        with nat.Frontend(fs, device=0, block_capacity=blk) as fe:
            ids = _member_setup(fe, m)
            _push_blocks(fe, xs[m], blk)
            alone = [(fe.chan_read_agc(c) if c != ids[0] else None, fe.chan_read_iq(c)) for c in ids]
        for j in (1, 2):
            _assert_same_bits(out[m][j][1], alone[j][1], ("iq", m, j))
            _assert_same_bits(out[m][j][0], alone[j][0], ("agc", m, j))
        N = (1024, 64, 2048)[m]
        _assert_same_bits(out[m][1][0], A.feedforward_agc(out[m][1][1], N, 1.0), ("restatement", m))
        _assert_same_bits(out[m][2][0], A.feedforward_agc(out[m][2][1], 200 + m, 0.75), ("restatement", m))
        assert len(rows[m]) == 0                              # the read above took everything
    # group_read_many("agc") serves the same stream as chan_read_agc
    fes = [nat.Frontend(fs, device=0, block_capacity=blk) for _ in range(3)]
    try:
        ids = [_member_setup(fe, m) for m, fe in enumerate(fes)]
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * blk:(b + 1) * blk] for xm in xs])
            rows = g.read_many([(m, ids[m][1]) for m in range(3)], what="agc", cap_each=1 << 13)
        for m in range(3):
            _assert_same_bits(rows[m], out[m][1][0], ("group read_many", m))
    finally:
        for fe in fes:
            fe.close()


def _stage2(nat, x, lag, agc_at):
    fs, nb, blk = 20e6, 256, 256 * 16 * 40
    bw = fs / nb
    proto = G.low_pass_2(1.0, fs, bw * 0.4, bw * 0.2, 60.0, G.WIN_BLACKMAN_HARRIS)
    with nat.Frontend(fs, 0.0, device=0, block_capacity=blk, hist_capacity=1 << 14, out_capacity=1 << 13) as fe:
        fe.set_stage2_lag(lag)
        fe.pfb_open(nb, nb, proto)
        ids = [fe.pfb_chan_open((5 + 17 * i) % nb, 12500, 12500.0 * ((i % 5) - 2)) for i in range(7)]
        from_ = None
        for b in range(len(x) // blk):
            if b == agc_at:
                from_ = fe.chan_produced(ids[2])
                fe.chan_agc(ids[2], 1024, 1.0)
            fe.push(x[b * blk:(b + 1) * blk])
        return fe.chan_read_agc(ids[2]), fe.chan_read_iq(ids[2]), fe.chan_read_fm(ids[3], 5.0), from_


def test_stage2_channel_with_agc_under_the_stage2_lag(gpu_required):
    nat = gpu_required
    blk = 256 * 16 * 40
    x, _ = synth.cfg2(n=8 * blk, seed=2300)
    for agc_at in (0, 3):                                    # from the start, and switched on while a launch lags
        a_on = _stage2(nat, x, True, agc_at)
        a_off = _stage2(nat, x, False, agc_at)
        agc, iq, fm, f = a_on
        assert len(agc) > 500 and len(agc) == len(iq) - f
        _assert_same_bits(agc, A.feedforward_agc(iq[f:], 1024, 1.0), agc_at)
        _assert_same_bits(agc, a_off[0], ("lag", agc_at))
        _assert_same_bits(iq, a_off[1], ("lag iq", agc_at))
        assert fm.tobytes() == a_off[2].tobytes()


def test_agc_on_a_1600_bin_bank_tap(gpu_required):
    nat = gpu_required
    fs = 20e6
    D, taps = G.channel_params(fs, 12500)
    rng = np.random.default_rng(1600)
    n = D * 3000
    f_k = 21 * fs / 1600 + 1500.0
    x = (0.02 * synth.awgn(rng, n) + synth.nbfm_carrier(n, fs, f_k, 800.0, 2000.0, 0.5)).astype(np.complex64)
    x = _fades(x, fs, 0.02)
    with nat.Frontend(fs, 0.0, device=0, block_capacity=D * 1000, hist_capacity=1 << 15, out_capacity=1 << 13) as fe:
        fe.pfb_open(1600, D, taps)
        tap = fe.pfb_tap_open(21, gr_phase=True)
        other = fe.pfb_tap_open(22, gr_phase=True)
        fe.chan_agc(tap, 1024, 1.0)
        _push_blocks(fe, x, D * 1000)
        agc = fe.chan_read_agc(tap)
        iq = fe.chan_read_iq(tap)
        fe.chan_read_iq(other)
    assert len(agc) == len(iq) == 3000
    _assert_same_bits(agc, A.feedforward_agc(iq, 1024, 1.0))
    assert float(np.abs(agc[1500:]).max()) > 0.5


def _read_device(ptr, nbytes):
    """copy device memory to the host with the HIP runtime librcf itself loaded"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(nbytes // 8, dtype=np.complex64)
    assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0     # hipMemcpyDeviceToHost
    return out


def test_lifecycle_mid_stream_off_on_retune_and_readers(gpu_required):
    nat = gpu_required
    x, meta = synth.cfg1(seconds=0.4, seed=3)
    x = _fades(x, meta["fs"], 0.035)
    blk = 48000
    with nat.Frontend(meta["fs"], device=0, block_capacity=blk) as fe:
        c1 = fe.chan_open(12500, meta["offset"])
        c2 = fe.chan_open_taps(c1, 1, p25.prefilter_taps(12500), 0.0)
        c3 = fe.chan_open(12500, meta["offset"] + 12500.0)
        _push_blocks(fe, x[:3 * blk], blk)
        f2, f3 = fe.chan_produced(c2), fe.chan_produced(c3)
        assert f2 > 0 and f3 > 0
        fe.chan_agc(c2, 1024, 1.0)                           # mid-stream: zero history from here
        fe.chan_agc(c3, 16, 2.0)
        _push_blocks(fe, x[3 * blk:5 * blk], blk)
        # the batched reader and the zero-copy ring serve the same stream
        fe.sync()
        ptr, cap = fe.chan_agc_ring(c2)
        assert cap == 1 << 16
        ring = _read_device(ptr, cap * 8)
        p = fe.chan_produced(c2)
        rows = fe.chan_read_many([c2, c3], what="agc")
        assert len(rows[0]) == p - f2
        np.testing.assert_array_equal(_bits(rows[0]), _bits(ring[np.arange(f2, p) & (cap - 1)]))
        a2 = [rows[0].copy()]
        a3 = [rows[1].copy()]
        # a retune keeps it
        fe.chan_set_offset(c1, meta["offset"] + 100.0)
        _push_blocks(fe, x[5 * blk:6 * blk], blk)
        a2.append(fe.chan_read_agc(c2))
        # off, and on again: a fresh start
        p_off = fe.chan_produced(c2)
        fe.chan_agc(c2, 0, 1.0)
        with pytest.raises(nat.RcfError) as e:
            fe.chan_read_agc(c2)
        assert e.value.code == nat.RCF_ESTATE
        _push_blocks(fe, x[6 * blk:7 * blk], blk)
        f2b = fe.chan_produced(c2)
        fe.chan_agc(c2, 512, 1.0)
        _push_blocks(fe, x[7 * blk:], blk)
        b2 = fe.chan_read_agc(c2)
        plan = fe.chan_read_many_plan([c3], what="agc")
        counts, out = plan()
        a3.append(out[0, :counts[0]].copy())
        iq2 = fe.chan_read_iq(c2)
        iq3 = fe.chan_read_iq(c3)
    assert f2b > p_off
    _assert_same_bits(np.concatenate(a2), A.feedforward_agc(iq2[f2:p_off], 1024, 1.0))
    _assert_same_bits(b2, A.feedforward_agc(iq2[f2b:], 512, 1.0))
    _assert_same_bits(np.concatenate(a3), A.feedforward_agc(iq3[f3:], 16, 2.0))


def test_refusals(gpu_required):
    nat = gpu_required
    lib = nat.lib()

    def code(fn, *a):
        with pytest.raises(nat.RcfError) as e:
            fn(*a)
        return e.value.code

    with nat.Frontend(2.4e6, device=0, block_capacity=48000) as fe:
        c = fe.chan_open(12500, 0.0)
        for N, R in ((-1, 1.0), (4097, 1.0), (1024, float("nan")), (1024, float("inf")), (1024, float("-inf"))):
            assert code(fe.chan_agc, c, N, R) == nat.RCF_EINVAL, (N, R)
        assert code(fe.chan_agc, 999, 1024, 1.0) == nat.RCF_ENOCHAN
        assert code(fe.chan_read_agc, c) == nat.RCF_ESTATE           # no AGC yet
        assert code(fe.chan_agc_ring, c) == nat.RCF_ESTATE
        counts, _ = fe.chan_read_many_plan([c, 999], what="agc")()
        assert counts[0] == nat.RCF_ESTATE and counts[1] == nat.RCF_ENOCHAN
        fe.chan_agc(c, 4096, 1.0)
        fe.chan_agc(c, 0, 1.0)                                # off twice: nothing to do
        fe.chan_agc(c, 0, 1.0)
        fe.chan_close(c)
        assert code(fe.chan_agc, c, 1024, 1.0) == nat.RCF_ENOCHAN   # closed
        assert code(fe.chan_read_agc, c) == nat.RCF_ENOCHAN
        ids = (ctypes.c_int * 1)(c)
        cnt = (ctypes.c_int64 * 1)()
        buf = np.zeros(16, dtype=np.complex64)
        assert lib.rcf_chan_read_many(fe._h, 3, ids, 1, 1.0, buf.ctypes.data_as(ctypes.c_void_p), 16, cnt) == nat.RCF_EINVAL
    # a too small ring: at enable time, and at a block that yields more than the ring holds beside the look-back
    with nat.Frontend(2.4e6, device=0, block_capacity=96 * 4000, out_capacity=1 << 12) as fe:
        c = fe.chan_open(12500, 0.0)
        assert code(fe.chan_agc, c, 4096, 1.0) == nat.RCF_ECAP
        fe.chan_agc(c, 2048, 1.0)
        rng = np.random.default_rng(1)
        x = synth.awgn(rng, 96 * 4000)
        fe.push(x[:96 * 1000])                                # 1000 + 2047 <= 4096
        assert code(fe.push, x[96 * 1000:]) == nat.RCF_ECAP   # 3000 + 2047 > 4096: refused, nothing queued
        assert fe.chan_produced(c) == 1000
        fe.push(x[96 * 1000:96 * 2000])
        agc, iq = fe.chan_read_agc(c), fe.chan_read_iq(c)
        _assert_same_bits(agc, A.feedforward_agc(iq, 2048, 1.0))
    # a discriminator-only tap has no IQ; an AGC keeps the tap from becoming one
    fs = 5e6
    D, taps = G.channel_params(fs, 12500)
    with nat.Frontend(fs, 0.0, device=0, block_capacity=D * 100, hist_capacity=1 << 14, out_capacity=1 << 12) as fe:
        fe.pfb_open(2 * D, D, taps)
        t1 = fe.pfb_tap_open(7, gr_phase=True)
        t2 = fe.pfb_tap_open(8, gr_phase=True)
        fe.chan_set_fm_only(t1, True)
        assert code(fe.chan_agc, t1, 1024, 1.0) == nat.RCF_ESTATE
        fe.chan_agc(t2, 1024, 1.0)
        assert code(fe.chan_set_fm_only, t2, True) == nat.RCF_ESTATE
        fe.chan_agc(t2, 0, 1.0)
        fe.chan_set_fm_only(t2, True)
