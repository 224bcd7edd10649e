"""The P25 CQPSK back half on the GPU (rcf_chan_costas; p25_control_demod.py:150-183): the Gardner / Costas loop behind a
channel's AGC.  include/rcf.h defines the stage (unpinned against op25), tests/gc_ref.py restates it.  Its soft symbols stay
within float32 rounding noise of the restatement run on the same channel's own AGC stream -- the yardstick is the distance
between the restatement's float32 and float64 runs on that input --, they slice to the dibits that were sent, and they are
the same bits however the stream is cut, however many channels and front-ends share the launch and however small the ring.

Beyond the P25 operating point (inputs decided by tests/test_costas_cpu.py): lanes of one wave that end at different
trips of the chunk loop, omega 2.08 .. 16, the window clamp, the guard through non-finite input and through mu <= 1, and
every symbol from 0 on.

Measured on an MI355X, soft-symbol units, GPU against the float32 restatement | yardstick; the new rows from one run of
the finished tests (their print lines).  DESIGN.md 9, row f-7 has the same.
  five cases, symbols 500 .. 1500      rms 1.1e-7 .. 2.3e-7 | 1.1e-3 .. 1.8e-3
  five cases, symbols 0 .. 500         rms 8.2e-8 .. 1.0e-7 | 1.5e-4 .. 4.5e-4, max 4.8e-7 .. 7.2e-7 | 2.3e-3 .. 5.1e-3
  five cases, the first 16 symbols     0 | 0 (the AGC of 1024 has not delivered yet)
  mixed rates, eight lanes, from 0     rms 1.2e-7 .. 2.0e-7 | 1.9e-4 .. 6.9e-3, max 4.8e-7 .. 3.6e-6 | 1.4e-3 .. 4.6e-2
  lanes 0, 63, 64, 129 of 130, from 0  rms 9.4e-8 .. 1.1e-7 | 5.3e-4 .. 2.1e-3; first 16: max 0 .. 2.4e-7 | 7.5e-8 .. 3.7e-7
  window clamp, prefix of 905, 15 hits max 4.8e-7 | 3.9e-2
  NaN / Inf burst, before it           rms 1.0e-7, 1.3e-7 | 1.0e-3, 1.5e-3, max 7.7e-7, 2.6e-6 | 6.6e-3, 7.7e-3
  NaN / Inf burst, 500 symbols after   rms 1.5e-7, 1.5e-7 | 1.1e-3, 1.1e-3; 15 and 19 slips, as the restatement
  gain_mu -40, 18 symbols to the slip  max 0 | 3.6e-7; 211 symbols, 25 slips, as the restatement"""
import numpy as np
import pytest

import gc_ref as R
import mm_ref as M
from oracle import grspec as G
from rcf import p25, synth

pytestmark = pytest.mark.gpu

FS, CR, OFF = R.FS, R.CHANNEL_RATE, R.CHANNEL_OFFSET
BLK = 16 * 1000                                               # 1000 channel samples a block


def _same_bits(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    np.testing.assert_array_equal(np.ascontiguousarray(got, dtype=np.float32).view(np.uint32),
                                  np.ascontiguousarray(want, dtype=np.float32).view(np.uint32), err_msg=str(what))


def _push_blocks(fe, x, blk):
    for a in range(0, len(x), blk):
        fe.push(x[a:a + blk])


def _code(nat, fn, *a, **kw):
    with pytest.raises(nat.RcfError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.fixture(scope="module")
def bank(gpu_required):
    return gpu_required.design_mmse_interpolator()


@pytest.fixture(scope="module")
def runs(gpu_required, bank):
    """per case: the GPU's soft symbols, its AGC stream and state, and the float32 / float64 restatements of that stream"""
    nat = gpu_required
    D, taps = G.channel_params(FS, CR)
    out = {}
    for case in R.CASES:
        baud, cfo, timing = case
        x, sent = R.case_signal(baud, cfo, timing)
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            c1 = fe.chan_open(CR, OFF)
            c2 = p25.cqpsk_demod(fe, c1, CR, baud)
            _push_blocks(fe, x, BLK)
            soft = fe.chan_read_costas(c2)
            st = fe.chan_costas_state(c2)
            agc = fe.chan_read_agc(c2)
        params = p25.costas_params(CR, baud)
        s32, g32 = R.gardner_costas(agc, params, bank)
        s64, _ = R.gardner_costas(agc, params, bank, dtype=np.float64)
        out[case] = dict(soft=soft, st=st, agc=agc, sent=sent, s32=s32, g32=g32, s64=s64, x=x,
                         delay=R.chain_delay(params["omega"], len(taps), D))
    return out


@pytest.mark.parametrize("case", R.CASES)
def test_parity_with_the_restatement_within_float32_rounding_noise(runs, case):
    r = runs[case]
    soft, s32, s64 = r["soft"], r["s32"], r["s64"]
    assert len(r["agc"]) == -(-len(r["x"]) // 16)                 # outputs at inputs 0, 16, 32, ...
    assert r["st"]["n_symbols"] == len(soft)
    assert abs(len(soft) - len(s32)) <= 1 and abs(len(s64) - len(s32)) <= 1
    n = min(len(soft), len(s32), len(s64))
    assert n > R.SKIP + 900
    rms = float(np.sqrt(np.mean(R.angle_diff_mod8(soft[R.SKIP:n], s32[R.SKIP:n]) ** 2)))
    yard = float(np.sqrt(np.mean(R.angle_diff_mod8(s32[R.SKIP:n], s64[R.SKIP:n]) ** 2)))
    print("%s: GPU against float32 restatement rms %.3e; yardstick (float32 against float64 restatement) %.3e; %d symbols"
          % (case, rms, yard, n - R.SKIP))
    assert rms <= yard, (case, rms, yard)
    # the start.  With the AGC of 1024 the loop reads zeros for its first 196 symbols or so: [0, 16) compares 0 with 0 (a
    # loop fed zeros puts out zeros, whatever its history holds), and [0, SKIP) covers the first symbols of the signal on a
    # loop that has been running.  A start on a live signal -- the zero history, the first chunk, windows that reach into
    # CostasState::hist -- is what the AGC-64 tests below compare from symbol 0: the mixed-rate lanes and the lanes of the
    # 130-channel test (a late lane of each starts in the middle of the signal), and gain_mu -40
    for lo, hi in ((0, R.SKIP), (0, 16)):
        g, y = R.distance(soft, s32, lo, hi), R.distance(s32, s64, lo, hi)
        print("    symbols [%d, %d): GPU against float32 restatement rms %.3e, max %.3e; yardstick rms %.3e, max %.3e"
              % (lo, hi, g[0], g[1], y[0], y[1]))
        assert g[1] <= y[1] and (hi == 16 or g[0] <= y[0]), (case, lo, hi, g, y)


@pytest.mark.parametrize("case", R.CASES)
def test_gpu_symbols_slice_to_the_sent_dibits(runs, case):
    r = runs[case]
    assert abs(len(r["soft"]) - R.N_SYMBOLS) <= 2
    assert np.isfinite(r["soft"]).all()
    lag, errs = R.decode_errors(r["soft"], r["sent"], r["delay"], skip=R.SKIP)
    st = r["st"]
    print("%s: %d symbols, chain delay %d + lag %d, %d dibit errors after the first %d; slips %d, freq %.5f rad/sample, omega %.4f"
          % (case, len(r["soft"]), r["delay"], lag, errs, R.SKIP, st["n_slips"], st["freq"], st["omega"]))
    got = p25.slice_dibits(r["soft"])[R.SKIP:]
    a = R.SKIP - r["delay"] - lag
    np.testing.assert_array_equal(got, r["sent"][a:a + len(got)])
    assert errs == 0 and st["n_slips"] == 0
    assert st["freq"] * case[1] < 0                           # the carrier estimate opposes the offset


def test_symbols_do_not_depend_on_the_cuts(gpu_required, runs):
    nat = gpu_required
    case = R.CASES[1]
    x = runs[case]["x"]
    rng = np.random.default_rng(33)
    # ~110 pieces: random ones, a run shorter than one channel sample (16 inputs) and runs shorter than one symbol (83 inputs)
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 45)}
    cuts |= {16 * 2000 + 5 * k for k in range(1, 14)} | {16 * 4100 + 3 + 16 * k for k in range(24)} | {16 * 6000 + 40 * k for k in range(24)}
    cuts = sorted(cuts)
    assert sum(b - a < 16 for a, b in zip(cuts[:-1], cuts[1:])) >= 10 and sum(b - a < 83 for a, b in zip(cuts[:-1], cuts[1:])) >= 50

    def run(pieces):
        with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
            c2 = p25.cqpsk_demod(fe, fe.chan_open(CR, OFF), CR, case[0])
            for a, b in zip(pieces[:-1], pieces[1:]):
                fe.push(x[a:b])
            return fe.chan_read_costas(c2), fe.chan_costas_state(c2), fe.chan_read_agc(c2)

    s1, st1, a1 = run([0, len(x)])
    s2, st2, a2 = run(cuts)
    assert a1.tobytes() == a2.tobytes()
    _same_bits(s2, s1, "cuts")
    assert st1 == st2 and st1["n_symbols"] == len(s1) and st1["n_slips"] == 0
    _same_bits(s1, runs[case]["soft"], "blocks of 1000")


def _many(nat, x, attach, K, blk, lin):
    """130 direct channels with an AGC of 64 each; attach(k) -> None, or (block the stage is attached before, baud,
    caller's bank or None).  -> per channel the soft symbols (or None), and the T_COSTAS launch count"""
    offs = [-190000.0 + 2900.0 * k for k in range(130)]
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [fe.chan_open(CR, f) for f in offs]
        for k, c in enumerate(cids):
            if attach(k):
                fe.chan_agc(c, 64, 1.0)
        fe.timing_enable(True, classes=[nat.T_COSTAS])
        for b in range(K):
            for k, c in enumerate(cids):
                if attach(k) and attach(k)[0] == b:
                    fe.chan_costas(c, interp_taps=lin if attach(k)[2] else None, **p25.costas_params(CR, attach(k)[1]))
            fe.push(x[b * blk:(b + 1) * blk])
        launches = fe.timing_read(nat.T_COSTAS)[1]
        out = [(fe.chan_read_costas(c), fe.chan_costas_state(c), fe.chan_read_agc(c)) if attach(k) else None
               for k, c in enumerate(cids)]
    return out, launches


def test_130_channels_three_workgroups_one_launch_per_block(gpu_required, bank):
    nat = gpu_required
    blk, K = 4000, 6                                          # 250 channel samples a block
    rng = np.random.default_rng(130)
    n = blk * K
    x = (0.05 * synth.awgn(rng, n)).astype(np.complex64)
    carriers = ((0, 4800), (63, 6000), (64, 4800), (129, 6000), (30, 4800))
    for k, baud in carriers:
        sent = rng.integers(0, 4, n * baud // int(FS) + 2)
        x = x + R.dqpsk_carrier(sent, baud, FS, -190000.0 + 2900.0 * k + 60.0, 0.4, amplitude=0.2, n_samples=n)
    x = x.astype(np.complex64)
    lin = M.linear_bank()

    def attach(k):                                            # mixed omega; a caller's bank on 64 and 100; 63 and 7 two blocks late
        return (2 if k in (63, 7) else 0, 6000 if k % 2 else 4800, k in (64, 100))

    many, launches = _many(nat, x, attach, K, blk, lin)
    assert launches == K                                      # one launch per block carries all 130 (three workgroups: 64 + 64 + 2)
    for k, (sym, st, _) in enumerate(many):
        omega = 25000.0 / (6000 if k % 2 else 4800)
        n_in = (K - attach(k)[0]) * blk // 16
        assert st["n_symbols"] == len(sym) and abs(len(sym) - n_in / omega) <= 2, (k, len(sym))
        assert np.isfinite(sym).all() and st["n_slips"] == 0, k
    for k in (0, 63, 64, 129):                                # first and last lane of a workgroup, the two-lane workgroup
        alone, launches = _many(nat, x, lambda j, k=k: attach(j) if j == k else None, K, blk, lin)
        assert launches == K - attach(k)[0]
        _same_bits(alone[k][0], many[k][0], ("lane", k))
        assert alone[k][1] == many[k][1], k
        # ... and against the restatement of the lane's own AGC stream, from the block the loop was attached before
        agc = many[k][2][attach(k)[0] * blk // 16:]
        params = p25.costas_params(CR, attach(k)[1])
        s32, g32 = R.gardner_costas(agc, params, lin if attach(k)[2] else bank)
        s64, _ = R.gardner_costas(agc, params, lin if attach(k)[2] else bank, dtype=np.float64)
        assert len(many[k][2]) == n // 16 and len(many[k][0]) == len(s32) == len(s64), (k, len(many[k][0]), len(s32), len(s64))
        g, y = R.distance(many[k][0], s32), R.distance(s32, s64)
        print("lane %d of 130: %d symbols, GPU against float32 restatement rms %.3e, max %.3e; yardstick rms %.3e, max %.3e"
              % (k, len(s32), g[0], g[1], y[0], y[1]))
        assert g[0] <= y[0], (k, g, y)
        if k in dict(carriers):
            g16, y16 = R.distance(many[k][0], s32, 0, 16)[1], R.distance(s32, s64, 0, 16)[1]
            print("    the first 16 symbols: max %.3e; yardstick %.3e" % (g16, y16))
            assert g16 <= y16, (k, g16, y16)
    assert many[64][0].tobytes() != many[0][0].tobytes()


def test_two_front_ends_in_a_group_share_the_launch(gpu_required):
    nat = gpu_required
    K = 8
    n = BLK * K
    rng = np.random.default_rng(2)
    offs = [(-100000.0, 60000.0), (30000.0, -150000.0)]
    bauds = [(4800, 6000), (6000, 4800)]
    xs = []
    for m in range(2):
        x = np.zeros(n, dtype=np.complex64)
        for j in range(2):
            sent = rng.integers(0, 4, n * bauds[m][j] // int(FS) + 2)
            x = x + R.dqpsk_carrier(sent, bauds[m][j], FS, offs[m][j] + 80.0, 0.45, amplitude=0.3, n_samples=n)
        xs.append(x.astype(np.complex64))

    def setup(fe, m):
        return [p25.cqpsk_demod(fe, fe.chan_open(CR, offs[m][j]), CR, bauds[m][j]) for j in range(2)]

    fes = [nat.Frontend(FS, device=0, block_capacity=BLK) for _ in range(2)]
    try:
        ids = [setup(fe, m) for m, fe in enumerate(fes)]
        fes[0].timing_enable(True, classes=[nat.T_COSTAS])
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * BLK:(b + 1) * BLK] for xm in xs])
            g.sync()
            assert fes[0].timing_read(nat.T_COSTAS)[1] == K   # one launch per group block for both members
            grouped = [[(fe.chan_read_costas(c), fe.chan_costas_state(c)) for c in ids[m]] for m, fe in enumerate(fes)]
    finally:
        for fe in fes:
            fe.close()
    for m in range(2):
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            cs = setup(fe, m)
            _push_blocks(fe, xs[m], BLK)
            for j, c in enumerate(cs):
                sym, st = fe.chan_read_costas(c), fe.chan_costas_state(c)
                assert len(sym) > 1000 and st["n_slips"] == 0
                _same_bits(grouped[m][j][0], sym, ("group", m, j))
                assert grouped[m][j][1] == st


def test_symbol_ring_wraps(gpu_required, runs):
    """out_capacity 256 and 1500 symbols: the soft-symbol ring (and the AGC ring it reads) wraps more than twice; read after
    every push, the concatenation is the stream of the same pushes into rings that never wrap"""
    nat = gpu_required
    case = R.CASES[3]
    x = runs[case]["x"]
    blk = 16 * 160                                            # 160 channel samples: 160 + 63 (the AGC's reach) <= 256

    def run(out_capacity):
        parts = []
        with nat.Frontend(FS, device=0, block_capacity=blk, **({"out_capacity": out_capacity} if out_capacity else {})) as fe:
            c = fe.chan_open(CR, OFF)
            fe.chan_agc(c, 64, 1.0)
            fe.chan_costas(c, **p25.costas_params(CR, case[0]))
            cap = fe.chan_costas_ring(c)[1]
            for a in range(0, len(x), blk):
                fe.push(x[a:a + blk])
                parts.append(fe.chan_read_costas(c))
            return np.concatenate(parts), parts, fe.chan_costas_state(c), cap

    s_small, parts, st_small, cap = run(256)
    s_big, _, st_big, cap_big = run(None)
    assert cap == 256 and cap_big > 2048 and len(s_small) > 2 * cap + 900 and all(len(p) < cap for p in parts)
    _same_bits(s_small, s_big, "wrapped ring")
    assert st_small == st_big and st_small["n_symbols"] == len(s_small)


def test_lifecycle_and_refusals(gpu_required, runs):
    nat = gpu_required
    case = R.CASES[0]
    x = runs[case]["x"]
    kw = p25.costas_params(CR, case[0])
    nan, inf = float("nan"), float("inf")

    def run(first_attach):
        """the stage attached before block first_attach (None: not at first), switched off after block 2, attached
        (again) before block 4"""
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            c1 = fe.chan_open(CR, OFF)
            c2 = p25.cqpsk_front_half(fe, c1, CR)
            if first_attach is not None:
                fe.chan_costas(c2, **kw)
                assert fe.chan_costas_state(c2)["n_symbols"] == 0
            _push_blocks(fe, x[:3 * BLK], BLK)
            first = None
            if first_attach is not None:
                first = fe.chan_read_costas(c2)
                assert len(first) > 500
                assert _code(nat, fe.chan_agc, c2, 0, 1.0) == nat.RCF_ESTATE        # the stage reads the AGC
                assert len(fe.chan_read_agc(c2)) == 3000                            # ... which is still there
                fe.chan_set_offset(c1, OFF + 20.0)                                  # a retune keeps the stage
                fe.chan_costas(c2, None)
                fe.chan_costas(c2, None)                                            # off twice: nothing to do
                for f in (fe.chan_read_costas, fe.chan_costas_state, fe.chan_costas_ring):
                    assert _code(nat, f, c2) == nat.RCF_ESTATE
            else:
                fe.chan_set_offset(c1, OFF + 20.0)
            fe.push(x[3 * BLK:4 * BLK])
            fe.chan_costas(c2, **kw)
            st0 = fe.chan_costas_state(c2)
            assert st0["n_symbols"] == 0 and st0["n_slips"] == 0 and st0["freq"] == 0.0
            assert st0["mu"] == st0["omega"] == np.float32(kw["omega"])
            _push_blocks(fe, x[4 * BLK:7 * BLK], BLK)
            again = fe.chan_read_costas(c2)
            st = fe.chan_costas_state(c2)
            fe.chan_close(c2)                                                       # closed with the stage attached
            assert _code(nat, fe.chan_read_costas, c2) == nat.RCF_ENOCHAN
        return first, again, st

    first, again, st = run(0)
    _, fresh, st_fresh = run(None)
    assert abs(len(again) - 3000 / kw["omega"]) <= 2 and st["n_symbols"] == len(again)
    _same_bits(again, fresh, "re-attached: symbol 0 is the first of the call, nothing of the earlier loop remains")
    assert st == st_fresh
    _same_bits(first, runs[case]["soft"][:len(first)], "before the restart")

    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        c = fe.chan_open(CR, OFF)
        assert _code(nat, fe.chan_costas, c, **kw) == nat.RCF_ESTATE                # no AGC
        assert _code(nat, fe.chan_costas, 999, **kw) == nat.RCF_ENOCHAN
        assert _code(nat, fe.chan_read_costas, 999) == nat.RCF_ENOCHAN
        for f in (fe.chan_read_costas, fe.chan_costas_state, fe.chan_costas_ring):
            assert _code(nat, f, c) == nat.RCF_ESTATE                               # no stage yet
        fe.chan_agc(c, 1024, 1.0)
        for name in kw:
            for bad in (nan, inf, -inf):
                assert _code(nat, fe.chan_costas, c, **dict(kw, **{name: bad})) == nat.RCF_EINVAL, (name, bad)
        for bad in (dict(omega=1.9), dict(omega=16.5), dict(omega=2.02), dict(omega=6.0, omega_limit=3.99),
                    dict(omega=6.0, gain_mu=4.0), dict(omega_limit=-0.001), dict(max_freq=-0.1), dict(max_freq=3.2),
                    dict(max_freq=float(np.float32(np.pi)))):
            assert _code(nat, fe.chan_costas, c, **dict(kw, **bad)) == nat.RCF_EINVAL, bad
        with pytest.raises(ValueError):
            fe.chan_costas(c, interp_taps=np.zeros((128, 8), dtype=np.float32), **kw)
        # (the rule holds for the float32 values the ABI carries: 2.03f - 0.005f - 0.025f is just under 2)
        for ok in (dict(omega=2.04), dict(omega=16.0), dict(max_freq=3.14), dict(max_freq=0.0, omega_limit=0.0)):
            fe.chan_costas(c, **dict(kw, **ok))
        fe.chan_agc(c, 512, 1.0)                                                    # the AGC again, with a window: allowed
        assert _code(nat, fe.chan_agc, c, 0, 1.0) == nat.RCF_ESTATE
        fe.chan_costas(c, None)
        fe.chan_agc(c, 0, 1.0)
    with nat.Frontend(FS, device=0, block_capacity=BLK, out_capacity=32) as fe:
        c = fe.chan_open(CR, OFF)
        fe.chan_agc(c, 16, 1.0)
        assert _code(nat, fe.chan_costas, c, **kw) == nat.RCF_ECAP


def _decodes(nat, fe, cid, sent, omega, delay, what):
    sym, st = fe.chan_read_costas(cid), fe.chan_costas_state(cid)
    lag, errs = R.decode_errors(sym, sent, delay, skip=R.SKIP)
    print("%s: %d symbols (omega %.4f), delay %d + lag %d, %d dibit errors after the first %d, slips %d"
          % (what, len(sym), omega, delay, lag, errs, R.SKIP, st["n_slips"]))
    assert st["n_symbols"] == len(sym) and abs(len(sym) - len(sent)) <= 3
    assert errs == 0 and st["n_slips"] == 0


def test_stage2_channel_and_filterbank_tap(gpu_required):
    """the other channel kinds that can carry an AGC (the chained pre-filter channel is the one every test above uses): a
    channel on a bin of a 64-bin bank, and a tap of a 400-bin reference-grid bank"""
    nat = gpu_required
    # a stage-2 channel: 3.2 Msps, 64 bins of 50 kS/s, pfb_chan_open -> decimation 2, 25 kS/s
    fs, nb = 3.2e6, 64
    rng = np.random.default_rng(64)
    sent = rng.integers(0, 4, R.N_SYMBOLS).astype(np.uint8)
    x = R.dqpsk_carrier(sent, 4800, fs, 5 * fs / nb + 120.0, 0.4)
    proto = G.low_pass_2(1.0, fs, fs / nb * 0.4, fs / nb * 0.2, 60.0, G.WIN_BLACKMAN_HARRIS)
    blk = nb * 2000
    with nat.Frontend(fs, 0.0, device=0, block_capacity=blk) as fe:
        fe.pfb_open(nb, nb, proto)
        c = fe.pfb_chan_open(5, CR, 0.0)
        rate = fe.chan_info(c)["out_rate"]
        fe.chan_agc(c, 1024, 1.0)
        kw = dict(p25.costas_params(CR, 4800), omega=rate / 4800.0, max_freq=2 * np.pi * 1200.0 / rate)
        fe.chan_costas(c, **kw)
        _push_blocks(fe, x, blk)
        _decodes(nat, fe, c, sent, kw["omega"], int(1023 / kw["omega"]), "stage-2 channel at %.0f S/s" % rate)
        assert rate == 25000.0
    # a tap of a 400-bin bank at 5 Msps (25 kS/s, the reference's own channel filter)
    fs = 5e6
    D, taps = G.channel_params(fs, CR)
    sent = rng.integers(0, 4, R.N_SYMBOLS).astype(np.uint8)
    x = R.dqpsk_carrier(sent, 4800, fs, 21 * fs / 400 - 140.0, 0.1)
    with nat.Frontend(fs, 0.0, device=0, block_capacity=D * 1000, hist_capacity=1 << 15, out_capacity=1 << 13) as fe:
        fe.pfb_open(2 * D, D, taps)
        tap = fe.pfb_tap_open(21, gr_phase=True)
        fe.chan_agc(tap, 1024, 1.0)
        fe.chan_costas(tap, **p25.costas_params(CR, 4800))
        _push_blocks(fe, x, D * 1000)
        _decodes(nat, fe, tap, sent, 25000 / 4800.0, R.chain_delay(25000 / 4800.0, len(taps), D, pre_ntaps=1), "filterbank tap")


# ---- beyond the P25 operating point.  tests/test_costas_cpu.py decides every input below on the oracle chain; the
# yardsticks here are taken on the GPU's own AGC streams


def _mixed_run(nat, x, only=None):
    """the eight channels of R.MIXED with their AGCs in one front-end, the loop on all of them (or on `only`) -> per
    channel with the loop (soft symbols, state, AGC stream), and the T_COSTAS launch count"""
    lin = M.linear_bank()
    with nat.Frontend(FS, device=0, block_capacity=R.MIXED_BLK) as fe:
        cids = [fe.chan_open(row[0], row[2]) for row in R.MIXED]
        for c in cids:
            fe.chan_agc(c, R.MIXED_AGC_N, 1.0)
        fe.timing_enable(True, classes=[nat.T_COSTAS])
        for b in range(R.MIXED_BLOCKS):
            for k, (cr, baud, _, _, _, late, own, _) in enumerate(R.MIXED):
                if late == b and only in (None, k):
                    fe.chan_costas(cids[k], interp_taps=lin if own else None, **p25.costas_params(cr, baud))
            fe.push(x[b * R.MIXED_BLK:(b + 1) * R.MIXED_BLK])
        launches = fe.timing_read(nat.T_COSTAS)[1]
        out = {k: (fe.chan_read_costas(c), fe.chan_costas_state(c), fe.chan_read_agc(c))
               for k, c in enumerate(cids) if only in (None, k)}
    return out, launches


@pytest.fixture(scope="module")
def mixed(gpu_required, bank):
    """the wave of R.MIXED on the GPU, and per channel the float32 and float64 restatements of its own AGC stream from the
    block its loop was attached before"""
    x, sent = R.mixed_signal()
    wave, launches = _mixed_run(gpu_required, x)
    ref = {}
    for k, (cr, baud, _, _, _, late, own, _) in enumerate(R.MIXED):
        D, _ = G.channel_params(FS, cr)
        a = wave[k][2][late * R.MIXED_BLK // D:]
        params = p25.costas_params(cr, baud)
        T = M.linear_bank() if own else bank
        s32, g32 = R.gardner_costas(a, params, T)
        ref[k] = (s32, g32, R.gardner_costas(a, params, T, dtype=np.float64)[0])
    return dict(x=x, sent=sent, wave=wave, launches=launches, ref=ref)


def test_mixed_rates_and_omega_range_in_one_wave(gpu_required, mixed):
    """eight loops at 12.5, 25 and 50 kS/s in one wave: n_k = 500, 1000 and 2000 a block, so the lanes leave the chunk loop
    at different trips while the others keep overwriting the columns behind their history; omega 2.08 (L = 10) to 16
    (L = 32, the window is the whole history); one lane joins two blocks late, one brings its own bank (a second pass)"""
    nat = gpu_required
    x, sent, wave = mixed["x"], mixed["sent"], mixed["wave"]
    assert mixed["launches"] == R.MIXED_BLOCKS                         # one launch per block carries all eight
    D_of = {}
    for k, (cr, baud, off, cfo, timing, late, own, skip) in enumerate(R.MIXED):
        sym, st, agc = wave[k]
        D, taps = G.channel_params(FS, cr)
        D_of[k] = D
        assert len(agc) == R.MIXED_BLOCKS * R.MIXED_BLK // D
        params = p25.costas_params(cr, baud)
        s32, g32, s64 = mixed["ref"][k]
        assert st["n_symbols"] == len(sym) == len(s32) and st["n_slips"] == 0, (k, st, len(sym), len(s32))
        assert len(s64) == len(s32) and g32.L == R.window_length(params["omega"])
        g, y = R.distance(sym, s32), R.distance(s32, s64)
        print("mixed %d: %d S/s, %d baud, omega %.4f, L %d, n_k %d, %d symbols; GPU against float32 restatement rms %.3e, "
              "max %.3e; yardstick rms %.3e, max %.3e" % (k, 2 * cr, baud, params["omega"], g32.L, R.MIXED_BLK // D, len(sym),
                                                         g[0], g[1], y[0], y[1]))
        assert g[0] <= y[0] and g[1] <= y[1], (k, g, y)
        if skip is not None:
            delay = R.chain_delay(params["omega"], len(taps), D, pre_ntaps=1, agc_n=R.MIXED_AGC_N)
            lag, errs = R.decode_errors(sym, sent[k][late * R.MIXED_BLK * baud // int(FS):], delay, skip=skip)
            print("    delay %d + lag %d, %d dibit errors after the first %d" % (delay, lag, errs, skip))
            assert errs == 0, (k, errs)
    assert sorted(set(R.MIXED_BLK // D for D in D_of.values())) == [500, 1000, 2000]
    for k in wave:                                            # each loop alone in a front-end: the same bits
        alone, launches = _mixed_run(nat, x, only=k)
        assert launches == R.MIXED_BLOCKS - R.MIXED[k][5]
        _same_bits(alone[k][0], wave[k][0], ("alone", k))
        assert alone[k][1] == wave[k][1], k


@pytest.fixture(scope="module")
def clamped(gpu_required, bank):
    """the window-clamp case on the GPU, and the float32 and float64 restatements of its AGC stream"""
    x, _ = R.case_signal(*R.CLAMP_CASE)
    params = dict(p25.costas_params(CR, R.CLAMP_CASE[0]), **R.CLAMP_PARAMS)
    with gpu_required.Frontend(FS, device=0, block_capacity=BLK) as fe:
        c2 = p25.cqpsk_front_half(fe, fe.chan_open(CR, OFF), CR)
        fe.chan_costas(c2, **params)
        _push_blocks(fe, x, BLK)
        soft, st, agc = fe.chan_read_costas(c2), fe.chan_costas_state(c2), fe.chan_read_agc(c2)
    return (params, soft, st) + R.gardner_costas(agc, params, bank) + R.gardner_costas(agc, params, bank, dtype=np.float64)


def test_window_clamp(clamped):
    """hs = min(hs, L - 8) taken: omega pinned at 4.15 with L = 10.  Without it the second window would read a column that
    is not derotated yet.  The loop is chaotic, so symbols are compared over the prefix in which the float32 and float64
    restatements are still the same loop, and the whole run must stay within its limits"""
    params, soft, st, s32, g32, s64, g64 = clamped
    P, hits = R.comparable_prefix(s32, g32, s64, g64)
    assert P >= 64 and len(hits) >= 3, (P, hits)              # (the conditions of the CPU test, on this stream)
    g, y = R.distance(soft, s32, 0, P)[1], R.distance(s32, s64, 0, P)[1]
    far = np.flatnonzero(np.abs(R.angle_diff_mod8(soft[:P], s32[:P])) > y)
    print("window clamp: %d symbols (restatement %d), the restatement took the clamp %d times, %d within P = %d, first at %s; "
          "GPU against float32 restatement over [0, P): max %.3e; yardstick %.3e; omega %.4f, freq %.5f"
          % (len(soft), len(s32), g32.n_clamped, len(hits), P, hits[:3], g, y, st["omega"], st["freq"]))
    assert g <= y, (g, y, far[:4], hits[:4])
    assert st["n_symbols"] == len(soft) and abs(len(soft) - len(s32)) <= 2
    assert np.isfinite(soft).all()
    mid, lim = np.float32(params["omega"]), np.float32(params["omega_limit"])
    assert mid - lim <= np.float32(st["omega"]) <= mid + lim
    assert abs(st["freq"]) <= np.float32(params["max_freq"])


@pytest.fixture(scope="module")
def bursts(gpu_required, bank):
    """the two burst cases and the clean signal as three grouped front-ends on the GPU, the clean one alone as well, and
    the float32 and float64 restatements of the two poisoned AGC streams"""
    nat = gpu_required
    sig = [R.burst_signal(*b[:4]) for b in R.BURSTS] + [R.burst_signal(R.BURST_CLEAN)]
    bauds = [b[0][0] for b in R.BURSTS] + [R.BURST_CLEAN[0]]
    n = max(len(x) for x, _ in sig)                           # (the 6000-baud signal ends first: its member is skipped then)
    fes = [nat.Frontend(FS, device=0, block_capacity=BLK) for _ in sig]
    try:
        ids = [p25.cqpsk_demod(fe, fe.chan_open(CR, OFF), CR, baud) for fe, baud in zip(fes, bauds)]
        fes[0].timing_enable(True, classes=[nat.T_COSTAS])
        with nat.Group(fes) as g:
            for a in range(0, n, BLK):
                g.push([x[a:a + BLK] for x, _ in sig])
            g.sync()
            launches = fes[0].timing_read(nat.T_COSTAS)[1]
            got = [(fe.chan_read_costas(c), fe.chan_costas_state(c), fe.chan_read_agc(c)) for fe, c in zip(fes, ids)]
    finally:
        for fe in fes:
            fe.close()
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:                  # the clean one without its neighbours
        c = p25.cqpsk_demod(fe, fe.chan_open(CR, OFF), CR, bauds[2])
        _push_blocks(fe, sig[2][0], BLK)
        clean = (fe.chan_read_costas(c), fe.chan_costas_state(c))
    ref = []
    for k, b in enumerate(R.BURSTS):
        params = p25.costas_params(CR, b[0][0])
        ref.append(R.gardner_costas(got[k][2], params, bank) + R.gardner_costas(got[k][2], params, bank, dtype=np.float64))
    return dict(sig=sig, n=n, launches=launches, got=got, clean=clean, ref=ref)


def test_coming_back_from_non_finite_input(bursts):
    """a NaN and an Inf burst in the front-end input of two loops, and an untouched third: three front-ends in a group, so
    that the three loops are lanes of one launch (a front-end has one input, which all of its channels see).  The guard
    fires as often as the restatement's, at the same symbols, the loops come back, the neighbour never notices"""
    sig, got = bursts["sig"], bursts["got"]
    assert bursts["launches"] == -(-bursts["n"] // BLK)       # one launch per group block: three lanes of a wave
    _same_bits(got[2][0], bursts["clean"][0], "the untouched lane")
    assert got[2][1] == bursts["clean"][1] and got[2][1]["n_slips"] == 0 and np.isfinite(got[2][0]).all()
    D, taps = G.channel_params(FS, CR)
    for k, (case, value, at, count, tail_errors) in enumerate(R.BURSTS):
        soft, st, agc = got[k]
        params = p25.costas_params(CR, case[0])
        s32, g32, s64, g64 = bursts["ref"][k]
        a, b = R.burst_span(agc, params["omega"])
        bad, bad32 = np.flatnonzero(~np.isfinite(soft)), np.flatnonzero(~np.isfinite(s32))
        fin = np.isfinite(s32)
        # the yardstick: the float64 run of the same stream, its non-finite symbols masked as well
        assert len(s64) == len(s32) and g64.n_slips == g32.n_slips and np.array_equal(np.flatnonzero(~np.isfinite(s64)), bad32)
        print("burst %s, %d x %s: %d symbols (restatement %d), slips %d (%d), %d non-finite symbols in %s .. %s, %d AGC outputs "
              "not finite, %d zeroed" % (case, count, value, len(soft), len(s32), st["n_slips"], g32.n_slips, len(bad), bad[:1], bad[-1:],
                                         int((~np.isfinite(agc)).sum()), int((agc[len(agc) // 4:] == 0).sum())))
        assert st["n_symbols"] == len(soft) == len(s32)
        assert st["n_slips"] == g32.n_slips > 0
        assert np.array_equal(bad, bad32) and 0 < len(bad) < 0.02 * len(soft)
        gb, yb = R.distance(soft, s32, 0, a, fin), R.distance(s32, s64, 0, a, fin)
        ga, ya = R.distance(soft, s32, b + R.SKIP, None, fin), R.distance(s32, s64, b + R.SKIP, None, fin)
        print("    before symbol %d: GPU against float32 restatement rms %.3e, max %.3e; yardstick rms %.3e, max %.3e"
              % (a, gb[0], gb[1], yb[0], yb[1]))
        print("    after symbol %d: GPU against float32 restatement rms %.3e; yardstick rms %.3e" % (b + R.SKIP, ga[0], ya[0]))
        assert gb[0] <= yb[0] and gb[1] <= yb[1] and ga[0] <= ya[0], (case, gb, yb, ga, ya)
        lag, errs = R.decode_errors(soft, sig[k][1], R.chain_delay(params["omega"], len(taps), D), skip=b + R.SKIP)
        print("    lag %d, %d dibit errors in the tail of %d" % (lag, errs, len(soft) - b - R.SKIP))
        assert len(soft) - b - R.SKIP > 200 and errs == tail_errors
        assert all(np.isfinite(st[f]) for f in ("mu", "omega", "freq", "phase"))


@pytest.mark.parametrize("gain_mu", R.MU_GAINS)
def test_guard_through_mu(gpu_required, bank, gain_mu):
    """the guard's other arm, mu <= 1, by a gain_mu that throws mu about: -40 makes it fire every few symbols; -3e38 sends
    mu to 1e36 at the first error that is not 0, where no input brings it back -- the loop sleeps, the calls return (the
    kernel's trip count is the block's)"""
    nat = gpu_required
    x, _ = R.case_signal(*R.CASES[0], n_symbols=R.MU_SYMBOLS)
    params = dict(p25.costas_params(CR, R.CASES[0][0]), gain_mu=gain_mu)
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        c = fe.chan_open(CR, OFF)
        fe.chan_agc(c, R.MU_AGC_N, 1.0)
        fe.chan_costas(c, **params)
        _push_blocks(fe, x, BLK)
        soft, st, agc = fe.chan_read_costas(c), fe.chan_costas_state(c), fe.chan_read_agc(c)
        if gain_mu != -40.0:
            _push_blocks(fe, np.concatenate([x, x])[:4 * BLK], BLK)          # four more blocks
            more, st_more, agc_more = fe.chan_read_costas(c), fe.chan_costas_state(c), fe.chan_read_agc(c)
    s32, g32 = R.gardner_costas(agc, params, bank)
    print("gain_mu %g: %d symbols (restatement %d), slips %d (%d), mu %g" % (gain_mu, len(soft), len(s32), st["n_slips"], g32.n_slips, st["mu"]))
    assert st["n_symbols"] == len(soft) == len(s32) and st["n_slips"] == g32.n_slips
    assert np.isfinite(soft).all()
    if gain_mu == -40.0:
        first = R.symbols_before_first_slip(agc, params, bank)
        s64, g64 = R.gardner_costas(agc, params, bank, dtype=np.float64)
        assert g32.n_slips > 0 and first >= 16 and len(s64) == len(s32) and g64.n_slips == g32.n_slips
        g, y = R.distance(soft, s32, 0, first)[1], R.distance(s32, s64, 0, first)[1]
        print("    the %d symbols before the first slip: GPU against float32 restatement max %.3e; yardstick %.3e" % (first, g, y))
        assert g <= y, (g, y)
    else:
        assert len(soft) < 32 and st["n_slips"] == 0 and st["mu"] > 1e30
        assert len(more) == 0 and len(agc_more) == 4 * BLK // 16
        assert (st_more["n_symbols"], st_more["n_slips"]) == (st["n_symbols"], st["n_slips"]) and st_more["mu"] > 1e30
        assert len(R.gardner_costas(np.concatenate([agc, agc_more]), params, bank)[0]) == len(s32)
