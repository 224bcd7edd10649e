"""The P25 C4FM back half on the GPU (rcf_chan_fsk4; p25_control_demod.py:118-135): the symbol loop of op25's fsk4_demod_ff
behind a channel's symbol filter.  include/rcf.h defines the stage (unpinned against op25), tests/fsk4_ref.py restates it.
Its soft symbols are compared with the float64 restatement -- the definition -- run on the same channel's own
chan_read_sym stream; the bar, rms and max, is the distance between the restatement's float32-state and float64 runs on
that input (about 1e-2 max: now and then the two pick neighbouring rows of the interpolator bank).  They slice to the
dibits that were sent (inputs decided by tests/test_fsk4_cpu.py), and they are the same bits however the stream is cut,
however many channels and front-ends share the launch and however small the ring.

Measured on an MI355X, soft-symbol units, GPU against the float64 restatement | yardstick (one run of these tests, their
print lines; DESIGN.md 9, row f-8 has the same).  The loop has nothing transcendental in it and the kernel rounds every
operation as the definition does, so the GPU is expected at 0; the bar asserted is the yardstick.
  six cases, symbols 500 .. 1500       max 0 | 5.9e-3 .. 1.3e-2 (rms 0 | 3.4e-4 .. 1.2e-3)
  six cases, symbols 0 .. 500          max 0 | 3.8e-6 .. 8.5e-3
  lanes 0, 63, 64, 129 of 130, from 0  max 0 | 2.9e-6 .. 7.6e-3
  mixed rates, eight lanes, from 0     max 0 | 1.4e-6 .. 1.6e-2
  NaN / Inf burst at the front-end     max 0 | 8.2e-3 .. 1.2e-2; no slip: the discriminator hands the loop finite values
  poisoned symbol filter, one block    max 0 | 1.3e-3 .. 1.1e-2; 168, 202, 168 slips, as the restatement
  discriminator-only tap (160 bins)    max 0 | 3.0e-3
The final state (clock, spread, fine, coarse) was the restatement's bit for bit in every case."""
import json
import os

import numpy as np
import pytest

import fsk4_ref as F
import mm_ref as M
from oracle import grspec as G
from rcf import p25, synth

pytestmark = pytest.mark.gpu

FS, CR, OFF = F.FS, F.CHANNEL_RATE, F.CHANNEL_OFFSET
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


def _read(fe, c):
    return fe.chan_read_fsk4(c), fe.chan_fsk4_state(c), fe.chan_read_sym(c)


def _within_yardstick(soft, u, params, T, what, lo=0, hi=None):
    """the GPU's soft symbols against the float64 restatement of u, symbol for symbol; the bar is the float32-state run's
    distance from it (over the symbols both of those runs have, should a loop that does not lock count one more or less
    in float32).  -> (s64, stage64)"""
    s64, g64 = F.fsk4_demod(u, params, T)
    s32, _ = F.fsk4_demod(u, params, T, dtype=np.float32)
    assert len(soft) == len(s64) and abs(len(s32) - len(s64)) <= 2, (what, len(soft), len(s64), len(s32))
    hi = min(len(s32), len(s64)) if hi is None else hi
    g, y = F.distance(soft, s64, lo, hi), F.distance(s32, s64, lo, hi)
    print("%s, symbols [%d, %s): GPU against float64 restatement rms %.3e, max %.3e; yardstick (float32-state against float64 "
          "restatement) rms %.3e, max %.3e" % (what, lo, hi if hi is not None else len(s64), g[0], g[1], y[0], y[1]))
    assert g[0] <= y[0] and g[1] <= y[1], (what, lo, hi, g, y)
    return s64, g64


@pytest.fixture(scope="module")
def bank(gpu_required):
    return gpu_required.design_mmse_interpolator()


@pytest.fixture(scope="module")
def runs(gpu_required, bank):
    """per case: the GPU's soft symbols, its symbol-filter stream and state"""
    nat = gpu_required
    D, taps = G.channel_params(FS, CR)
    out = {}
    for case in F.CASES:
        x, sent = F.case_signal(*case)
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            c2 = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, case[0])
            _push_blocks(fe, x, BLK)
            soft, st, u = _read(fe, c2)
        sps = len(p25.symbol_taps(CR, case[0]))
        out[case] = dict(soft=soft, st=st, u=u, sent=sent, x=x, params=p25.fsk4_params(CR, case[0]),
                         delay=F.chain_delay(2.0 * CR / case[0], len(taps), D, box=sps))
    return out


@pytest.mark.parametrize("case", F.CASES)
def test_parity_with_the_restatement_within_the_float32_state_yardstick(runs, bank, case):
    r = runs[case]
    assert len(r["u"]) == -(-len(r["x"]) // 16)                   # outputs at inputs 0, 16, 32, ...
    assert r["st"]["n_symbols"] == len(r["soft"])
    for lo, hi in ((0, F.SKIP), (F.SKIP, None)):
        _, g64 = _within_yardstick(r["soft"], r["u"], r["params"], bank, case, lo, hi)
    assert len(r["soft"]) > F.SKIP + 900
    ref = g64.state()
    print("    state: GPU %s; restatement %s" % (r["st"], ref))
    assert (r["st"]["n_symbols"], r["st"]["n_slips"]) == (ref["n_symbols"], ref["n_slips"])


@pytest.mark.parametrize("case", F.CASES)
def test_gpu_symbols_slice_to_the_sent_dibits(runs, case):
    r = runs[case]
    assert abs(len(r["soft"]) - F.N_SYMBOLS) <= 2
    assert np.isfinite(r["soft"]).all()
    lag, errs = F.decode_errors(r["soft"], r["sent"], r["delay"], skip=F.SKIP)
    st = r["st"]
    print("%s: %d symbols, chain delay %d + lag %d, %d dibit errors after the first %d; slips %d, spread %.4f, fine %.4f, coarse %.4f"
          % (case, len(r["soft"]), r["delay"], lag, errs, F.SKIP, st["n_slips"], st["spread"], st["fine"], st["coarse"]))
    got = p25.slice_dibits(r["soft"])[F.SKIP:]
    a = F.SKIP - r["delay"] - lag
    np.testing.assert_array_equal(got, r["sent"][a:a + len(got)])
    assert errs == 0 and st["n_slips"] == 0
    if case[1]:
        assert st["coarse"] * case[1] > 0                         # the offset estimate has the carrier offset's sign


def test_symbols_do_not_depend_on_the_cuts(gpu_required, runs):
    nat = gpu_required
    case = F.CASES[1]
    x = runs[case]["x"]
    rng = np.random.default_rng(33)
    # ~110 pieces: random ones, a run shorter than one channel sample (16 inputs) and runs shorter than one symbol (83 inputs)
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 45)}
    cuts |= {16 * 2000 + 5 * k for k in range(1, 14)} | {16 * 4100 + 3 + 16 * k for k in range(24)} | {16 * 6000 + 40 * k for k in range(24)}
    cuts = sorted(cuts)
    assert sum(b - a < 16 for a, b in zip(cuts[:-1], cuts[1:])) >= 10 and sum(b - a < 83 for a, b in zip(cuts[:-1], cuts[1:])) >= 50

    def run(pieces):
        with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
            c2 = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, case[0])
            for a, b in zip(pieces[:-1], pieces[1:]):
                fe.push(x[a:b])
            return _read(fe, c2)

    s1, st1, u1 = run([0, len(x)])
    s2, st2, u2 = run(cuts)
    assert u1.tobytes() == u2.tobytes()
    _same_bits(s2, s1, "cuts")
    assert st1 == st2 and st1["n_symbols"] == len(s1) and st1["n_slips"] == 0
    _same_bits(s1, runs[case]["soft"], "blocks of 1000")
    assert st1 == runs[case]["st"]


def _many(nat, x, attach, K, blk, lin):
    """130 direct channels with their symbol filters; attach(k) -> None, or (block the stage is attached before, baud,
    caller's bank or not).  -> per channel (soft symbols, state, symbol-filter stream) or None, and the T_FSK4 launch count"""
    offs = [-190000.0 + 2900.0 * k for k in range(130)]
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [fe.chan_open(CR, f) for f in offs]
        for k, c in enumerate(cids):
            if attach(k):
                fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, attach(k)[1]))
        fe.timing_enable(True, classes=[nat.T_FSK4])
        for b in range(K):
            for k, c in enumerate(cids):
                if attach(k) and attach(k)[0] == b:
                    fe.chan_fsk4(c, interp_taps=lin if attach(k)[2] else None, **p25.fsk4_params(CR, attach(k)[1]))
            fe.push(x[b * blk:(b + 1) * blk])
        launches = fe.timing_read(nat.T_FSK4)[1]
        out = [_read(fe, c) if attach(k) else None for k, c in enumerate(cids)]
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
        x = x + F.c4fm_carrier(sent, baud, FS, -190000.0 + 2900.0 * k + 60.0, 0.4, amplitude=0.2, n_samples=n)
    x = x.astype(np.complex64)
    lin = M.linear_bank()

    def attach(k):                                            # mixed baud; a caller's bank on 64 and 100; 63 and 7 two blocks late
        return (2 if k in (63, 7) else 0, 6000 if k % 2 else 4800, k in (64, 100))

    many, launches = _many(nat, x, attach, K, blk, lin)
    assert launches == K                                      # one launch per block carries all 130 (three workgroups: 64 + 64 + 2)
    for k, (sym, st, u) in enumerate(many):
        omega = 25000.0 / (6000 if k % 2 else 4800)
        n_in = (K - attach(k)[0]) * blk // 16
        assert len(u) == n // 16
        # (a lane without a carrier, or with its neighbour's in the passband -- 63 and 64 --, demodulates noise: the
        # discriminator's +-20 throws the clock about, the count wanders and the guard may fire)
        assert st["n_symbols"] == len(sym) and 0 < len(sym) <= n_in and np.isfinite(sym).all(), (k, len(sym))
        if k in (0, 30, 129):                                 # a carrier of their own and quiet neighbours
            assert abs(len(sym) - n_in / omega) <= 2 and st["n_slips"] == 0, (k, len(sym), st)
    for k in (0, 63, 64, 129):                                # first and last lane of a workgroup, the two-lane workgroup
        alone, launches = _many(nat, x, lambda j, k=k: attach(j) if j == k else None, K, blk, lin)
        assert launches == K - attach(k)[0]
        _same_bits(alone[k][0], many[k][0], ("lane", k))
        assert alone[k][1] == many[k][1], k
        # ... and against the restatement of the lane's own symbol-filter stream, from the block the loop was attached before
        u = many[k][2][attach(k)[0] * blk // 16:]
        _, g64 = _within_yardstick(many[k][0], u, p25.fsk4_params(CR, attach(k)[1]), lin if attach(k)[2] else bank, "lane %d of 130" % k)
        assert many[k][1]["n_slips"] == g64.n_slips, k
    assert many[64][0].tobytes() != many[0][0].tobytes()


# (chan_open's rate, baud, channel offset, the block the loop is attached before, a caller's bank): channels of 12.5, 25
# and 50 kS/s interleaved across the lanes of one wave, so that with blocks of 16000 inputs n_k is 500, 1000 or 2000 and
# the lanes leave the kernel's chunk loop at different trips; sample_rate / symbol_rate from 2.08 to 16
MIXED_BLK, MIXED_BLOCKS = 16000, 6
MIXED = [
    (25000, 9600, -130000.0, 2, False),      # 5.2083 samples a symbol at 50 kS/s, two blocks late
    (6250, 2400, 20000.0, 0, False),         # 5.2083 at 12.5 kS/s
    (12500, 3125, -75000.0, 0, False),       # 8
    (25000, 3125, 150000.0, 0, False),       # 16
    (6250, 6000, 50000.0, 0, False),         # 2.0833
    (12500, 4800, -25000.0, 0, False),       # the P25 shape
    (12500, 6000, 90000.0, 0, True),         # a caller's bank (linear): a second pass in the wave
    (6250, 2400, -190000.0, 0, False),
]


def test_mixed_rates_in_one_wave(gpu_required, bank):
    nat = gpu_required
    n = MIXED_BLK * MIXED_BLOCKS
    rng = np.random.default_rng(816)
    x = 0.002 * synth.awgn(rng, n)
    for cr, baud, off, _, _ in MIXED:
        d = rng.integers(0, 4, n * baud // int(FS) + 2)
        x = x + F.c4fm_carrier(d, baud, FS, off + 70.0, 0.5, amplitude=0.1, n_samples=n)
    x = x.astype(np.complex64)
    lin = M.linear_bank()
    params = [dict(F.fsk4_params(cr, baud)) for cr, baud, _, _, _ in MIXED]
    assert min(p["sample_rate"] / p["symbol_rate"] for p in params) < 2.1 and max(p["sample_rate"] / p["symbol_rate"] for p in params) == 16.0
    with nat.Frontend(FS, device=0, block_capacity=MIXED_BLK) as fe:
        cids = [fe.chan_open(cr, off) for cr, _, off, _, _ in MIXED]
        for c, (cr, baud, _, _, _) in zip(cids, MIXED):
            fe.chan_fm_filter(c, p25.fm_gain(cr), p25.symbol_taps(cr, baud))
        fe.timing_enable(True, classes=[nat.T_FSK4])
        for b in range(MIXED_BLOCKS):
            for k, (cr, baud, _, late, own) in enumerate(MIXED):
                if late == b:
                    fe.chan_fsk4(cids[k], interp_taps=lin if own else None, **params[k])
            fe.push(x[b * MIXED_BLK:(b + 1) * MIXED_BLK])
        assert fe.timing_read(nat.T_FSK4)[1] == MIXED_BLOCKS
        got = [_read(fe, c) for c in cids]
    assert {MIXED_BLK * 2 * row[0] // int(FS) for row in MIXED} == {500, 1000, 2000}
    for k, ((cr, baud, off, late, own), (sym, st, u)) in enumerate(zip(MIXED, got)):
        n_in = (MIXED_BLOCKS - late) * MIXED_BLK * 2 * cr // int(FS)
        assert len(u) == n * 2 * cr // int(FS)
        assert st["n_symbols"] == len(sym) and 0 < len(sym) <= n_in, (k, len(sym), n_in)     # (the exact count: the restatement's, below)
        _, g64 = _within_yardstick(sym, u[len(u) - n_in:], params[k], lin if own else bank,
                                   "mixed %d (%d S/s, %d baud)" % (k, 2 * cr, baud))
        assert st["n_slips"] == g64.n_slips, k


@pytest.fixture(scope="module")
def bursts(gpu_required, bank):
    """the two burst cases and the clean signal as three grouped front-ends on the GPU, the clean one alone as well"""
    nat = gpu_required
    sig = [F.burst_signal(*b) for b in F.BURSTS] + [F.burst_signal(F.BURST_CLEAN)]
    bauds = [b[0][0] for b in F.BURSTS] + [F.BURST_CLEAN[0]]
    n = max(len(x) for x, _ in sig)                           # (the 6000-baud signal ends first: its member is skipped then)
    fes = [nat.Frontend(FS, device=0, block_capacity=BLK) for _ in sig]
    try:
        ids = [p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, baud) for fe, baud in zip(fes, bauds)]
        fes[0].timing_enable(True, classes=[nat.T_FSK4])
        with nat.Group(fes) as g:
            for a in range(0, n, BLK):
                g.push([x[a:a + BLK] for x, _ in sig])
            g.sync()
            launches = fes[0].timing_read(nat.T_FSK4)[1]
            got = [_read(fe, c) for fe, c in zip(fes, ids)]
    finally:
        for fe in fes:
            fe.close()
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:                  # the clean one without its neighbours
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, bauds[2])
        _push_blocks(fe, sig[2][0], BLK)
        clean = _read(fe, c)
    return dict(sig=sig, n=n, launches=launches, got=got, clean=clean, bauds=bauds)


def _poisoned_lane(soft, st, u, sent, params, T, a, b, what):
    """a lane whose input was poisoned so that only the symbols a .. b can have seen it directly: the guard fired as often
    as the restatement's, the non-finite symbols are the restatement's, parity holds before a and from 500 symbols after b
    on, where the lane decodes again (every slip costs a fraction of a symbol: the lag is searched widely)"""
    s64, g64 = F.fsk4_demod(u, params, T)
    s32, g32 = F.fsk4_demod(u, params, T, dtype=np.float32)
    bad, bad64 = np.flatnonzero(~np.isfinite(soft)), np.flatnonzero(~np.isfinite(s64))
    print("%s: %d symbols (restatement %d, float32 state %d), slips %d (%d, %d), %d inputs of the loop not finite, %d symbols not "
          "finite (%s .. %s)" % (what, len(soft), len(s64), len(s32), st["n_slips"], g64.n_slips, g32.n_slips,
                                 int((~np.isfinite(u)).sum()), len(bad), bad[:1], bad[-1:]))
    assert st["n_symbols"] == len(soft) == len(s64) == len(s32)
    assert st["n_slips"] == g64.n_slips == g32.n_slips
    assert np.array_equal(bad, bad64) and (len(bad) == 0 or (a <= bad[0] and bad[-1] <= b))
    assert all(np.isfinite(st[f]) for f in ("clock", "spread", "fine", "coarse"))
    for lo, hi in ((0, a), (b + F.SKIP, len(s64))):
        g, y = F.distance(soft, s64, lo, hi), F.distance(s32, s64, lo, hi)
        print("    symbols [%d, %d): GPU against float64 restatement rms %.3e, max %.3e; yardstick rms %.3e, max %.3e"
              % (lo, hi, g[0], g[1], y[0], y[1]))
        assert g[0] <= y[0] and g[1] <= y[1], (what, lo, hi, g, y)
    lag, errs = F.decode_errors_any_lag(soft, sent, skip=b + F.SKIP)
    print("    lag %d, %d dibit errors in the tail of %d" % (lag, errs, len(soft) - b - F.SKIP))
    assert len(soft) - b - F.SKIP > 200 and errs == 0
    return g64.n_slips


def test_guard_next_to_a_clean_lane(bursts, bank):
    """a NaN and an Inf burst in the front-end input of two loops, and an untouched third: three front-ends in a group, so
    that the three loops are lanes of one launch (a front-end has one input, which all of its channels see).  The guard
    fires as often as the restatement's on the lane's own symbol-filter stream (the discriminator turns a NaN sample into 0,
    so it may not fire at all: the test below poisons the loop's input itself), the loops decode again, the neighbour
    never notices"""
    sig, got = bursts["sig"], bursts["got"]
    assert bursts["launches"] == -(-bursts["n"] // BLK)       # one launch per group block: three lanes of a wave
    _same_bits(got[2][0], bursts["clean"][0], "the untouched lane")
    assert got[2][1] == bursts["clean"][1] and got[2][1]["n_slips"] == 0 and np.isfinite(got[2][0]).all()
    D, taps = G.channel_params(FS, CR)
    for k, (case, value, at, count) in enumerate(F.BURSTS):
        soft, st, u = got[k]
        params = p25.fsk4_params(CR, case[0])
        omega = params["sample_rate"] / params["symbol_rate"]
        # the loop's inputs the burst can reach: from its first channel sample to the end of the three filters behind it
        first, last = at // 16, (at + count) // 16 + len(taps) // D + 1 + 69 + len(p25.symbol_taps(CR, case[0]))
        bad_u = np.flatnonzero(~np.isfinite(u))
        assert len(bad_u) == 0 or (first <= bad_u[0] and bad_u[-1] <= last), (bad_u[:1], bad_u[-1:], first, last)
        _poisoned_lane(soft, st, u, sig[k][1], params, bank, int(first / omega) - 4, int((last + F.NTAPS) / omega) + 4,
                       "burst %s, %d x %s" % (case, count, value))


def test_guard_fires_on_a_poisoned_symbol_filter(gpu_required, bank):
    """the loop's own input made NaN, non-finite and 1e30 for one block through the symbol filter (a second
    rcf_chan_fm_filter call with NaN taps, an infinite gain, taps of 2e29; the next call puts the boxcar back), on three
    channels of one front-end with a clean fourth in the same launches: the guard fires at every symbol of that block, as
    in the restatement, and 500 symbols later the lanes decode again"""
    nat = gpu_required
    cases = [F.CASES[1], F.CASES[4], F.CASES[3], F.CASES[2]]
    offs = [-150000.0, -50000.0, 50000.0, 150000.0]
    n_symbols = 2500
    n = int(n_symbols * FS / 6000) // BLK * BLK
    x, sent = np.zeros(n, dtype=np.complex64), []
    for case, off in zip(cases, offs):
        xs, d = F.case_signal(*case, offset=off, n_symbols=n_symbols)
        x = x + 0.4 * xs[:n]
        sent.append(d)
    x = x.astype(np.complex64)
    poison = [dict(taps=[float("nan")] * 5), dict(gain=float("inf")), dict(taps=[2e29] * 4), None]
    at = 4                                                    # the block that is poisoned: the loop's inputs 4000 .. 4999

    def run(only=None):
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            cids = {}
            for k, (case, off) in enumerate(zip(cases, offs)):
                if only in (None, k):
                    c = cids[k] = fe.chan_open(CR, off)
                    fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, case[0]))
                    fe.chan_fsk4(c, **p25.fsk4_params(CR, case[0]))
            for b in range(n // BLK):
                for k, c in cids.items():
                    if poison[k] and b in (at, at + 1):
                        kw = dict(gain=p25.fm_gain(CR), taps=p25.symbol_taps(CR, cases[k][0]))
                        fe.chan_fm_filter(c, **(dict(kw, **poison[k]) if b == at else kw))
                fe.push(x[b * BLK:(b + 1) * BLK])
            return {k: _read(fe, c) for k, c in cids.items()}

    got = run()
    alone = run(only=3)
    _same_bits(got[3][0], alone[3][0], "the clean lane")
    assert got[3][1] == alone[3][1] and got[3][1]["n_slips"] == 0 and np.isfinite(got[3][0]).all()
    for k in range(3):
        soft, st, u = got[k]
        params = p25.fsk4_params(CR, cases[k][0])
        omega = params["sample_rate"] / params["symbol_rate"]
        lo, hi = at * BLK // 16, (at + 1) * BLK // 16
        assert np.isfinite(u[:lo]).all() and np.isfinite(u[hi:]).all()
        assert (~np.isfinite(u[lo:hi])).all() if k < 2 else (np.abs(u[lo + 8:hi]) > 1e27).all()
        slips = _poisoned_lane(soft, st, u, sent[k], params, bank, int(lo / omega) - 4, int((hi + F.NTAPS) / omega) + 4,
                               "symbol filter %s" % (poison[k],))
        # one slip per symbol of the block: a loop that starts over at every symbol needs ceil(omega) inputs for the next
        assert abs(slips - (hi - lo) / np.ceil(omega)) <= 3, slips


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
            x = x + F.c4fm_carrier(sent, bauds[m][j], FS, offs[m][j] + 80.0, 0.45, amplitude=0.3, n_samples=n)
        xs.append(x.astype(np.complex64))

    def setup(fe, m):
        return [p25.c4fm_demod(fe, fe.chan_open(CR, offs[m][j]), CR, bauds[m][j]) for j in range(2)]

    fes = [nat.Frontend(FS, device=0, block_capacity=BLK) for _ in range(2)]
    try:
        ids = [setup(fe, m) for m, fe in enumerate(fes)]
        fes[0].timing_enable(True, classes=[nat.T_FSK4])
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * BLK:(b + 1) * BLK] for xm in xs])
            g.sync()
            assert fes[0].timing_read(nat.T_FSK4)[1] == K     # one launch per group block for both members
            grouped = [[(fe.chan_read_fsk4(c), fe.chan_fsk4_state(c)) for c in ids[m]] for m, fe in enumerate(fes)]
    finally:
        for fe in fes:
            fe.close()
    for m in range(2):
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            cs = setup(fe, m)
            _push_blocks(fe, xs[m], BLK)
            for j, c in enumerate(cs):
                sym, st = fe.chan_read_fsk4(c), fe.chan_fsk4_state(c)
                assert len(sym) > 1000 and st["n_slips"] == 0
                _same_bits(grouped[m][j][0], sym, ("group", m, j))
                assert grouped[m][j][1] == st


def test_small_ring_with_reads_between_pushes(gpu_required, runs):
    """out_capacity 256 and 1500 symbols: the soft-symbol ring (and the symbol-filter ring it reads) wraps more than twice;
    read after every push, the concatenation is the stream of the same pushes into rings that never wrap"""
    nat = gpu_required
    case = F.CASES[4]
    x = runs[case]["x"]
    blk = 16 * 160                                            # 160 channel samples a block

    def run(out_capacity):
        parts = []
        with nat.Frontend(FS, device=0, block_capacity=blk, **({"out_capacity": out_capacity} if out_capacity else {})) as fe:
            c = fe.chan_open(CR, OFF)
            fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, case[0]))
            fe.chan_fsk4(c, **p25.fsk4_params(CR, case[0]))
            cap = fe.chan_fsk4_ring(c)[1]
            for a in range(0, len(x), blk):
                fe.push(x[a:a + blk])
                parts.append(fe.chan_read_fsk4(c))
            return np.concatenate(parts), parts, fe.chan_fsk4_state(c), cap

    s_small, parts, st_small, cap = run(256)
    s_big, _, st_big, cap_big = run(None)
    assert cap == 256 and cap_big > 2048 and len(s_small) > 2 * cap + 900 and all(len(p) < cap for p in parts)
    _same_bits(s_small, s_big, "wrapped ring")
    assert st_small == st_big and st_small["n_symbols"] == len(s_small)
    with nat.Frontend(FS, device=0, block_capacity=BLK, out_capacity=8) as fe:
        c = fe.chan_open(CR, OFF)
        fe.chan_fm_filter(c, p25.fm_gain(CR), [0.5, 0.5])
        assert _code(nat, fe.chan_fsk4, c, **p25.fsk4_params(CR, 4800)) == nat.RCF_ECAP


def test_lifecycle_and_refusals(gpu_required, runs, bank):
    nat = gpu_required
    case = F.CASES[1]
    x = runs[case]["x"]
    kw = p25.fsk4_params(CR, case[0])
    nan, inf = float("nan"), float("inf")

    def run(first_attach):
        """the stage attached before block first_attach (None: not at first), switched off after block 2, attached
        (again) before block 4"""
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            c1 = fe.chan_open(CR, OFF)
            c2 = p25.c4fm_front_half(fe, c1, CR, case[0])
            if first_attach is not None:
                fe.chan_fsk4(c2, **kw)
                assert fe.chan_fsk4_state(c2)["n_symbols"] == 0
            _push_blocks(fe, x[:BLK], BLK)
            # a second chan_fm_filter call (the same taps again) keeps the stage, its state and its ring
            fe.chan_fm_filter(c2, p25.fm_gain(CR), p25.symbol_taps(CR, case[0]))
            _push_blocks(fe, x[BLK:3 * BLK], BLK)
            first = None
            if first_attach is not None:
                first = fe.chan_read_fsk4(c2)
                assert len(first) > 500
                fe.chan_set_offset(c1, OFF + 20.0)                                  # a retune keeps the stage
                assert fe.chan_fsk4_state(c2)["n_symbols"] == len(first)
                fe.chan_fsk4(c2, None)
                fe.chan_fsk4(c2, None)                                              # off twice: nothing to do
                for f in (fe.chan_read_fsk4, fe.chan_fsk4_state, fe.chan_fsk4_ring):
                    assert _code(nat, f, c2) == nat.RCF_ESTATE
                assert len(fe.chan_read_sym(c2)) == 3000                            # the symbol filter is still there
            else:
                fe.chan_set_offset(c1, OFF + 20.0)
            fe.push(x[3 * BLK:4 * BLK])
            fe.chan_fsk4(c2, **kw)
            st0 = fe.chan_fsk4_state(c2)
            assert st0 == dict(n_symbols=0, n_slips=0, clock=0.0, spread=2.0, fine=0.0, coarse=0.0)
            _push_blocks(fe, x[4 * BLK:7 * BLK], BLK)
            again = fe.chan_read_fsk4(c2)
            st = fe.chan_fsk4_state(c2)
            fe.chan_close(c2)                                                       # closed with the stage attached
            assert _code(nat, fe.chan_read_fsk4, c2) == nat.RCF_ENOCHAN
            c3 = p25.c4fm_demod(fe, c1, CR, case[0])                                # ... and another one opened
            fe.push(x[7 * BLK:8 * BLK])
            # (its pre-filter fills up from zero history in the middle of the signal: the discriminator's transient throws
            # the clock about for a few symbols, so the count is the restatement's, not 1000 / omega)
            soft3, st3, u3 = _read(fe, c3)
            assert 500 < len(u3) <= 1000 and st3["n_symbols"] == len(soft3)        # (a chained channel's first block is short)
            _within_yardstick(soft3, u3, kw, bank, "a channel opened after one with the stage was closed")
        return first, again, st

    first, again, st = run(0)
    _, fresh, st_fresh = run(None)
    assert abs(len(again) - 3000 * case[0] / 25000.0) <= 2 and st["n_symbols"] == len(again)
    _same_bits(again, fresh, "re-attached: symbol 0 is the first of the call, nothing of the earlier loop remains")
    assert st == st_fresh
    _same_bits(first, runs[case]["soft"][:len(first)], "before the restart, across the second chan_fm_filter call")

    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        c = fe.chan_open(CR, OFF)
        assert _code(nat, fe.chan_fsk4, c, **kw) == nat.RCF_ESTATE                  # no symbol filter
        assert _code(nat, fe.chan_fsk4, 999, **kw) == nat.RCF_ENOCHAN
        assert _code(nat, fe.chan_read_fsk4, 999) == nat.RCF_ENOCHAN
        fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR))
        for f in (fe.chan_read_fsk4, fe.chan_fsk4_state, fe.chan_fsk4_ring):
            assert _code(nat, f, c) == nat.RCF_ESTATE                               # no stage yet
        for name in kw:
            for bad in (nan, inf, -inf):
                assert _code(nat, fe.chan_fsk4, c, **dict(kw, **{name: bad})) == nat.RCF_EINVAL, (name, bad)
        for bad in (dict(symbol_rate=12600.0), dict(sample_rate=9500.0), dict(sample_rate=4800.0 * 4097), dict(symbol_rate=0.0),
                    dict(symbol_rate=-4800.0), dict(spread_min=0.0), dict(spread_min=-1.0), dict(spread_min=2.01),
                    dict(spread_max=1.99), dict(spread_min=2.2, spread_max=2.4)):
            assert _code(nat, fe.chan_fsk4, c, **dict(kw, **bad)) == nat.RCF_EINVAL, bad
        with pytest.raises(ValueError):
            fe.chan_fsk4(c, interp_taps=np.zeros((128, 8), dtype=np.float32), **kw)
        for ok in (dict(symbol_rate=12500.0), dict(sample_rate=4800.0 * 4096), dict(spread_min=2.0, spread_max=2.0),
                   dict(spread_min=1e-3, spread_max=1e6)):
            fe.chan_fsk4(c, **dict(kw, **ok))
        fe.chan_fsk4(c, None)


def test_discriminator_only_tap_of_the_smallest_bank(gpu_required, bank):
    """a tap that exposes its discriminator only, on the smallest bank shape of tests/golden/pfb_shapes.json that has such
    taps (a supported frame-major bank: 160 bins, decimation 80, the reference's own channel filter as prototype): the
    stage reads no IQ"""
    nat = gpu_required
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pfb_shapes.json")))
    col = {name: i for i, name in enumerate(g["columns"])}
    nb, D = min((r[col["NB"]], r[col["D"]]) for r in g["rows"] if r[col["supported"]] and r[col["frame_major"]])
    assert (nb, D) == (160, 80)
    fs = 25000.0 * D                                          # 2 MS/s: 160 bins 12.5 kHz apart at 25 kS/s each
    D_, proto = G.channel_params(fs, CR)
    assert D_ == D and any(r[col["NB"]] == nb and r[col["D"]] == D and r[col["supported"]] and r[col["ntaps"]] >= len(proto)
                           for r in g["rows"])
    rng = np.random.default_rng(64)
    sent = rng.integers(0, 4, F.N_SYMBOLS).astype(np.uint8)
    x = F.c4fm_carrier(sent, 4800, fs, 5 * fs / nb + 100.0, 0.5)
    params = p25.fsk4_params(CR, 4800)
    with nat.Frontend(fs, 0.0, device=0, block_capacity=D * 1000, hist_capacity=1 << 14, out_capacity=1 << 13) as fe:
        fe.pfb_open(nb, D, proto)
        tap = fe.pfb_tap_open(5, gr_phase=True)
        fe.chan_set_fm_only(tap, True)
        fe.chan_fm_filter(tap, p25.fm_gain(CR), p25.symbol_taps(CR))
        fe.chan_fsk4(tap, **params)
        _push_blocks(fe, x, D * 1000)
        assert _code(nat, fe.chan_read_iq, tap) == nat.RCF_ESTATE
        soft, st, u = _read(fe, tap)
    assert abs(len(u) - len(x) / D) <= 1 and st["n_symbols"] == len(soft) and abs(len(soft) - F.N_SYMBOLS) <= 2
    _, g64 = _within_yardstick(soft, u, params, bank, "discriminator-only tap of a %d-bin bank" % nb)
    assert st["n_slips"] == g64.n_slips
    lag, errs = F.decode_errors(soft, sent, 0, skip=F.SKIP, max_lag=24)
    print("    lag %d, %d dibit errors after the first %d, slips %d" % (lag, errs, F.SKIP, st["n_slips"]))
