"""Hard decisions on the GPU (rcf_chan_slicer; slice.hip): slicer, MSB-first packing and frame-sync search behind a
channel's symbol loop.  include/rcf.h defines the stage, tests/slicer_ref.py restates it in numpy.  The yardstick is always
that restatement applied to the channel's OWN soft symbols as its loop's reader delivers them (chan_read_clock / _costas /
_fsk4): the stage is integer work on those floats, so every comparison -- words, hits, counters -- is of bits.  (A NaN soft
symbol in binary mode cannot be produced through the chain -- the discriminator hands the clock finite values --; that
rule is held on the kernel's arithmetic header by tests/test_slicer_cpu.py.)"""
import ctypes

import numpy as np
import pytest

import fsk4_ref as F
import gc_ref as R
import mm_ref as M
import slicer_ref as S
from rcf import control, p25, synth

pytestmark = pytest.mark.gpu

FS, CR, OFF = F.FS, F.CHANNEL_RATE, F.CHANNEL_OFFSET          # 400 kS/s front-ends, 25 kS/s channels (decimation 16)
BLK = 16 * 1000
SYNC8 = dict(sync_word=0b10101100, sync_bits=8, sync_max_errors=2)          # loose enough to hit on any bits
READER = {"clock": "chan_read_clock", "costas": "chan_read_costas", "fsk4": "chan_read_fsk4"}


def _source(nat, kind):
    return {"clock": nat.READ_CLOCK, "costas": nat.READ_COSTAS, "fsk4": nat.READ_FSK4}[kind]


def _loop(fe, c, kind, cr=CR, baud=4800, agc_n=64):
    """the symbol loop `kind` (and the stage it reads) on channel c of rate 2 cr"""
    if kind == "fsk4":
        fe.chan_fm_filter(c, p25.fm_gain(cr), p25.symbol_taps(cr, baud))
        fe.chan_fsk4(c, **p25.fsk4_params(cr, baud))
    elif kind == "costas":
        fe.chan_agc(c, agc_n, 1.0)
        fe.chan_costas(c, **p25.costas_params(cr, baud))
    else:
        fe.chan_clock_mm(c, 2 * cr / 3600.0)


def _n_loop(fe, c, kind):
    return {"clock": lambda: fe.chan_clock_produced(c)[0], "costas": lambda: fe.chan_costas_state(c)["n_symbols"],
            "fsk4": lambda: fe.chan_fsk4_state(c)["n_symbols"]}[kind]()


def _slicer(nat, fe, c, kind, mode, **kw):
    fe.chan_slicer(c, _source(nat, kind), mode, **kw)


def _want(soft, mode, kw):
    return S.run(soft, mode, levels=kw.get("levels", S.LEVELS), sync_word=kw.get("sync_word", 0), sync_bits=kw.get("sync_bits", 0),
                 max_errors=kw.get("sync_max_errors", 0))


def _read(fe, c, kind):
    """(soft symbols, packed bytes, hit k, hit dist, state) of channel c, everything unread"""
    soft = getattr(fe, READER[kind])(c)
    by = fe.chan_read_hard(c)
    k, dist = fe.chan_read_sync(c)
    return soft, by, k, dist, fe.chan_slicer_state(c)


def _check(got, mode, kw, skip=0, what=""):
    """what _read gave against the restatement of the soft symbols from `skip` on -> the restatement"""
    soft, by, k, dist, st = got
    r = _want(soft[skip:], mode, kw)
    assert by.dtype == np.uint8 and k.dtype == np.int64 and dist.dtype == np.uint8
    assert st == dict(n_symbols=len(soft) - skip, n_words=len(r["words"]), n_hits=len(r["k"])), (what, st, len(soft), skip, len(r["words"]), len(r["k"]))
    assert np.array_equal(by, r["bytes"]), what                                   # the uint8 view: GNU Radio's byte stream
    assert np.array_equal(by.view("<u4"), r["words"]), what
    assert np.array_equal(k, r["k"]) and np.array_equal(dist, r["dist"]), (what, k[:8], r["k"][:8])
    return r


def _code(nat, fn, *a, **kw):
    with pytest.raises(nat.RcfError) as e:
        fn(*a, **kw)
    return e.value.code


def _noise(seed, n, amp=0.05):
    return (amp * synth.awgn(np.random.default_rng(seed), n)).astype(np.complex64)


# ------------------------------------------------------------------------------------------------ one channel per source kind
def test_c4fm_with_a_planted_frame_sync(gpu_required):
    nat = gpu_required
    rng = np.random.default_rng(4800)
    sent = rng.integers(0, 4, 1500).astype(np.uint8)
    sync = np.array([(p25.FRAME_SYNC >> (46 - 2 * i)) & 3 for i in range(24)], np.uint8)
    for at in (600, 800, 1000, 1200):
        sent[at:at + 24] = sync
    x = F.c4fm_carrier(sent, 4800, FS, OFF + 150.0, 0.5, 600.0)
    kw = dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=p25.FRAME_SYNC_MAX_ERRORS)
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True)
        for a in range(0, len(x), BLK):
            fe.push(x[a:a + BLK])
        got = _read(fe, c, "fsk4")
        assert fe.chan_slicer_rings(c)[1] == fe.chan_fsk4_ring(c)[1] and fe.chan_slicer_rings(c)[3] == 256
    r = _check(got, S.FSK4, kw, what="c4fm")
    assert abs(len(got[0]) - 1500) <= 2 and len(r["words"]) >= 92
    k = got[2]
    print("c4fm: %d symbols, hits at %s, distances %s" % (len(got[0]), k.tolist(), got[3].tolist()))
    assert len(k) >= 3 and np.all(np.diff(k) % 200 == 0)                          # the planted words, 200 dibits apart
    # the bytes at a hit are the word's, up to the hit's bit errors and the dibit phase of the window
    d = S.decisions(got[0], S.FSK4)
    assert int(np.count_nonzero(S.bits_of(d[k[0] - 23:k[0] + 1], S.FSK4) != S.bits_of(sync, S.FSK4))) == got[3][0]


def test_cqpsk_behind_the_gardner_costas_loop(gpu_required):
    nat = gpu_required
    x, _ = R.case_signal(*R.CASES[0])
    kw = dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=p25.FRAME_SYNC_MAX_ERRORS)
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        c = p25.cqpsk_demod(fe, fe.chan_open(CR, OFF), CR, R.CASES[0][0], hard=True)
        for a in range(0, len(x), BLK):
            fe.push(x[a:a + BLK])
        got = _read(fe, c, "costas")
    r = _check(got, S.FSK4, kw, what="cqpsk")
    assert len(got[0]) > 1000 and len(r["words"]) > 60


@pytest.mark.parametrize("system", ["smartnet", "edacs"])
def test_binary_behind_the_symbol_clock(gpu_required, system):
    nat = gpu_required
    rate, n_bits, setup, word, bits = {"smartnet": (3600.0, 1200, control.smartnet_clock, control.SMARTNET_SYNC, 8),
                                       "edacs": (9600.0, 3800, control.edacs_clock, control.EDACS_SYNC, 48)}[system]
    rng = np.random.default_rng(int(rate))
    sent = rng.integers(0, 2, n_bits)
    word_bits = [(word >> (bits - 1 - i)) & 1 for i in range(bits)]
    for at in (400, 700, 1000):
        sent[at:at + bits] = word_bits
    x = M.fsk2_carrier(sent, rate, 2.4e6, 150000.0, 1200.0, rng)
    with nat.Frontend(2.4e6, device=0, block_capacity=48000) as fe:
        c = fe.chan_open(12500, 150000.0)
        setup(fe, c, hard=True)
        for a in range(0, len(x), 48000):
            fe.push(x[a:a + 48000])
        got = _read(fe, c, "clock")
    _check(got, S.BINARY, dict(sync_word=word, sync_bits=bits), what=system)
    k = got[2]
    print("%s: %d symbols, hits at %s" % (system, len(got[0]), k.tolist()))
    assert abs(len(got[0]) - n_bits) <= 4
    ks = set(k.tolist())                                                          # (an 8-bit word also matches in the payload)
    assert sum(1 for a in ks if a + 300 in ks and a + 600 in ks) >= 1             # the three planted words, exact matches


# ------------------------------------------------------------------------------------------------ cuts
def test_words_and_hits_do_not_depend_on_the_cuts(gpu_required):
    nat = gpu_required
    x, _ = F.case_signal(*F.CASES[1])
    rng = np.random.default_rng(33)
    # ~110 pieces: random ones, pieces of less than one channel sample (the loop gets nothing: a block that gives 0), runs of
    # pieces of less than 16 symbols (83 channel samples), so that whole blocks end inside a word
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 45)}
    cuts |= {16 * 2000 + 5 * j for j in range(1, 14)} | {16 * 4100 + 3 + 16 * j for j in range(24)} | {16 * 6000 + 40 * 16 * j for j in range(24)}
    cuts = sorted(cuts)
    assert sum(b - a < 16 for a, b in zip(cuts[:-1], cuts[1:])) >= 10 and sum(b - a < 16 * 83 for a, b in zip(cuts[:-1], cuts[1:])) >= 50
    kw = dict(sync_word=0x2D, sync_bits=8, sync_max_errors=2)

    def run(pieces):
        with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
            c = fe.chan_open(CR, OFF)
            _loop(fe, c, "fsk4")
            _slicer(nat, fe, c, "fsk4", nat.SLICE_FSK4, **kw)
            for a, b in zip(pieces[:-1], pieces[1:]):
                fe.push(x[a:b])
            return _read(fe, c, "fsk4")

    one, ragged = run([0, len(x)]), run(cuts)
    r = _check(one, S.FSK4, kw, what="one push")
    _check(ragged, S.FSK4, kw, what="ragged pushes")
    assert one[0].tobytes() == ragged[0].tobytes() and one[1].tobytes() == ragged[1].tobytes()
    assert np.array_equal(one[2], ragged[2]) and np.array_equal(one[3], ragged[3]) and one[4] == ragged[4]
    assert len(r["words"]) >= 92 and len(r["k"]) > 20


# ------------------------------------------------------------------------------------------------ many channels, groups, mixed rates
def _kind_of(j):
    return ("fsk4", "costas", "clock")[j % 3]


def _mode_of(nat, j):
    """FSK4 behind the two P25 loops, binary behind the clock -- and the other way round on every seventh channel"""
    first = nat.SLICE_BINARY if _kind_of(j) == "clock" else nat.SLICE_FSK4
    return first if j % 7 else nat.SLICE_BINARY + nat.SLICE_FSK4 - first


def _kw_of(nat, j):
    return dict(SYNC8, hit_capacity=1024) if _mode_of(nat, j) == nat.SLICE_BINARY else dict(sync_word=0x2D6, sync_bits=10, sync_max_errors=3, hit_capacity=1024)


def test_130_channels_mixed_kinds_one_launch_per_block(gpu_required):
    nat = gpu_required
    blk, K = 4000, 6                                          # 250 channel samples a block
    x = _noise(130, blk * K)
    offs = [-190000.0 + 2900.0 * j for j in range(130)]
    late = {7: 2, 63: 2, 128: 2}                              # slicers attached in mid-stream
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [fe.chan_open(CR, f) for f in offs]
        for j, c in enumerate(cids):
            _loop(fe, c, _kind_of(j))
        fe.timing_enable(True, classes=[nat.T_SLICE])
        skip = {}
        for b in range(K):
            for j, c in enumerate(cids):
                if late.get(j, 0) == b:
                    skip[j] = _n_loop(fe, c, _kind_of(j))
                    _slicer(nat, fe, c, _kind_of(j), _mode_of(nat, j), **_kw_of(nat, j))
            fe.push(x[b * blk:(b + 1) * blk])
        assert fe.timing_read(nat.T_SLICE)[1] == K            # one launch per block carries all 130 (33 workgroups of 4 waves)
        got = [_read(fe, c, _kind_of(j)) for j, c in enumerate(cids)]
    n_hits = 0
    for j, g in enumerate(got):                               # lanes 0, 3, 4, 129 among them: workgroup boundaries at 4 channels
        assert (skip[j] > 0) == (j in late) and len(g[0]) - skip[j] > 80, (j, skip[j], len(g[0]))
        n_hits += len(_check(g, _mode_of(nat, j), _kw_of(nat, j), skip[j], ("lane", j))["k"])
    assert n_hits > 1000
    assert got[0][1].tobytes() != got[3][1].tobytes()


def _trio(nat, fe, offs):
    cids = [fe.chan_open(CR, f) for f in offs]
    for j, c in enumerate(cids):
        _loop(fe, c, _kind_of(j))
        _slicer(nat, fe, c, _kind_of(j), _mode_of(nat, j + 1), **_kw_of(nat, j + 1))
    return cids


def test_two_front_ends_in_a_group_share_the_launch(gpu_required):
    nat = gpu_required
    blk, K = 4000, 5
    xs = [_noise(20 + m, blk * K) for m in range(2)]
    offs = [(-100000.0, 60000.0, 150000.0), (30000.0, -150000.0, 90000.0)]
    fes = [nat.Frontend(FS, device=0, block_capacity=blk) for _ in range(2)]
    try:
        ids = [_trio(nat, fe, offs[m]) for m, fe in enumerate(fes)]
        fes[0].timing_enable(True, classes=[nat.T_SLICE])
        pairs = [(m, c) for m in range(2) for c in ids[m]]
        words, hits = [[] for _ in pairs], [[] for _ in pairs]
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * blk:(b + 1) * blk] for xm in xs])
                if b % 2:                                     # rcf_group_read_many: uint32 rows, the single readers' cursors
                    for rows, acc in ((g.read_many(pairs, "hard", cap_each=64), words), (g.read_many(pairs, "sync", cap_each=256), hits)):
                        assert all(row is not None and row.dtype == np.uint32 for row in rows)
                        for i, row in enumerate(rows):
                            acc[i].append(row)
            g.sync()
            assert fes[0].timing_read(nat.T_SLICE)[1] == K    # one launch per group block for both members
            grouped = [[_read(fe, c, _kind_of(j)) for j, c in enumerate(ids[m])] for m, fe in enumerate(fes)]
    finally:
        for fe in fes:
            fe.close()
    for m in range(2):
        with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
            cs = _trio(nat, fe, offs[m])
            for b in range(K):
                fe.push(xs[m][b * blk:(b + 1) * blk])
            for j, c in enumerate(cs):
                alone, grp = _read(fe, c, _kind_of(j)), grouped[m][j]
                r = _check(alone, _mode_of(nat, j + 1), _kw_of(nat, j + 1), what=("alone", m, j))
                i = 3 * m + j
                # what the group's batched reads took and what the single readers found afterwards: the whole stream, once
                assert np.concatenate(words[i] + [grp[1].view("<u4")]).tobytes() == alone[1].tobytes(), (m, j)
                k, dist = nat.widen_hits(np.concatenate(hits[i]), grp[4]["n_symbols"])
                assert np.array_equal(np.concatenate([k, grp[2]]), alone[2]) and np.array_equal(np.concatenate([dist, grp[3]]), alone[3])
                assert grp[0].tobytes() == alone[0].tobytes() and grp[4] == alone[4] and len(r["words"]) > 4


def test_mixed_rates_lanes_leave_the_chunk_loop_at_different_trips(gpu_required):
    """gc_ref.MIXED: 2.08 .. 16 samples per symbol on channels of 12.5, 25 and 50 kS/s: a block of 16000 inputs bounds the
    slicers' walks by 500, 1000 or 2000 inputs and gives them 60 .. 380 symbols"""
    nat = gpu_required
    x, _ = R.mixed_signal()
    kw = dict(sync_word=0x2D6, sync_bits=10, sync_max_errors=3, hit_capacity=4096)
    with nat.Frontend(FS, device=0, block_capacity=R.MIXED_BLK) as fe:
        cids = [fe.chan_open(row[0], row[2]) for row in R.MIXED]
        for c in cids:
            fe.chan_agc(c, R.MIXED_AGC_N, 1.0)
        fe.timing_enable(True, classes=[nat.T_SLICE])
        for b in range(R.MIXED_BLOCKS):
            for c, row in zip(cids, R.MIXED):
                if row[5] == b:
                    fe.chan_costas(c, **p25.costas_params(row[0], row[1]))
                    _slicer(nat, fe, c, "costas", nat.SLICE_FSK4, **kw)
            fe.push(x[b * R.MIXED_BLK:(b + 1) * R.MIXED_BLK])
        assert fe.timing_read(nat.T_SLICE)[1] == R.MIXED_BLOCKS
        got = [_read(fe, c, "costas") for c in cids]
    counts = [len(g[0]) for g in got]
    for j, g in enumerate(got):
        _check(g, S.FSK4, kw, what=("mixed", j))
    print("mixed rates: symbols per channel %s" % counts)
    assert min(counts) > 400 and max(counts) > 1400


# ------------------------------------------------------------------------------------------------ small rings
def test_word_ring_of_64_wraps_with_reads_between_pushes(gpu_required):
    nat = gpu_required
    x, _ = F.case_signal(*F.CASES[4])
    blk = 16 * 40                                             # 40 channel samples a block: ~10 symbols, less than a word
    kw = dict(sync_word=0x2D, sync_bits=8, sync_max_errors=2, hit_capacity=16)
    parts = []
    with nat.Frontend(FS, device=0, block_capacity=blk, out_capacity=64) as fe:
        c = fe.chan_open(CR, OFF)
        _loop(fe, c, "fsk4", baud=6000)
        _slicer(nat, fe, c, "fsk4", nat.SLICE_FSK4, **kw)
        assert fe.chan_slicer_rings(c)[1] == 64 and fe.chan_slicer_rings(c)[3] == 16
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk])
            parts.append(_read(fe, c, "fsk4"))
    soft, by, k, dist = (np.concatenate([p[j] for p in parts]) for j in range(4))
    r = _check((soft, by, k, dist, parts[-1][4]), S.FSK4, kw, what="ring of 64")
    assert len(r["words"]) > 64 + 25 and len(r["k"]) > 3 * 16 and max(len(p[1]) for p in parts) <= 8
    with nat.Frontend(FS, device=0, block_capacity=blk, out_capacity=32) as fe:
        c = fe.chan_open(CR, OFF)
        _loop(fe, c, "clock")
        assert _code(nat, _slicer, nat, fe, c, "clock", nat.SLICE_BINARY) == nat.RCF_ECAP


def test_word_ring_of_256_readers_left_behind_get_its_last_words(gpu_required):
    """out_capacity 256 and more than 256 words before anybody reads: the batched and the single reader of the word stream
    both return exactly the ring's last 256 words -- of the whole stream, which a third twin gives whose single reader
    comes after every block and never lags -- and go on block by block from there"""
    nat = gpu_required
    blk, K, cap = 16 * 150, 160, 256                          # 150 channel samples a block: ~29 dibits, under two words
    x = _noise(256, blk * (K + 2))

    def open_():
        fe = nat.Frontend(FS, device=0, block_capacity=blk, out_capacity=cap)
        c = fe.chan_open(CR, OFF)
        _loop(fe, c, "fsk4")
        _slicer(nat, fe, c, "fsk4", nat.SLICE_FSK4)
        return fe, c

    (fe, c), (tw, c_t), (al, c_a) = open_(), open_(), open_()
    whole = []
    try:
        at = 0
        for phase, n in enumerate((K, 1, 1)):
            before = len(whole)
            for _ in range(n):
                for f in (fe, tw, al):
                    f.push(x[at:at + blk])
                at += blk
                whole.extend(al.chan_read_hard(c_a).view("<u4").tolist())
            row = fe.chan_read_many([c], "hard", cap_each=2 * cap)[0]
            one = tw.chan_read_hard(c_t).view("<u4")
            assert al.chan_slicer_state(c_a)["n_words"] == len(whole)
            want = np.array(whole[-cap:] if phase == 0 else whole[before:], np.uint32)
            assert phase or len(whole) > cap + 16                 # more than a ring behind
            assert np.array_equal(row, want), (phase, len(row), len(want))
            assert np.array_equal(one, want), (phase, len(one), len(want))
        assert len(whole) > before                                # the last block brought words
    finally:
        for f in (fe, tw, al):
            f.close()


@pytest.mark.parametrize("max_errors", [2, 4])
def test_hit_ring_of_16_wraps_between_reads_and_the_oldest_go(gpu_required, max_errors):
    """sync_bits 8 on the bits of noise: at 2 errors a seventh of the symbols hit, at 4 two thirds -- more than the ring
    holds inside one chunk of 64 symbols.  A reader that comes every third block gets exactly the newest 16."""
    nat = gpu_required
    blk, K = 16000, 9
    x = _noise(16, blk * K)
    kw = dict(sync_word=0b10101100, sync_bits=8, sync_max_errors=max_errors, hit_capacity=16)
    soft, cursor, lost = np.zeros(0, np.float32), 0, 0
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = fe.chan_open(CR, OFF)
        _loop(fe, c, "clock")
        _slicer(nat, fe, c, "clock", nat.SLICE_BINARY, **kw)
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk])
            if b % 3 != 2:
                continue
            soft = np.concatenate([soft, fe.chan_read_clock(c)])
            r = _want(soft, S.BINARY, kw)
            n = len(r["k"])
            assert fe.chan_slicer_state(c) == dict(n_symbols=len(soft), n_words=len(soft) // 32, n_hits=n)
            k, dist = fe.chan_read_sync(c)
            first = max(cursor, n - 16)
            assert n - cursor > 16 and np.array_equal(k, r["k"][first:n]) and np.array_equal(dist, r["dist"][first:n]), (b, n, cursor, k)
            lost += first - cursor
            cursor = n
            assert len(fe.chan_read_sync(c)[0]) == 0
    assert lost > 30


# ------------------------------------------------------------------------------------------------ attach in mid-stream
def test_attach_in_mid_stream_starts_at_the_loops_next_symbol(gpu_required):
    nat = gpu_required
    blk, K = 4000, 5
    x = _noise(5, blk * K)
    every = dict(sync_word=0xA5, sync_bits=8, sync_max_errors=7, hit_capacity=4096)        # every complete window but 0x5A is a hit
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cs = {kind: fe.chan_open(CR, off) for kind, off in (("costas", -50000.0), ("clock", 50000.0))}
        for kind, c in cs.items():
            _loop(fe, c, kind)
        fe.push(x[:blk])
        fe.push(x[blk:2 * blk])
        n0 = {kind: _n_loop(fe, c, kind) for kind, c in cs.items()}
        _slicer(nat, fe, cs["costas"], "costas", nat.SLICE_FSK4, **every)
        _slicer(nat, fe, cs["clock"], "clock", nat.SLICE_BINARY, **every)
        for c in cs.values():
            assert fe.chan_slicer_state(c) == dict(n_symbols=0, n_words=0, n_hits=0)
        for b in range(2, K):
            fe.push(x[b * blk:(b + 1) * blk])
        got = {kind: _read(fe, c, kind) for kind, c in cs.items()}
    for kind, mode, L in (("costas", S.FSK4, 4), ("clock", S.BINARY, 8)):
        g = got[kind]
        assert n0[kind] > 50
        _check(g, mode, every, n0[kind], kind)                # k = 0 is the loop's symbol n0: the first after the call
        n = len(g[0]) - n0[kind]
        # the first window completes at k = L - 1 (sought in a stream whose first windows are not the word's complement)
        assert n > 100 and g[2][0] == L - 1 and g[2][-1] == n - 1 and n - (L - 1) - 4 <= len(g[2]) <= n - (L - 1)


# ------------------------------------------------------------------------------------------------ poisoned input
def test_nan_soft_symbols_slice_by_the_rule_and_the_neighbour_never_notices(gpu_required):
    """the C4FM loop's input made NaN for one block through the symbol filter (tests/test_gpu_fsk4.py's poisoned case): its
    soft symbols of that block are NaN and slice to dibit 1; a clean channel of the same launches is what it is alone"""
    nat = gpu_required
    n = BLK * 7
    x = np.zeros(n, dtype=np.complex64)
    for case, off in ((F.CASES[1], -150000.0), (F.CASES[2], 150000.0)):
        x = x + 0.4 * F.case_signal(*case, offset=off, n_symbols=2500)[0][:n]
    x = x.astype(np.complex64)
    kw = dict(sync_word=0x55, sync_bits=8, sync_max_errors=1)                     # 01 01 01 01: four NaN symbols in a row hit

    def run(only=None):
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            cids = {}
            for j, off in enumerate((-150000.0, 150000.0)):
                if only in (None, j):
                    c = cids[j] = fe.chan_open(CR, off)
                    _loop(fe, c, "fsk4")
                    _slicer(nat, fe, c, "fsk4", nat.SLICE_FSK4, **kw)
            for b in range(n // BLK):
                if 0 in cids and b in (3, 4):
                    fe.chan_fm_filter(cids[0], p25.fm_gain(CR), [float("nan")] * 5 if b == 3 else p25.symbol_taps(CR))
                fe.push(x[b * BLK:(b + 1) * BLK])
            return {j: _read(fe, c, "fsk4") for j, c in cids.items()}

    got, alone = run(), run(only=1)
    bad = np.flatnonzero(np.isnan(got[0][0]))
    assert len(bad) > 120 and np.isfinite(got[1][0]).all()
    r = _check(got[0], S.FSK4, kw, what="poisoned")
    assert np.all(S.decisions(got[0][0], S.FSK4)[bad] == 1)
    run_of_nan = bad[np.flatnonzero(np.diff(bad) == 1)[:40]]                      # inside a run of NaN symbols every window is 0x55
    assert len(run_of_nan) == 40 and set(run_of_nan[8:].tolist()) <= set(r["k"][r["dist"] == 0].tolist())
    _check(got[1], S.FSK4, kw, what="clean")
    for a, b in zip(got[1], alone[1]):
        assert (a == b) if isinstance(a, dict) else (a.tobytes() == b.tobytes())


# ------------------------------------------------------------------------------------------------ batched readers
def test_read_many_over_64_channels_interleaves_with_the_single_readers(gpu_required):
    nat = gpu_required
    blk, K = 8000, 6
    x = _noise(64, blk * K)
    offs = [-190000.0 + 5900.0 * j for j in range(64)]
    kw = dict(SYNC8, hit_capacity=64)

    def open_():
        fe = nat.Frontend(FS, device=0, block_capacity=blk)
        cids = [fe.chan_open(CR, f) for f in offs]
        for c in cids:
            _loop(fe, c, "clock")
            _slicer(nat, fe, c, "clock", nat.SLICE_BINARY, **kw)
        return fe, cids

    fe, cids = open_()
    tw, cids_t = open_()
    bare = fe.chan_open(CR, 195000.0)                         # no slicer
    lst = cids + [bare, 9999, cids[5]]
    words, hits = [[] for _ in cids], [[] for _ in cids]
    want_w, want_h = [[] for _ in cids], [[] for _ in cids]
    try:
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk])
            tw.push(x[b * blk:(b + 1) * blk])
            for what, acc, cap in (("hard", words, 2), ("sync", hits, 5)):    # small rows: several passes per block
                for it in range(100):
                    rows = fe.chan_read_many(lst, what, cap_each=cap)
                    assert rows[64] is None and rows[65] is None and rows[66] is None     # RCF_ESTATE, RCF_ENOCHAN, listed twice
                    assert all(row.dtype == np.uint32 and len(row) <= cap for row in rows[:64])
                    for j in range(64):
                        acc[j].append(rows[j].copy())
                    # single readers in between, on two of the channels
                    one = fe.chan_read_hard(cids[1], 1).view("<u4") if what == "hard" else \
                        S.hit_items(*fe.chan_read_sync(cids[1], 3))
                    acc[1].append(one)
                    if not any(len(row) for row in rows[:64]) and not len(one):
                        break
                assert it < 99
            for j, c in enumerate(cids_t):
                want_w[j].append(tw.chan_read_hard(c).view("<u4"))
                want_h[j].append(S.hit_items(*tw.chan_read_sync(c)))
        total = 0
        for j in range(64):                                   # nothing lost, nothing twice
            assert np.array_equal(np.concatenate(words[j]), np.concatenate(want_w[j])), j
            assert np.array_equal(np.concatenate(hits[j]), np.concatenate(want_h[j])), j
            assert fe.chan_slicer_state(cids[j]) == tw.chan_slicer_state(cids_t[j])
            total += len(np.concatenate(hits[j]))
        assert total > 64 * 30 and len(np.concatenate(want_w[0])) >= 8
    finally:
        fe.close()
        tw.close()


# ------------------------------------------------------------------------------------------------ lifecycle and refusals
def test_lifecycle(gpu_required):
    nat = gpu_required
    blk, K = 4000, 9
    x = _noise(8, blk * K)
    kw = dict(sync_word=0x2D, sync_bits=8, sync_max_errors=2, hit_capacity=4096)
    streams = ("chan_read_iq", "chan_read_sym", "chan_read_agc", "chan_read_clock", "chan_read_fsk4")

    def everything(fe, c):
        return [getattr(fe, f)(c) for f in streams] + [fe.chan_read_fm(c, 5.0)]

    def setup(fe):
        c = fe.chan_open(CR, OFF)
        for kind in ("fsk4", "costas", "clock"):
            _loop(fe, c, kind)
        return c

    with nat.Frontend(FS, device=0, block_capacity=blk) as fe, nat.Frontend(FS, device=0, block_capacity=blk) as tw:
        c, ct = setup(fe), setup(tw)                          # tw: the same channel without the stage, ever
        plain = fe.chan_open(CR, -OFF)                        # ... and a channel of fe without it
        plain_t = tw.chan_open(CR, -OFF)
        for f in (fe.chan_read_hard, fe.chan_read_sync, fe.chan_slicer_state, fe.chan_slicer_rings):
            assert _code(nat, f, c) == nat.RCF_ESTATE
        _slicer(nat, fe, c, "fsk4", nat.SLICE_FSK4, **kw)
        for b in range(2):
            fe.push(x[b * blk:(b + 1) * blk])
            tw.push(x[b * blk:(b + 1) * blk])
        fe.chan_set_offset(c, OFF + 20.0)                     # a retune keeps it
        tw.chan_set_offset(ct, OFF + 20.0)
        fe.push(x[2 * blk:3 * blk])
        tw.push(x[2 * blk:3 * blk])
        first = _read(fe, c, "fsk4")
        tw.chan_read_fsk4(ct)
        _check(first, S.FSK4, kw, what="across a retune")
        assert first[4]["n_symbols"] > 100
        # a second call starts it afresh, behind another loop: k = 0 at that loop's next symbol
        n0 = _n_loop(fe, c, "clock")
        fe.chan_read_clock(c)
        tw.chan_read_clock(ct)
        _slicer(nat, fe, c, "clock", nat.SLICE_BINARY, **SYNC8)
        assert fe.chan_slicer_state(c) == dict(n_symbols=0, n_words=0, n_hits=0) and n0 > 60
        fe.push(x[3 * blk:4 * blk])
        tw.push(x[3 * blk:4 * blk])
        _check(_read(fe, c, "clock"), S.BINARY, SYNC8, what="behind the clock")
        tw.chan_read_clock(ct)
        # off and on
        fe.chan_slicer(c, None)
        fe.chan_slicer(c, None)                               # off twice: nothing to do
        for f in (fe.chan_read_hard, fe.chan_read_sync, fe.chan_slicer_state, fe.chan_slicer_rings):
            assert _code(nat, f, c) == nat.RCF_ESTATE
        assert fe.chan_read_many([c], "hard", cap_each=8) == [None]
        fe.push(x[4 * blk:5 * blk])
        tw.push(x[4 * blk:5 * blk])
        fe.chan_read_costas(c)
        tw.chan_read_costas(ct)
        _slicer(nat, fe, c, "costas", nat.SLICE_FSK4, **kw)
        fe.push(x[5 * blk:6 * blk])
        tw.push(x[5 * blk:6 * blk])
        got = _read(fe, c, "costas")
        _check(got, S.FSK4, kw, what="on again")
        assert got[4]["n_symbols"] > 30
        tw.chan_read_costas(ct)
        # attaching the source loop again detaches the slicer; so does switching it off; another loop's restart does not
        fe.chan_clock_mm(c, 2 * CR / 3600.0)
        tw.chan_clock_mm(ct, 2 * CR / 3600.0)
        assert fe.chan_slicer_state(c)["n_symbols"] == got[4]["n_symbols"]
        fe.chan_costas(c, **p25.costas_params(CR, 4800))
        tw.chan_costas(ct, **p25.costas_params(CR, 4800))
        assert _code(nat, fe.chan_slicer_state, c) == nat.RCF_ESTATE
        _slicer(nat, fe, c, "costas", nat.SLICE_FSK4, **kw)
        fe.chan_costas(c, None)
        tw.chan_costas(ct, None)
        assert _code(nat, fe.chan_read_hard, c) == nat.RCF_ESTATE
        assert _code(nat, _slicer, nat, fe, c, "costas", nat.SLICE_FSK4, **kw) == nat.RCF_ESTATE
        _slicer(nat, fe, c, "fsk4", nat.SLICE_FSK4, **kw)
        fe.chan_read_fsk4(c)
        tw.chan_read_fsk4(ct)
        skip = fe.chan_fsk4_state(c)["n_symbols"]
        fe.push(x[6 * blk:7 * blk])
        tw.push(x[6 * blk:7 * blk])
        g = _read(fe, c, "fsk4")
        _check(g, S.FSK4, kw, what="behind the C4FM loop again")
        assert skip > 200 and g[4]["n_symbols"] > 30
        tw.chan_read_fsk4(ct)
        fe.push(x[7 * blk:8 * blk])
        tw.push(x[7 * blk:8 * blk])
        # every other stream of the channel WITH the stage, and the channel without it, read as on the twin
        for a, b in zip(everything(fe, c) + [fe.chan_read_iq(plain)], everything(tw, ct) + [tw.chan_read_iq(plain_t)]):
            assert a.tobytes() == b.tobytes() and len(a) > 30
        assert fe.chan_read_many([plain], "sync", cap_each=8) == [None]
        fe.chan_close(c)                                      # closed with the stage attached
        assert _code(nat, fe.chan_read_hard, c) == nat.RCF_ENOCHAN
        fe.push(x[8 * blk:])
        assert len(fe.chan_read_iq(plain)) == 250


def test_refusals(gpu_required):
    nat = gpu_required
    lib = nat.lib()
    nan, inf = float("nan"), float("inf")
    blk = 1600
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = fe.chan_open(CR, OFF)
        _loop(fe, c, "clock")
        ok = dict(sync_word=0x2D, sync_bits=8, sync_max_errors=2)
        B, Q = nat.SLICE_BINARY, nat.SLICE_FSK4
        src = nat.READ_CLOCK
        for source in (nat.READ_SYM, nat.READ_AUDIO, nat.READ_FM, nat.HARD_BITS, 5, -1):
            assert _code(nat, fe.chan_slicer, c, source, B, **ok) == nat.RCF_EINVAL, source
        for mode in (0, 3, -1):
            assert _code(nat, fe.chan_slicer, c, src, mode, **ok) == nat.RCF_EINVAL, mode
        for levels in ((nan, 0, 2, 4), (-2, 0, inf, 4), (-2, 0, 2, -inf), (0, -2, 2, 4), (-2, 0, 2, 1)):
            assert _code(nat, fe.chan_slicer, c, src, Q, levels=levels, **ok) == nat.RCF_EINVAL, levels
        fe.chan_slicer(c, src, B, levels=(nan, 3, 2, 1), **ok)                   # the levels are the FSK4 mode's alone
        fe.chan_slicer(c, src, Q, levels=(0, 0, 0, 0), **ok)                     # non-decreasing
        for mode, bits in ((B, 7), (B, 65), (B, -8), (B, 4), (Q, 9), (Q, 63), (Q, 6), (Q, 66)):
            assert _code(nat, fe.chan_slicer, c, src, mode, **dict(ok, sync_bits=bits)) == nat.RCF_EINVAL, (mode, bits)
        for bits, err in ((8, -1), (8, 8), (48, 48), (64, 64), (0, 1)):
            assert _code(nat, fe.chan_slicer, c, src, B, sync_word=1, sync_bits=bits, sync_max_errors=err) == nat.RCF_EINVAL, (bits, err)
        for cap in (8, 15, 24, -16, (1 << 27)):
            assert _code(nat, fe.chan_slicer, c, src, B, hit_capacity=cap, **ok) == nat.RCF_EINVAL, cap
        for good in (dict(sync_bits=64, sync_max_errors=63, sync_word=(1 << 64) - 1), dict(sync_bits=0), dict(ok, hit_capacity=16),
                     dict(sync_bits=8, sync_max_errors=7, sync_word=0x1FF)):
            fe.chan_slicer(c, src, B, **good)
        fe.chan_slicer(c, src, Q, sync_bits=64, sync_max_errors=63, sync_word=5)
        assert _code(nat, fe.chan_slicer, 999, src, B, **ok) == nat.RCF_ENOCHAN
        for f in (fe.chan_read_hard, fe.chan_read_sync, fe.chan_slicer_state, fe.chan_slicer_rings):
            assert _code(nat, f, 999) == nat.RCF_ENOCHAN
        for source in (nat.READ_COSTAS, nat.READ_FSK4):                          # loops the channel does not carry
            assert _code(nat, fe.chan_slicer, c, source, Q, **ok) == nat.RCF_ESTATE
        # the raw batched ABI: 32 and 33 are streams, uint32 rows
        cid, cnt = (ctypes.c_int * 1)(c), (ctypes.c_int64 * 1)()
        buf = np.zeros(64, dtype=np.uint32)
        for what in (nat.HARD_BITS, nat.HARD_SYNC):
            assert lib.rcf_chan_read_many(fe._h, what, cid, 1, 7.0, buf.ctypes.data_as(ctypes.c_void_p), 16, cnt) == nat.RCF_OK and cnt[0] == 0
        for what in (31, 34):
            assert lib.rcf_chan_read_many(fe._h, what, cid, 1, 1.0, buf.ctypes.data_as(ctypes.c_void_p), 16, cnt) == nat.RCF_EINVAL
        # the pump delivers neither (the follow-up): refused at start and at subscribe, as 3 is
        ring = nat.PinnedArray(2 * 2 * blk, np.uint8)
        ring.array[:] = 127
        counter = np.zeros(1, dtype=np.uint64)
        grp = nat.Group([fe])
        try:
            for what in ("hard", "sync"):
                assert _code(nat, nat.Pump, grp, [ring], blk, FS, (), fmt=nat.FMT_U8, what=what, max_read=4, written=[counter],
                             start_delay_s=0.0) == nat.RCF_EINVAL
            pump = nat.Pump(grp, [ring], blk, FS, (), fmt=nat.FMT_U8, what="clock", max_read=4, written=[counter], start_delay_s=0.0)
            cur = ctypes.c_int64(0)
            for what in (nat.HARD_BITS, nat.HARD_SYNC, 3):
                assert lib.rcf_pump_subscribe(pump._p, 0, c, what, 1.0, ctypes.byref(cur)) == nat.RCF_EINVAL, what
            assert lib.rcf_pump_subscribe(pump._p, 0, c, nat.READ_CLOCK, 1.0, ctypes.byref(cur)) >= 0
            pump.stop()
        finally:
            grp.close()
            ring.free()
