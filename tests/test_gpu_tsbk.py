"""P25 trunking blocks on the GPU (rcf_chan_tsbk; tsbk.hip): frames from the slicer's sync hits, status symbols, NID,
deinterleave, rate-1/2 trellis and CRC behind a channel's slicer.  include/rcf.h defines the stage, tests/tsbk_ref.py restates
it in numpy.  The yardstick is always that restatement applied to the channel's OWN packed words and sync hits as the
slicer's readers deliver them (chan_read_hard / chan_read_sync): the stage is integer work on those two streams, so every
comparison -- records, counters -- is of bits.  Where a case needs many frames on many channels it loosens the slicer's
sync search until the bits of noise hit: a frame is whatever follows a hit."""
import numpy as np
import pytest

import fsk4_ref as F
import tsbk_ref as T
from rcf import p25, synth

pytestmark = pytest.mark.gpu

FS, CR, OFF = F.FS, F.CHANNEL_RATE, F.CHANNEL_OFFSET          # 400 kS/s front-ends, 25 kS/s channels (decimation 16)
BLK = 16 * 1000
NAC = 0x293
STRICT = dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=p25.FRAME_SYNC_MAX_ERRORS)
# a search so loose that every window hits: a frame every 24 dibits, all of them frame records
EVERY = dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=47, hit_capacity=4096)


def _loose(kind):
    """a search loose enough that a few in a hundred of noise's dibits hit.  Behind the C4FM loop noise leans towards the sync
    word (its dibits are mostly 1 and 3, as the word's are: about 19 of 48 bits differ on average), behind the Gardner /
    Costas loop its bits are even (24 of 48)"""
    return dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=13 if kind == "fsk4" else 17, hit_capacity=4096)


LOOSE = _loose("fsk4")


def _shift(x0, f):
    return (x0 * np.exp(2j * np.pi * f / FS * np.arange(len(x0)))).astype(np.complex64)


def _noise(seed, n, amp=0.05):
    return (amp * synth.awgn(np.random.default_rng(seed), n)).astype(np.complex64)


def _code(nat, fn, *a, **kw):
    with pytest.raises(nat.RcfError) as e:
        fn(*a, **kw)
    return e.value.code


def tsdu_dibits():
    """1000 dibits for the loop to settle, three back-to-back 360-dibit TSDUs, a 180-, a 288- and a 360-dibit one, a data
    unit with DUID 5, and a tail -> (the dibits, the TSBKs sent per TSDU, the frames' starts)"""
    rng = np.random.default_rng(25)
    sent, starts = [], []
    d = [rng.integers(0, 4, 1000).astype(np.uint8)]
    at = 1000
    for n in (3, 3, 3, 1, 2, 3):
        tsbks = [T.tsbk_octets(rng) for _ in range(n)]
        f = T.frame(NAC, 7, tsbks, rng)
        sent.append(tsbks); starts.append(at); d.append(f)
        at += len(f)
    d.append(rng.integers(0, 4, 50).astype(np.uint8))
    starts.append(at + 50)
    d.append(T.frame(NAC, 5, [], rng, total=360))
    d.append(rng.integers(0, 4, 480).astype(np.uint8))
    return np.concatenate(d), sent, starts


@pytest.fixture(scope="module")
def tsdu():
    """tsdu_dibits as one 4800-baud C4FM carrier at baseband, 150 Hz off -> (x, the TSBKs sent per TSDU, the frames' starts)"""
    d, sent, starts = tsdu_dibits()
    return F.c4fm_carrier(d, 4800, FS, 150.0, 0.5, 600.0), sent, starts


def _want(fe, c, **kw):
    """the restatement over everything the slicer's two readers deliver (the whole streams: nobody has read them before)"""
    by = fe.chan_read_hard(c)
    k, dist = fe.chan_read_sync(c)
    return T.run(by, k, dist, **kw)


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, len(got), len(want), got[:4], want[:4])


def _run_tsdu(nat, x, pieces, attach_at=None):
    """the TSDU carrier pushed in pieces -> (records, state, restatement's records, its state, n_hits at the attach)"""
    with nat.Frontend(FS, device=0, block_capacity=max(b - a for a, b in zip(pieces[:-1], pieces[1:]))) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, tsbk=attach_at is None)
        first = 0
        for a, b in zip(pieces[:-1], pieces[1:]):
            if attach_at is not None and a == attach_at:
                first = fe.chan_slicer_state(c)["n_hits"]
                fe.chan_tsbk(c)
            fe.push(x[a:b])
        recs, st = fe.chan_read_tsbk(c), fe.chan_tsbk_state(c)
        assert len(fe.chan_read_tsbk(c)) == 0
        want, want_st = _want(fe, c, first_hit=first)
    return recs, st, want, want_st, first


# ------------------------------------------------------------------------------------------------ one channel, real frames
def test_every_sent_tsbk_is_recovered_and_records_equal_the_restatement(gpu_required, tsdu):
    nat = gpu_required
    x, sent, starts = tsdu
    x = _shift(x, OFF)
    recs, st, want, want_st, _ = _run_tsdu(nat, x, list(range(0, len(x), BLK)) + [len(x)])
    _same(recs, want, "one channel")
    assert st == want_st and st["n_lost"] == 0
    frames = [f for f in p25.tsdu_frames(recs) if f["nac"] == NAC]
    print("tsdu: %d records, frames %s, state %s" % (len(recs), [(f["k"], f["duid"], f["frame_dibits"], len(f["tsbk"])) for f in frames], st))
    assert [f["frame_dibits"] for f in frames] == [360, 360, 360, 180, 288, 360, 360] and [f["duid"] for f in frames] == [7] * 6 + [5]
    assert np.all(np.diff([f["k"] for f in frames][:6]) == [360, 360, 360, 180, 288]) and any((f["k"] - 23) % 16 for f in frames)
    for f, tsbks in zip(frames, sent):                              # every sent TSBK, with a good CRC
        assert [t["octets"] for t in f["tsbk"]] == tsbks and not any(t["crc"] for t in f["tsbk"])
    assert frames[6]["tsbk"] == [] and st["n_blocks"] >= 15 and st["n_frames"] >= 7           # the DUID-5 unit: a frame record
    ref = [f for f in p25.tsdu_frames(recs, reference_rule=True) if f["nac"] == NAC]
    for f, r in zip(frames, ref):                                   # what procTSDU would list: up to the first block followed by a 1
        stop = next((i for i, t in enumerate(f["tsbk"]) if t["next_bit"]), len(f["tsbk"]) - 1)
        assert r["tsbk"] == f["tsbk"][:stop + 1]
    assert sum(len(r["tsbk"]) for r in ref) < sum(len(f["tsbk"]) for f in frames)


def test_records_do_not_depend_on_the_cuts(gpu_required, tsdu):
    nat = gpu_required
    x = _shift(tsdu[0], OFF)
    rng = np.random.default_rng(34)
    # random pieces, pieces of less than one channel sample (a block of 0 symbols), runs of pieces of one symbol (83 samples)
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 40)}
    cuts |= {16 * 4000 + 5 * j for j in range(1, 14)} | {16 * 6000 + 84 * j for j in range(40)} | {16 * 9000 + 16 * 30 * j for j in range(20)}
    cuts = sorted(cuts)
    one = _run_tsdu(nat, x, [0, len(x)])
    ragged = _run_tsdu(nat, x, cuts)
    _same(one[0], one[2], "one push"); _same(ragged[0], ragged[2], "ragged pushes")
    _same(ragged[0], one[0], "cuts")
    assert one[1] == one[3] == ragged[1] == ragged[3] and one[1]["n_blocks"] >= 15


def test_attach_in_mid_frame_that_frame_does_not_appear(gpu_required, tsdu):
    nat = gpu_required
    x, sent, starts = tsdu
    x = _shift(x, OFF)
    sps = FS / 4800.0
    attach = int((starts[1] + 100) * sps) // 16 * 16                # inside the second TSDU, behind its sync word
    recs, st, want, want_st, first = _run_tsdu(nat, x, [0, attach, len(x)], attach_at=attach)
    _same(recs, want, "late attach")
    assert st == want_st and first >= 1
    frames = [f for f in p25.tsdu_frames(recs) if f["nac"] == NAC]
    assert [[t["octets"] for t in f["tsbk"]] for f in frames[:4]] == sent[2:]                # the third TSDU is the first to appear
    assert len(frames) == 5


def test_a_second_sync_10_dibits_behind_a_first_is_not_accepted(gpu_required):
    nat = gpu_required
    rng = np.random.default_rng(10)
    sync = np.array(T.SYNC_DIBITS, np.uint8)
    bits = lambda d: np.stack([(d >> 1) & 1, d & 1], axis=1).reshape(-1)
    both = np.concatenate([sync, sync[14:]])                        # a window that ends 10 dibits behind the word's
    errors = int(np.count_nonzero(bits(both[10:]) != bits(sync)))
    assert 4 < errors < 24
    f = T.frame(NAC, 7, [T.tsbk_octets(rng) for _ in range(3)], rng)
    f[24:34] = sync[14:]                                            # (over the NID's first dibits)
    d = np.concatenate([rng.integers(0, 4, 1000).astype(np.uint8), f, rng.integers(0, 4, 500).astype(np.uint8)])   # (1000 dibits: the loop has settled)
    x = F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0)
    with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800)
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=errors)
        fe.chan_tsbk(c)
        fe.push(x)
        recs, st = fe.chan_read_tsbk(c), fe.chan_tsbk_state(c)
        by = fe.chan_read_hard(c)
        k, dist = fe.chan_read_sync(c)
    want, want_st = T.run(by, k, dist)
    _same(recs, want, "second sync")
    exact = k[dist == 0]
    assert st == want_st and len(exact) == 1 and int(exact[0]) + 10 in k.tolist()             # both hit
    ks = set(recs["k"].tolist())
    assert int(exact[0]) in ks and int(exact[0]) + 10 not in ks


# ------------------------------------------------------------------------------------------------ designed errors
def test_designed_carrier_of_wrong_blocks_walks_every_correcting_path(gpu_required):
    """T.designed_dibits as a noise-free C4FM carrier under the strict search: 50 TSDUs with DUID 7 whose 147 blocks are random
    dibits (30 frames) or valid TSBKs with 1 .. 4 wrong dibits, every code word 0 .. 48 damaged in some block, a 180- and a
    288-dibit frame among them.  Records and counters are the restatement's over the channel's own words and hits; and the
    census over those delivered streams says that the kernel's scan, its n_inexact ballot and its CRC reduction met what the
    input was built for: all 64 (state, code word) pairs, an inexact word at every lane, every lane entered from all four
    states, n_inexact >= 32, bad and good CRCs.  tests/test_tsbk_cpu.py holds the same census on the planted dibits."""
    nat = gpu_required
    d, starts = T.designed_dibits(NAC)
    x = F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0)
    blk = 4 * BLK
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, tsbk=True)
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk])
        recs, st = fe.chan_read_tsbk(c), fe.chan_tsbk_state(c)
        by = fe.chan_read_hard(c)
        k, dist = fe.chan_read_sync(c)
    blocks = []
    want, want_st = T.run(by, k, dist, blocks=blocks)
    census = T.census(blocks, want_st)
    f = nat.tsbk_fields(recs)
    print("designed: %d hits, %s; census: %d pairs, %d lanes inexact, n_inexact up to %d (device: %d), %d good CRCs" % (
        len(k), st, len(census["pairs"]), len(census["inexact_lanes"]), census["max_inexact"], int(f["n_inexact"].max()), census["n_crc_good"]))
    _same(recs, want, "designed")
    assert st == want_st and st["n_lost"] == 0
    # the planted frames, all of them, at distance 0 and where they were put (the loop's delay moves them all alike)
    assert len(k) == len(starts) and not np.any(dist) and np.diff(k).tolist() == np.diff(starts).tolist()
    frames = p25.tsdu_frames(recs)
    assert [fr["frame_dibits"] for fr in frames] == T.DESIGNED_FRAME_DIBITS and all(fr["duid"] == 7 and fr["nac"] == NAC for fr in frames)
    assert st["n_frames"] == 50 and st["n_blocks"] == len(blocks) == 147
    T.check_census(census)
    assert int(f["n_inexact"].max()) == census["max_inexact"] and st["n_crc_bad"] == census["n_crc_bad"] == int(np.sum(f["crc_bad"]))
    assert not any(t["crc"] or t["n_inexact"] for t in frames[-1]["tsbk"])       # the last frame is clean


# ------------------------------------------------------------------------------------------------ many channels, groups
def _kind_of(j):
    return "costas" if j % 3 == 1 else "fsk4"


def _open_loose(nat, fe, f, j, tsbk=True, capacity=0, search=None):
    """channel j at offset f: a P25 loop (6000 baud on every fourth), the slicer with a loose search, the stage"""
    baud = 6000 if j % 4 == 3 else 4800
    c = fe.chan_open(CR, f)
    if _kind_of(j) == "fsk4":
        fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, baud))
        fe.chan_fsk4(c, **p25.fsk4_params(CR, baud))
    else:
        fe.chan_agc(c, 64, 1.0)
        fe.chan_costas(c, **p25.costas_params(CR, baud))
    fe.chan_slicer(c, nat.READ_FSK4 if _kind_of(j) == "fsk4" else nat.READ_COSTAS, nat.SLICE_FSK4, **(search or _loose(_kind_of(j))))
    if tsbk:
        fe.chan_tsbk(c, capacity)
    return c


def test_130_channels_one_launch_behind_the_slicers(gpu_required, tsdu):
    """noise, and the TSDU carrier under every twelfth channel (C4FM loops at 4800 baud, 34.8 kHz apart), which search strictly;
    the others search the noise -- and their neighbours' carriers -- loosely"""
    nat = gpu_required
    blk = 16000                                                   # 1000 channel samples a block: 192 or 240 symbols
    x0, sent, _ = tsdu
    K = (len(x0) + blk - 1) // blk
    offs = [-190000.0 + 2900.0 * j for j in range(130)]
    real = set(range(0, 130, 12))
    x0 = np.concatenate([x0, np.zeros(K * blk - len(x0), np.complex64)])
    x = _noise(131, blk * K)
    for j in real:
        x = x + 0.2 * _shift(x0, offs[j])
    bare = {2, 64, 129}                                           # a slicer but no TSBK stage
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [_open_loose(nat, fe, f, j, tsbk=j not in bare, search=STRICT if j in real else None) for j, f in enumerate(offs)]
        fe.timing_enable(True, classes=[nat.T_SLICE])
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk])
        assert fe.timing_read(nat.T_SLICE)[1] == 2 * K            # the slicers' launch and the stages' behind it, 33 workgroups each
        n_rec = n_blk = 0
        n_good = []
        for j, c in enumerate(cids):
            if j in bare:
                assert _code(nat, fe.chan_read_tsbk, c) == nat.RCF_ESTATE and _code(nat, fe.chan_tsbk_state, c) == nat.RCF_ESTATE
                continue
            recs, st = fe.chan_read_tsbk(c), fe.chan_tsbk_state(c)
            want, want_st = _want(fe, c)
            _same(recs, want, ("lane", j))
            assert st == want_st and st["n_lost"] == 0, (j, st, want_st)
            n_rec += len(recs); n_blk += st["n_blocks"]
            if j in real:
                # under noise and ten other carriers a symbol error may cost a block (the clean channel above recovers all):
                # what has a good CRC is a sent TSBK, in the order sent, and each of the eleven channels brings some
                good = [t["octets"] for f in p25.tsdu_frames(recs) if f["nac"] == NAC for t in f["tsbk"] if not t["crc"]]
                every = [t for tsbks in sent for t in tsbks]
                assert good and [t for t in every if t in good] == good, (j, len(good))
                n_good.append(len(good))
    print("130 channels: %d records, %d blocks; good TSBKs of 15 sent on the carriers' channels: %s" % (n_rec, n_blk, n_good))
    assert n_rec > 130 and n_blk >= sum(n_good)


def test_two_front_ends_in_a_group_share_the_launch(gpu_required):
    nat = gpu_required
    blk, K = 16000, 5
    xs = [_noise(40 + m, blk * K) for m in range(2)]
    offs = [(-100000.0, 60000.0, 150000.0), (30000.0, -150000.0, 90000.0)]
    fes = [nat.Frontend(FS, device=0, block_capacity=blk) for _ in range(2)]
    try:
        ids = [[_open_loose(nat, fe, f, j) for j, f in enumerate(offs[m])] for m, fe in enumerate(fes)]
        fes[0].timing_enable(True, classes=[nat.T_SLICE])
        pairs = [(m, c) for m in range(2) for c in ids[m]]
        taken = [[] for _ in pairs]
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * blk:(b + 1) * blk] for xm in xs])
                if b >= 2:                                        # rcf_group_read_many: records, the single readers' cursors
                    rows = g.read_many(pairs, "tsbk", cap_each=64)
                    assert all(row is not None and row.dtype == nat.TSBK_DTYPE for row in rows)
                    for i, row in enumerate(rows):
                        taken[i].append(row.copy())
            g.sync()
            assert fes[0].timing_read(nat.T_SLICE)[1] == 2 * K    # two launches per group block for both members
            total = 0
            for i, (m, c) in enumerate(pairs):
                assert len(fes[m].chan_read_tsbk(c)) == 0
                want, want_st = _want(fes[m], c)
                _same(np.concatenate(taken[i]), want, ("group", m, c))
                assert fes[m].chan_tsbk_state(c) == want_st
                total += len(want)
            print("group: %d records" % total)
            assert total > len(pairs)
    finally:
        for fe in fes:
            fe.close()


def test_read_many_over_64_channels_interleaved_with_the_single_readers(gpu_required):
    nat = gpu_required
    blk, K = 16000, 6
    x = _noise(64, blk * K)
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [_open_loose(nat, fe, -180000.0 + 5600.0 * j, j) for j in range(64)]
        taken = [[] for _ in cids]
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk])
            if b % 2:                                             # the batched reader, and on every fifth channel the single one first
                for i in range(0, 64, 5):
                    taken[i].append(fe.chan_read_tsbk(cids[i], max_records=3))
                for i, row in enumerate(fe.chan_read_many(cids, "tsbk", cap_each=32)):
                    assert row is not None and row.dtype == nat.TSBK_DTYPE
                    taken[i].append(row.copy())
        total = 0
        for i, c in enumerate(cids):
            taken[i].append(fe.chan_read_tsbk(c))
            want, want_st = _want(fe, c)
            _same(np.concatenate(taken[i]), want, ("channel", i))
            total += len(want)
        print("read_many: %d records" % total)
        assert total > 64 and fe.chan_read_many(cids[:2], "tsbk", cap_each=4)[0].shape == (0,)


# ------------------------------------------------------------------------------------------------ small rings
def test_record_ring_of_16_wraps_and_a_reader_left_behind_loses_the_oldest(gpu_required):
    nat = gpu_required
    blk, K = 16000, 15                                            # 192 symbols a block: 8 frames, each decided 384 dibits late
    x = _noise(16, blk * K)
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe, nat.Frontend(FS, device=0, block_capacity=blk) as tw:
        c, c_t = _open_loose(nat, fe, OFF, 0, capacity=16, search=EVERY), _open_loose(nat, tw, OFF, 0, capacity=1024, search=EVERY)
        assert fe.chan_tsbk_ring(c)[1] == 16 and tw.chan_tsbk_ring(c_t)[1] == 1024 and fe.chan_tsbk_ring(c)[0]
        cursor = lost = 0
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk]); tw.push(x[b * blk:(b + 1) * blk])
            if b % 5 != 4:                                        # every fifth block: 24 records the first time, 40 after
                continue
            n = tw.chan_tsbk_state(c_t)["n_records"]
            assert fe.chan_tsbk_state(c)["n_records"] == n and n - cursor > 16
            got = fe.chan_read_tsbk(c)
            first = max(cursor, n - 16)
            lost += first - cursor
            cursor = n
            whole = tw.chan_read_tsbk(c_t)                        # the twin's reader never lags: the stream's new records
            _same(got, whole[len(whole) - (n - first):], ("block", b))
        want, _ = _want(tw, c_t)
        assert lost > 10 and len(want) == cursor


def test_word_ring_of_64_wraps_and_a_hit_ring_of_16_loses_hits(gpu_required, tsdu):
    """out_capacity 64: the slicer's word ring holds 1024 dibits and wraps three times under the TSDU carrier; the frames are
    read across the wrap.  A block may not yield more than the rings hold (RCF_ECAP), so the stage never meets a frame whose
    words a block overwrote -- that count is held on the kernel's header by tests/test_tsbk_cpu.py.  The other loss it does
    meet: a hit ring of 16 under a search that hits 2.6 times in a hundred dibits fills while a frame waits for its 384
    dibits; n_lost and the records are the restatement's, which walks the whole streams -- from a twin with large rings --
    launch by launch, and the stage decodes on afterwards"""
    nat = gpu_required
    x = _shift(tsdu[0], OFF)
    blk = 16 * 48                                                 # 48 channel samples a block (and 5 of history in rings of 64): 9 or 10 symbols
    search = dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=14)
    launches, parts = [], []
    with nat.Frontend(FS, device=0, block_capacity=16 * 200, out_capacity=64) as fe, nat.Frontend(FS, device=0, block_capacity=blk) as tw:
        c, c_t = fe.chan_open(CR, OFF), tw.chan_open(CR, OFF)
        for f, ch in ((fe, c), (tw, c_t)):                        # (no pre-filter: its 69 taps reach further back than 64)
            f.chan_fm_filter(ch, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
            f.chan_fsk4(ch, **p25.fsk4_params(CR, 4800))
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, hit_capacity=16, **search)
        tw.chan_slicer(c_t, nat.READ_FSK4, nat.SLICE_FSK4, hit_capacity=4096, **search)
        fe.chan_tsbk(c, 1024)
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk]); tw.push(x[a:a + blk])
            s = fe.chan_slicer_state(c)
            launches.append((s["n_words"], s["n_hits"]))
            parts.append(fe.chan_read_tsbk(c))
        st = fe.chan_tsbk_state(c)
        assert fe.chan_slicer_state(c) == tw.chan_slicer_state(c_t) and launches[-1][0] > 3 * 64
        by = tw.chan_read_hard(c_t)
        k, dist = tw.chan_read_sync(c_t)
        assert _code(nat, fe.push, x[:16 * 200]) == nat.RCF_ECAP  # 200 outputs do not fit rings of 64
    want, want_st = T.run(by, k, dist, launches=launches, hit_cap=16)
    whole, whole_st = T.run(by, k, dist)
    _same(np.concatenate(parts), want, "rings of 64 and 16")
    print("rings of 64 and 16: %d hits, %s; with a ring that loses nothing %s" % (len(k), st, whole_st))
    assert st == want_st and st["n_lost"] > 0 and st["n_records"] > 0 and whole_st["n_lost"] == 0 and whole.tobytes() != want.tobytes()
    late = [len(p) for p in parts[len(parts) // 2:]]
    assert sum(late) > 0                                          # records still come in the stream's second half


# ------------------------------------------------------------------------------------------------ lifecycle, refusals, neighbours
def test_lifecycle_refusals_and_an_untouched_neighbour(gpu_required):
    nat = gpu_required
    blk, K = 16000, 4
    x = _noise(77, blk * K)

    def neighbour(with_stage):
        with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
            a, b = _open_loose(nat, fe, OFF, 0, tsbk=with_stage), _open_loose(nat, fe, OFF + 30000.0, 1, tsbk=False)
            for i in range(K):
                fe.push(x[i * blk:(i + 1) * blk])
            return fe.chan_read_hard(a).tobytes(), fe.chan_read_hard(b).tobytes(), fe.chan_read_sync(b)[0].tobytes()

    assert neighbour(True) == neighbour(False)                    # the stage writes nothing but its own ring and state
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = fe.chan_open(CR, OFF)
        assert _code(nat, fe.chan_tsbk, c) == nat.RCF_ESTATE      # no slicer
        assert _code(nat, fe.chan_tsbk, c + 1000) == nat.RCF_ENOCHAN
        fe.chan_tsbk(c, on=False)                                 # off without the stage: nothing to do
        fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
        fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_BINARY, sync_word=p25.FRAME_SYNC, sync_bits=48)
        assert _code(nat, fe.chan_tsbk, c) == nat.RCF_ESTATE      # not FSK4 mode
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, sync_word=0x2D6, sync_bits=10)
        assert _code(nat, fe.chan_tsbk, c) == nat.RCF_ESTATE      # not a 48-bit word
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **LOOSE)
        for cap in (8, 24, -16, (1 << 20) + 1):
            assert _code(nat, fe.chan_tsbk, c, cap) == nat.RCF_EINVAL
        fe.chan_tsbk(c, 64)
        assert fe.chan_tsbk_ring(c)[1] == 64 and fe.chan_tsbk_state(c) == dict(n_records=0, n_frames=0, n_blocks=0, n_crc_bad=0, n_lost=0)
        fe.push(x[:blk]); fe.push(x[blk:2 * blk]); fe.push(x[2 * blk:3 * blk])
        n1 = fe.chan_tsbk_state(c)["n_records"]
        assert n1 > 0
        first = fe.chan_slicer_state(c)["n_hits"]
        fe.chan_tsbk(c)                                           # again: afresh, from the hits that follow
        assert fe.chan_tsbk_ring(c)[1] == 256 and fe.chan_tsbk_state(c)["n_records"] == 0
        fe.push(x[3 * blk:])
        fe.push(x[:blk]); fe.push(x[blk:2 * blk])
        recs = fe.chan_read_tsbk(c)
        want, want_st = _want(fe, c, first_hit=first)
        _same(recs, want, "afresh")
        assert fe.chan_tsbk_state(c) == want_st and len(recs) > 0
        fe.chan_tsbk(c, on=False)
        assert _code(nat, fe.chan_tsbk_state, c) == nat.RCF_ESTATE and _code(nat, fe.chan_tsbk_ring, c) == nat.RCF_ESTATE
        fe.chan_tsbk(c)
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **LOOSE)   # the slicer attached again: the stage went with the old one
        assert _code(nat, fe.chan_tsbk_state, c) == nat.RCF_ESTATE
        fe.chan_tsbk(c)
        fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))              # the source loop attached again: slicer and stage go
        assert _code(nat, fe.chan_tsbk_state, c) == nat.RCF_ESTATE and _code(nat, fe.chan_slicer_state, c) == nat.RCF_ESTATE
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **LOOSE)
        fe.chan_tsbk(c)
        fe.chan_slicer(c, None)                                   # slicer off
        assert _code(nat, fe.chan_tsbk_state, c) == nat.RCF_ESTATE
        fe.push(x[:blk])                                          # and the front-end runs on without either
        fe.chan_close(c)
        assert _code(nat, fe.chan_tsbk, c) == nat.RCF_ENOCHAN
