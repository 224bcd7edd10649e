"""EDACS control frames on the GPU (rcf_chan_edacs; edacs.hip): frames from the slicer's sync hits of either polarity, six
40-bit copies per frame BCH-decoded and two messages elected behind a channel's binary slicer.  include/rcf.h defines the
stage, tests/edacs_ref.py restates it.  The yardstick is always that restatement applied to the channel's OWN packed words
and sync hits as the slicer's readers deliver them (chan_read_hard / chan_read_sync): the stage is integer work on those two
streams, so every comparison -- records, counters -- is of bits.  Where a case needs many frames on many channels it loosens
the slicer's sync search until the bits of noise hit: a frame is whatever follows a hit."""
import ctypes

import numpy as np
import pytest

import edacs_ref as E
import mm_ref as M
import slicer_ref as S
from rcf import control, p25, synth

pytestmark = pytest.mark.gpu

FS24, OFF24 = 2.4e6, 150000.0                                  # the clock's own test bench: 25 kS/s channels by 96
FS, CR, OFF = 400e3, 12500, 50000.0                            # 400 kS/s front-ends, 25 kS/s channels (decimation 16)
BAUD, DEV = 9600.0, 1200.0
BLK = 16 * 1000                                                # 1000 channel samples: 384 symbols
SEARCH = dict(sync_word=control.EDACS_SYNC, sync_bits=48)
# searches loose enough that noise hits: 17 of 48 lets about six in a hundred windows through (either polarity), 23 nine in ten
LOOSE = dict(SEARCH, sync_max_errors=17, sync_both=1, hit_capacity=4096)
MOST = dict(SEARCH, sync_max_errors=23, sync_both=1)


def _noise(seed, n, amp=0.05):
    return (amp * synth.awgn(np.random.default_rng(seed), n)).astype(np.complex64)


def _code(nat, fn, *a, **kw):
    with pytest.raises(nat.RcfError) as e:
        fn(*a, **kw)
    return e.value.code


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, len(got), len(want), got[:3], want[:3])


def _want(fe, c, **kw):
    """the restatement over everything the slicer's two readers deliver (the whole streams: nobody has read them before)"""
    by = fe.chan_read_hard(c)
    k, dist = fe.chan_read_sync(c)
    return E.run(by, k, dist, **kw)


def edacs_bits():
    """600 bits for the clock to settle, then twelve frames -> (bits, per frame (m1, m2) as the stage should give them, starts).
    Frames 0-2 clean and back to back; 3-5 with up to two flipped bits in every copy; 6 with three flips in one copy of each
    message; 7 with every copy of m2 beyond repair; 8-11 clean behind gaps that are no multiple of a word"""
    rng = np.random.default_rng(48)
    parts, sent, starts = [rng.integers(0, 2, 600).astype(np.uint8)], [], []
    at = 600
    for n in range(12):
        if n >= 8:
            gap = rng.integers(0, 2, 37 + n).astype(np.uint8)
            parts.append(gap)
            at += len(gap)
        m1, m2 = E.encode(rng.integers(0, 2, 28)), E.encode(rng.integers(0, 2, 28))
        f = E.frame(m1, m2)
        want = [E.bitstr(m1), E.bitstr(m2)]
        if 3 <= n <= 5:
            for c in range(6):
                for p in rng.choice(40, int(rng.integers(1, 3)), replace=False):
                    f[48 + 40 * c + p] ^= 1
        if n == 6:
            for c in (1, 5):
                for p in rng.choice(40, 3, replace=False):
                    f[48 + 40 * c + p] ^= 1
        if n == 7:
            f[48 + 120:48 + 240] ^= np.random.default_rng(0).integers(0, 2, 120).astype(np.uint8)
            want[1] = -1
        statuses, g1, g2 = E.decode_frame(f[48:])
        assert [E.bitstr(g1), E.bitstr(g2)] == want, n            # (what the restatement makes of the planted frame)
        parts.append(f); sent.append(tuple(want)); starts.append(at)
        at += 288
    parts.append(rng.integers(0, 2, 420).astype(np.uint8))
    return np.concatenate(parts), sent, starts


@pytest.fixture(scope="module")
def carriers():
    """edacs_bits as a 9600-baud 2-FSK carrier, and the same with every bit inverted -> ({inverted: x}, sent, starts)"""
    bits, sent, starts = edacs_bits()
    return {inv: M.fsk2_carrier(bits ^ inv, BAUD, FS24, OFF24, DEV, np.random.default_rng(5)) for inv in (0, 1)}, sent, starts


def _run(nat, x, pieces, attach_at=None, **stage):
    """the carrier pushed in pieces -> (records, state, the restatement's records, its state, n_hits at the attach)"""
    with nat.Frontend(FS24, device=0, block_capacity=max(b - a for a, b in zip(pieces[:-1], pieces[1:]))) as fe:
        c = fe.chan_open(12500, OFF24)
        control.edacs_clock(fe, c)
        fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_BINARY, sync_both=1, **SEARCH)
        if attach_at is None:
            fe.chan_edacs(c, **stage)
        first = 0
        for a, b in zip(pieces[:-1], pieces[1:]):
            if attach_at is not None and a == attach_at:
                first = fe.chan_slicer_state(c)["n_hits"]
                fe.chan_edacs(c, **stage)
            fe.push(x[a:b])
        recs, st = fe.chan_read_edacs(c), fe.chan_edacs_state(c)
        assert len(fe.chan_read_edacs(c)) == 0
        want, want_st = _want(fe, c, first_hit=first, esk=bool(stage.get("esk")))
    return recs, st, want, want_st, first


def _pieces(x, blk=48000):
    return list(range(0, len(x), blk)) + [len(x)]


# ------------------------------------------------------------------------------------------------ one channel, real frames
@pytest.mark.parametrize("inverted", [0, 1])
def test_every_sent_message_is_recovered_and_records_equal_the_restatement(gpu_required, carriers, inverted):
    nat = gpu_required
    xs, sent, starts = carriers
    recs, st, want, want_st, _ = _run(nat, xs[inverted], _pieces(xs[inverted]))
    _same(recs, want, "one channel")
    assert st == want_st and st["n_lost"] == 0 and st["n_frames"] == st["n_records"] == 12
    msgs = control.edacs_messages(recs)
    f = nat.edacs_fields(recs)
    print("edacs %s: %s, k %s, statuses %s" % ("inverted" if inverted else "upright", st, [m[0] for m in msgs], f["status"].tolist()))
    assert [m[1] for m in msgs] == [bool(inverted)] * 12 and not np.any(f["dist"])
    assert [(m[2], m[3]) for m in msgs] == sent                    # every sent message; "none" where all copies are broken
    assert np.diff([m[0] for m in msgs]).tolist() == np.diff(starts).tolist() and any((m[0] - 47) % 32 for m in msgs)
    status = f["status"]
    assert not np.any(status[:3]) and np.all((status[3:6] >= 1) & (status[3:6] <= 2))         # clean; one or two positions per copy
    assert status[7, 3:].tolist() == [3, 3, 3] and st["n_msgs"] == 23 and st["n_msgs_none"] == 1
    assert np.all(recs["zero"] == 0) and np.all(recs["m1"][:, 5:] == 0) and np.all(recs["m2"][:, 5:] == 0)


def test_records_do_not_depend_on_the_cuts(gpu_required, carriers):
    nat = gpu_required
    x = carriers[0][0]
    rng = np.random.default_rng(34)
    # random pieces, pieces of less than one channel sample (a block of 0 symbols), runs of pieces of one symbol (250 samples)
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 40)}
    cuts |= {96 * 4000 + 5 * j for j in range(1, 14)} | {96 * 6000 + 250 * j for j in range(40)} | {96 * 8000 + 96 * 30 * j for j in range(20)}
    cuts = sorted(cuts)
    one = _run(nat, x, [0, len(x)])
    ragged = _run(nat, x, cuts)
    _same(one[0], one[2], "one push"); _same(ragged[0], ragged[2], "ragged pushes")
    _same(ragged[0], one[0], "cuts")
    assert one[1] == one[3] == ragged[1] == ragged[3] and one[1]["n_records"] == 12


def test_attach_in_mid_frame_that_frame_does_not_appear_and_esk(gpu_required, carriers):
    nat = gpu_required
    xs, sent, starts = carriers
    x = xs[1]
    sps = FS24 / BAUD
    attach = int((starts[1] + 100) * sps) // 96 * 96               # inside the second frame, behind its sync word
    recs, st, want, want_st, first = _run(nat, x, [0, attach, len(x)], attach_at=attach, esk=True, capacity=32)
    _same(recs, want, "late attach")
    assert st == want_st and first >= 2 and st["n_records"] == 10
    esk = lambda m: m if m == -1 else "".join("1" if i in (0, 2) else ch for i, ch in enumerate(m))
    assert [(m[2], m[3]) for m in control.edacs_messages(recs)] == [(esk(a), esk(b)) for a, b in sent[2:]]
    assert any(esk(a) != a for a, _ in sent[2:])


# ------------------------------------------------------------------------------------------------ designed errors
def _run_designed(nat, bits):
    """the bits as a noise-free 2-FSK carrier on a 400 kS/s front-end, strict search of both polarities -> (records, state,
    the restatement's records, its state, the hits' k and dist, the decided frames' data bits)"""
    x = M.fsk2_carrier(bits, BAUD, FS, OFF, DEV, np.random.default_rng(5), noise=0.0)
    blk = 8 * BLK
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = fe.chan_open(CR, OFF)
        control.edacs_clock(fe, c, hard=True, frames=True)
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk])
        recs, st = fe.chan_read_edacs(c), fe.chan_edacs_state(c)
        by = fe.chan_read_hard(c)
        k, dist = fe.chan_read_sync(c)
    frames = []
    want, want_st = E.run(by, k, dist, frames=frames)
    return recs, st, want, want_st, k, dist, frames


@pytest.mark.parametrize("flips", [1, 2])
def test_designed_carrier_every_single_flip_and_every_pair_of_flips_is_corrected(gpu_required, flips):
    """All 40 single flips of a 40-bit copy on an inverted carrier (7 frames), all 780 pairs on an upright one (130 frames), the
    patterns rotating through the six copy slots -- the inverted slots 1 and 4 and both halves of the kernel's packed
    syndrome registers get every kind; every lane 0 .. 39 is a root of the Chien ballot, position 0 (lane 0's trial of 63)
    among them.  Records and counters are the restatement's over the channel's own words and hits; per copy status == number
    of flips; both messages elected and as sent.  tests/test_edacs_cpu.py holds the same on the planted bits."""
    nat = gpu_required
    patterns = E.flip_patterns()[flips - 1]
    bits, sent, starts, planted = E.designed_bits(patterns, 60 + flips, inverted=flips == 1)
    recs, st, want, want_st, k, dist, _ = _run_designed(nat, bits)
    f = nat.edacs_fields(recs)
    print("designed, %d flip(s): %d hits, %s" % (flips, len(k), st))
    _same(recs, want, "designed")
    assert st == want_st and st["n_lost"] == 0 and st["n_records"] == len(starts) == (len(patterns) + 5) // 6
    # the planted frames, all of them, at distance 0 of their polarity and where they were put
    assert len(k) == len(starts) and np.all(dist == (48 if flips == 1 else 0)) and np.diff(k).tolist() == np.diff(starts).tolist()
    assert not np.any(f["dist"]) and np.all(f["inverted"] == (flips == 1))
    assert f["status"].tolist() == [[len(p) for p in six] for six in planted]
    assert sorted(p for six in planted for p in six if p) == patterns and len(patterns) == (40, 780)[flips - 1]
    assert [(m[2], m[3]) for m in control.edacs_messages(recs)] == sent and st["n_msgs"] == 2 * len(starts)


def test_designed_carrier_of_the_classes_that_do_not_correct_and_the_election(gpu_required):
    """Copies chosen on the CPU from random 3- and 4-flip patterns (E.class_patterns: a bounded search that finds ten of each):
    status 3, status 2 that miscorrects, "stands" with S1 = 0 and S3 != 0, a position in 40 .. 47 (accepted, no bit changed),
    a position > 47 (fails); and frames for the election: one of three copies decoded, two that disagree, two that agree
    against a third.  The census is taken from the restatement over the delivered streams."""
    nat = gpu_required
    patterns, found = E.designed_classes()
    assert all(found[c] >= 10 for c in E.CLASSES), found
    bits, sent, starts, _ = E.designed_bits(patterns, 62)
    recs, st, want, want_st, k, dist, frames = _run_designed(nat, bits)
    seen = E.census(frames, sent)
    print("designed classes: %d hits, %s, census %s" % (len(k), st, seen))
    _same(recs, want, "designed classes")
    assert st == want_st and st["n_lost"] == 0 and st["n_records"] == len(starts) == len(frames)
    assert len(k) == len(starts) and not np.any(dist) and np.diff(k).tolist() == np.diff(starts).tolist()
    assert all(seen[c] >= 10 for c in E.CLASSES) and min(seen["one"], seen["differ"], seen["outvoted"]) >= 2, seen
    f = nat.edacs_fields(recs)
    assert set(f["status"].reshape(-1).tolist()) == {0, 1, 2, 3} and st["n_msgs_none"] == seen["differ"] > 0


# ------------------------------------------------------------------------------------------------ many channels, groups
def _kind_of(j):
    return "clock" if j in (0, 63, 64, 129) or j % 3 == 2 else ("fsk4", "costas")[j % 3]


def _open_loose(nat, fe, f, stage=True, search=LOOSE, **kw):
    """a channel at offset f with the EDACS clock, a slicer that searches noise loosely in both polarities, and the stage"""
    c = fe.chan_open(CR, f)
    control.edacs_clock(fe, c)
    fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_BINARY, **search)
    if stage:
        fe.chan_edacs(c, **kw)
    return c


def test_130_channels_of_mixed_kinds_one_launch_behind_the_slicers(gpu_required):
    nat = gpu_required
    K = 7
    x = _noise(131, BLK * K)
    offs = [-190000.0 + 2900.0 * j for j in range(130)]
    p25_search = dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=17, hit_capacity=4096)
    bare = {2, 65}                                                # a binary slicer but no stage
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        cids = []
        for j, f in enumerate(offs):
            if _kind_of(j) == "clock":
                cids.append(_open_loose(nat, fe, f, stage=j not in bare, esk=j % 2 == 1))
                continue
            c = fe.chan_open(CR, f)
            if _kind_of(j) == "fsk4":
                fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
                fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
                fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **p25_search)
                fe.chan_tsbk(c)                                   # the other stage behind a slicer rides in its own launch
            else:
                fe.chan_agc(c, 64, 1.0)
                fe.chan_costas(c, **p25.costas_params(CR, 4800))
                fe.chan_slicer(c, nat.READ_COSTAS, nat.SLICE_FSK4, **p25_search)
            cids.append(c)
        fe.timing_enable(True, classes=[nat.T_SLICE])
        for b in range(K):
            fe.push(x[b * BLK:(b + 1) * BLK])
        assert fe.timing_read(nat.T_SLICE)[1] == 3 * K            # the slicers' launch, the TSBK stages' and the EDACS stages'
        n_rec = n_inv = 0
        for j, c in enumerate(cids):
            if _kind_of(j) != "clock" or j in bare:
                assert _code(nat, fe.chan_read_edacs, c) == nat.RCF_ESTATE and _code(nat, fe.chan_edacs_state, c) == nat.RCF_ESTATE
                continue
            recs, st = fe.chan_read_edacs(c), fe.chan_edacs_state(c)
            want, want_st = _want(fe, c, esk=j % 2 == 1)
            _same(recs, want, ("lane", j))
            assert st == want_st and st["n_lost"] == 0 and len(recs) >= 3, (j, st, want_st)
            n_rec += len(recs); n_inv += int(np.sum(recs["flags"] & 1))
        print("130 channels: %d records on %d channels, %d inverted" % (n_rec, sum(_kind_of(j) == "clock" for j in range(130)) - len(bare), n_inv))
        assert 0 < n_inv < n_rec


def test_two_front_ends_in_a_group_and_the_group_reader_beside_the_single_one(gpu_required):
    nat = gpu_required
    K = 8
    xs = [_noise(40 + m, BLK * K) for m in range(2)]
    offs = [(-100000.0, 60000.0, 150000.0), (30000.0, -150000.0, 90000.0)]
    fes = [nat.Frontend(FS, device=0, block_capacity=BLK) for _ in range(2)]
    try:
        ids = [[_open_loose(nat, fe, f) for f in offs[m]] for m, fe in enumerate(fes)]
        fes[0].timing_enable(True, classes=[nat.T_SLICE])
        pairs = [(m, c) for m in range(2) for c in ids[m]]
        taken = [[] for _ in pairs]
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * BLK:(b + 1) * BLK] for xm in xs])
                if b >= 2:                                        # rcf_group_read_many, and the single reader first on two of them
                    for i in (1, 4):
                        taken[i].append(fes[pairs[i][0]].chan_read_edacs(pairs[i][1], max_records=1))
                    rows = g.read_many(pairs, "edacs", cap_each=64)
                    assert all(row is not None and row.dtype == nat.EDACS_DTYPE for row in rows)
                    for i, row in enumerate(rows):
                        taken[i].append(row.copy())
            g.sync()
            assert fes[0].timing_read(nat.T_SLICE)[1] == 2 * K    # two launches per group block for both members
            total = 0
            for i, (m, c) in enumerate(pairs):
                assert len(fes[m].chan_read_edacs(c)) == 0
                want, want_st = _want(fes[m], c)
                _same(np.concatenate(taken[i]), want, ("group", m, c))
                assert fes[m].chan_edacs_state(c) == want_st
                total += len(want)
            print("group: %d records" % total)
            assert total > 3 * len(pairs)
    finally:
        for fe in fes:
            fe.close()


def test_read_many_over_64_channels_interleaved_with_the_single_readers(gpu_required):
    nat = gpu_required
    K = 6
    x = _noise(64, BLK * K)
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        cids = [_open_loose(nat, fe, -180000.0 + 5600.0 * j) for j in range(64)]
        taken = [[] for _ in cids]
        for b in range(K):
            fe.push(x[b * BLK:(b + 1) * BLK])
            if b % 2:                                             # the batched reader, and on every fifth channel the single one first
                for i in range(0, 64, 5):
                    taken[i].append(fe.chan_read_edacs(cids[i], max_records=1))
                for i, row in enumerate(fe.chan_read_many(cids, "edacs", cap_each=32)):
                    assert row is not None and row.dtype == nat.EDACS_DTYPE
                    taken[i].append(row.copy())
        total = 0
        for i, c in enumerate(cids):
            taken[i].append(fe.chan_read_edacs(c))
            want, _ = _want(fe, c)
            _same(np.concatenate(taken[i]), want, ("channel", i))
            total += len(want)
        print("read_many: %d records" % total)
        assert total > 3 * 64 and fe.chan_read_many(cids[:2], "edacs", cap_each=4)[0].shape == (0,)


# ------------------------------------------------------------------------------------------------ small rings
def test_record_ring_of_16_wraps_and_a_reader_left_behind_loses_the_oldest(gpu_required):
    nat = gpu_required
    K = 32                                                        # 384 symbols a block: a frame every 288 under a search that hits nine bits in ten
    x = _noise(16, BLK * K)
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe, nat.Frontend(FS, device=0, block_capacity=BLK) as tw:
        c = _open_loose(nat, fe, OFF, search=dict(MOST, hit_capacity=1 << 14), capacity=16)     # (11000 hits: the twin's reader keeps them all)
        c_t = _open_loose(nat, tw, OFF, search=dict(MOST, hit_capacity=1 << 14), capacity=1024)
        assert fe.chan_edacs_ring(c)[1] == 16 and tw.chan_edacs_ring(c_t)[1] == 1024 and fe.chan_edacs_ring(c)[0]
        cursor = lost = 0
        for b in range(K):
            fe.push(x[b * BLK:(b + 1) * BLK]); tw.push(x[b * BLK:(b + 1) * BLK])
            if b % 16 != 15:                                      # every sixteenth block: about 21 records
                continue
            n = tw.chan_edacs_state(c_t)["n_records"]
            assert fe.chan_edacs_state(c)["n_records"] == n and n - cursor > 16
            got = fe.chan_read_edacs(c)
            first = max(cursor, n - 16)
            lost += first - cursor
            cursor = n
            whole = tw.chan_read_edacs(c_t)                       # the twin's reader never lags: the stream's new records
            _same(got, whole[len(whole) - (n - first):], ("block", b))
        want, _ = _want(tw, c_t)
        assert lost >= 2 and len(want) == cursor


def test_a_hit_ring_of_16_loses_hits_and_they_are_counted(gpu_required):
    """a search that lets three in a hundred windows through brings about 45 hits per push of 1536 symbols to a ring of 16:
    the frame that waited for its 288 bits has left the ring by the next launch, and so have the hits in front of the last 16.
    n_lost and the records are the restatement's, which walks the whole streams -- from a twin with a large hit ring -- launch
    by launch; a frame among the last 16 hits is still decoded every time"""
    nat = gpu_required
    K, blk = 6, 4 * BLK
    x = _noise(17, blk * K)
    search = dict(SEARCH, sync_max_errors=16, sync_both=1)
    launches, parts = [], []
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe, nat.Frontend(FS, device=0, block_capacity=blk) as tw:
        c = _open_loose(nat, fe, OFF, search=dict(search, hit_capacity=16))
        c_t = _open_loose(nat, tw, OFF, search=dict(search, hit_capacity=4096), stage=False)
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk]); tw.push(x[b * blk:(b + 1) * blk])
            s = fe.chan_slicer_state(c)
            launches.append((s["n_words"], s["n_hits"]))
            parts.append(fe.chan_read_edacs(c))
        st = fe.chan_edacs_state(c)
        assert fe.chan_slicer_state(c) == tw.chan_slicer_state(c_t)
        by = tw.chan_read_hard(c_t)
        k, dist = tw.chan_read_sync(c_t)
    want, want_st = E.run(by, k, dist, launches=launches, hit_cap=16)
    whole, whole_st = E.run(by, k, dist)
    _same(np.concatenate(parts), want, "hit ring of 16")
    print("hit ring of 16: %d hits, %s; with a ring that loses nothing %s" % (len(k), st, whole_st))
    assert st == want_st and st["n_lost"] > 20 and st["n_records"] >= 2 and whole_st["n_lost"] == 0 and whole_st["n_records"] > st["n_records"]


# ------------------------------------------------------------------------------------------------ the slicer alone
@pytest.mark.parametrize("max_errors", [0, 17, 23])
def test_slicer_with_sync_both_alone_against_its_restatement(gpu_required, carriers, max_errors):
    nat = gpu_required
    x = carriers[0][1][:96 * 3000] if max_errors else carriers[0][1]          # the inverted carrier (a part of it under the loose searches)
    rng = np.random.default_rng(max_errors)
    pieces = sorted({0, len(x)} | {int(v) for v in rng.integers(1, len(x), 12)})
    kw = dict(SEARCH, sync_max_errors=max_errors, hit_capacity=1 << 16)
    with nat.Frontend(FS24, device=0, block_capacity=len(x)) as fe:
        c, c0 = fe.chan_open(12500, OFF24), fe.chan_open(12500, OFF24)
        control.edacs_clock(fe, c); control.edacs_clock(fe, c0)
        fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_BINARY, sync_both=1, **kw)
        fe.chan_slicer(c0, nat.READ_CLOCK, nat.SLICE_BINARY, **kw)                 # its twin with sync_both = 0: as before
        for a, b in zip(pieces[:-1], pieces[1:]):
            fe.push(x[a:b])
        soft = fe.chan_read_clock(c)
        got = (fe.chan_read_hard(c), *fe.chan_read_sync(c), fe.chan_slicer_state(c))
        got0 = (fe.chan_read_hard(c0), *fe.chan_read_sync(c0), fe.chan_slicer_state(c0))
    for (by, k, dist, st), both in ((got, 1), (got0, 0)):
        r = E.slicer(soft, max_errors=max_errors, sync_both=both)
        assert np.array_equal(by.view("<u4"), r["words"]) and np.array_equal(k, r["k"]) and np.array_equal(dist, r["dist"]), (both, k[:8], r["k"][:8])
        assert st == dict(n_symbols=len(soft), n_words=len(r["words"]), n_hits=len(r["k"]))
    r0 = S.run(soft, S.BINARY, sync_word=control.EDACS_SYNC, sync_bits=48, max_errors=max_errors)
    assert np.array_equal(got0[1], r0["k"]) and np.array_equal(got0[2], r0["dist"])            # the existing restatement, untouched
    inv = got[2] > 24
    print("sync_both, max_errors %d: %d hits, %d of them inverted; %d without" % (max_errors, len(got[1]), int(np.sum(inv)), len(got0[1])))
    assert np.sum(inv) >= (12 if max_errors == 0 else 3) and np.all((got[2][inv] >= 48 - max_errors))
    assert got[0].tobytes() == got0[0].tobytes() and len(got[1]) > len(got0[1])


# ------------------------------------------------------------------------------------------------ lifecycle, refusals
def test_lifecycle_and_refusals(gpu_required):
    nat = gpu_required
    lib = nat.lib()
    K = 4
    x = _noise(77, BLK * K)
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        c = fe.chan_open(CR, OFF)
        assert _code(nat, fe.chan_edacs, c) == nat.RCF_ESTATE     # no slicer
        assert _code(nat, fe.chan_edacs, c + 1000) == nat.RCF_ENOCHAN
        fe.chan_edacs(c, on=False)                                # off without the stage: nothing to do
        control.edacs_clock(fe, c)
        B = nat.SLICE_BINARY
        # sync_both: 0 or 1, and the two polarities' ranges of dist must not meet
        for bad in (dict(SEARCH, sync_both=2), dict(SEARCH, sync_both=-1), dict(SEARCH, sync_both=1, sync_max_errors=24),
                    dict(sync_word=0x2D, sync_bits=8, sync_both=1, sync_max_errors=4), dict(sync_both=1)):
            assert _code(nat, fe.chan_slicer, c, nat.READ_CLOCK, B, **bad) == nat.RCF_EINVAL, bad
        for good in (dict(SEARCH, sync_both=1, sync_max_errors=23), dict(sync_word=0x2D, sync_bits=8, sync_both=1, sync_max_errors=3)):
            fe.chan_slicer(c, nat.READ_CLOCK, B, **good)
        assert _code(nat, fe.chan_edacs, c) == nat.RCF_ESTATE     # not a 48-bit word
        fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_FSK4, sync_word=p25.FRAME_SYNC, sync_bits=48, sync_both=1, sync_max_errors=4)
        assert _code(nat, fe.chan_edacs, c) == nat.RCF_ESTATE     # not binary
        assert _code(nat, fe.chan_tsbk, c) == nat.RCF_ESTATE      # and the TSBK stage refuses a slicer that searches both polarities
        fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_FSK4, sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=4)
        fe.chan_tsbk(c)                                           # (as before without the flag)
        fe.chan_slicer(c, nat.READ_CLOCK, B, **SEARCH)            # sync_both = 0: the stage applies, upright frames only
        fe.chan_edacs(c)
        fe.chan_slicer(c, nat.READ_CLOCK, B, **LOOSE)
        assert _code(nat, fe.chan_edacs_state, c) == nat.RCF_ESTATE                      # the slicer attached again: the stage went with the old one
        for cap in (8, 24, -16, (1 << 20) + 1):
            assert _code(nat, fe.chan_edacs, c, cap) == nat.RCF_EINVAL
        fe.chan_edacs(c, 64)
        assert fe.chan_edacs_ring(c)[1] == 64 and fe.chan_edacs_state(c) == dict(n_records=0, n_frames=0, n_msgs=0, n_msgs_none=0, n_lost=0)
        for b in range(3):
            fe.push(x[b * BLK:(b + 1) * BLK])
        assert fe.chan_edacs_state(c)["n_records"] > 0
        first = fe.chan_slicer_state(c)["n_hits"]
        fe.chan_edacs(c)                                          # again: afresh, from the hits that follow
        assert fe.chan_edacs_ring(c)[1] == 256 and fe.chan_edacs_state(c)["n_records"] == 0
        fe.push(x[3 * BLK:]); fe.push(x[:BLK]); fe.push(x[BLK:2 * BLK])
        recs = fe.chan_read_edacs(c)
        want, want_st = _want(fe, c, first_hit=first)
        _same(recs, want, "afresh")
        assert fe.chan_edacs_state(c) == want_st and len(recs) > 0
        # the raw batched ABI: 49 is a stream of 8-word records; 50 is none
        cid, cnt = (ctypes.c_int * 1)(c), (ctypes.c_int64 * 1)()
        buf = np.zeros(16 * 8, dtype=np.uint32)
        assert lib.rcf_chan_read_many(fe._h, nat.HARD_EDACS, cid, 1, 1.0, buf.ctypes.data_as(ctypes.c_void_p), 16, cnt) == nat.RCF_OK and cnt[0] == 0
        assert lib.rcf_chan_read_many(fe._h, 50, cid, 1, 1.0, buf.ctypes.data_as(ctypes.c_void_p), 16, cnt) == nat.RCF_EINVAL
        # the pump does not deliver it: refused at start and at subscribe, as 32, 33 and 48 are
        ring = nat.PinnedArray(2 * 2 * BLK, np.uint8)
        ring.array[:] = 127
        counter = np.zeros(1, dtype=np.uint64)
        grp = nat.Group([fe])
        try:
            assert _code(nat, nat.Pump, grp, [ring], BLK, FS, (), fmt=nat.FMT_U8, what="edacs", max_read=4, written=[counter],
                         start_delay_s=0.0) == nat.RCF_EINVAL
            pump = nat.Pump(grp, [ring], BLK, FS, (), fmt=nat.FMT_U8, what="clock", max_read=4, written=[counter], start_delay_s=0.0)
            cur = ctypes.c_int64(0)
            for what in (nat.HARD_EDACS, nat.HARD_TSBK):
                assert lib.rcf_pump_subscribe(pump._p, 0, c, what, 1.0, ctypes.byref(cur)) == nat.RCF_EINVAL, what
            pump.stop()
        finally:
            grp.close()
            ring.free()
        fe.chan_edacs(c, on=False)
        assert _code(nat, fe.chan_edacs_state, c) == nat.RCF_ESTATE and _code(nat, fe.chan_edacs_ring, c) == nat.RCF_ESTATE
        fe.chan_edacs(c)
        control.edacs_clock(fe, c)                                # the source loop attached again: slicer and stage go
        assert _code(nat, fe.chan_edacs_state, c) == nat.RCF_ESTATE and _code(nat, fe.chan_slicer_state, c) == nat.RCF_ESTATE
        control.edacs_clock(fe, c, hard=True, frames=True, esk=True)             # the helper: clock, slicer with sync_both, stage
        assert fe.chan_edacs_ring(c)[1] == 256
        fe.chan_slicer(c, None)                                   # slicer off
        assert _code(nat, fe.chan_edacs_state, c) == nat.RCF_ESTATE
        fe.push(x[:BLK])                                          # and the front-end runs on without either
        fe.chan_close(c)
        assert _code(nat, fe.chan_edacs, c) == nat.RCF_ENOCHAN
