"""P25 voice data units on the GPU (rcf_chan_p25lc; p25lc.hip): frames from the slicer's sync hits, status symbols, NID, and
for an HDU, an LDU1 or a TLC the inner Golay / Hamming words and the outer Reed-Solomon word behind a channel's slicer.
include/rcf.h defines the stage, tests/p25lc_ref.py restates it in numpy.  The yardstick is always that restatement applied
to the channel's OWN packed words and sync hits as the slicer's readers deliver them (chan_read_hard / chan_read_sync): the
stage is integer work on those two streams, so every comparison -- records, counters -- is of bits.  Where a case needs many
frames on many channels it loosens the slicer's sync search until the bits of noise hit: a frame is whatever follows a hit."""
import ctypes

import numpy as np
import pytest

import fsk4_ref as F
import gc_ref as G
import p25lc_ref as R
import tsbk_ref as T
from rcf import p25, synth

pytestmark = pytest.mark.gpu

FS, CR, OFF = F.FS, F.CHANNEL_RATE, F.CHANNEL_OFFSET          # 400 kS/s front-ends, 25 kS/s channels (decimation 16)
BLK = 16 * 1000
NAC = R.CALL["nac"]


def _loose(kind, errors=None):
    """a search loose enough that noise's dibits hit now and then (tests/test_gpu_tsbk.py: behind the C4FM loop about 19 of
    48 bits of noise differ from the sync word, behind the Gardner / Costas loop 24); `errors` below that default makes the
    hits sparse enough for frames of hundreds of dibits"""
    return dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=errors or (13 if kind == "fsk4" else 17), hit_capacity=4096)


def _shift(x0, f):
    return (x0 * np.exp(2j * np.pi * f / FS * np.arange(len(x0)))).astype(np.complex64)


def _noise(seed, n, amp=0.05):
    return (amp * synth.awgn(np.random.default_rng(seed), n)).astype(np.complex64)


def _code(nat, fn, *a, **kw):
    with pytest.raises(nat.RcfError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.fixture(scope="module")
def call():
    """R.call_dibits as one 4800-baud C4FM carrier at the channel's offset, 150 Hz off -> (x, the frames' starts, their names)"""
    d, starts, shorts = R.call_dibits()
    return F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0), starts, shorts


def _want(fe, c, **kw):
    """the restatement over everything the slicer's two readers deliver (the whole streams: nobody has read them before)"""
    by = fe.chan_read_hard(c)
    k, dist = fe.chan_read_sync(c)
    return R.run(by, k, dist, **kw)


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, len(got), len(want), got[:4], want[:4])


def _run_call(nat, x, pieces, correct, attach_at=None, demod=p25.c4fm_demod):
    """the carrier pushed in pieces -> (records, state, restatement's records, its state, n_hits at the attach)"""
    with nat.Frontend(FS, device=0, block_capacity=max(b - a for a, b in zip(pieces[:-1], pieces[1:]))) as fe:
        c = demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, lc=attach_at is None)
        if attach_at is None and not correct:
            fe.chan_p25lc(c, correct=False)
        first = 0
        for a, b in zip(pieces[:-1], pieces[1:]):
            if attach_at is not None and a == attach_at:
                first = fe.chan_slicer_state(c)["n_hits"]
                fe.chan_p25lc(c, correct=correct)
            fe.push(x[a:b])
        recs, st = fe.chan_read_p25lc(c), fe.chan_p25lc_state(c)
        assert len(fe.chan_read_p25lc(c)) == 0
        want, want_st = _want(fe, c, first_hit=first, correct=correct)
    return recs, st, want, want_st, first


def _check_call(units, shorts, correct):
    """the planted call as voice_units gives it: every unit in order, the sent talkgroup, source and termination"""
    c = R.CALL
    assert [u["short"] for u in units] == shorts and all(u["nac"] == NAC and u["dist"] == 0 for u in units)
    assert [u["frame_dibits"] for u in units] == [396] + [864] * 7 and [u["decoded"] for u in units] == [s in ("HDU", "LDU1", "TLC") for s in shorts]
    hdu, ldu1, tlc = units[0], [u for u in units if u["short"] == "LDU1"], units[-1]
    assert (hdu["mi"], hdu["mfid"], hdu["algid"], hdu["kid"], hdu["tgid"]) == (c["mi"], c["mfid"], c["algid"], c["kid"], c["tgid"])
    clean = ldu1 if correct else [ldu1[0], ldu1[2]]                # the second LDU1 carries errors that only the decoders remove
    for u in clean:
        assert (u["lc"]["lcf_long"], u["lc"]["tgid"], u["lc"]["source_id"], u["lsd"]) == ("Group Voice Channel User", c["tgid"], c["source_id"], c["lsd"])
    assert tlc["lc"]["lcf_long"] == "Call Termination / Cancellation"
    if correct:
        assert [(u["n_rs"], u["n_fixed"], u["n_bad"], u["rs_bad"]) for u in ldu1] == [(0, 0, 0, 0), (2, 4, 0, 0), (0, 0, 0, 0)]
    else:
        assert not any(u["n_rs"] or u["n_fixed"] or u["n_bad"] or u["rs_bad"] for u in units) and ldu1[1]["lc"] != ldu1[0]["lc"]


# ------------------------------------------------------------------------------------------------ one channel, a call
@pytest.mark.parametrize("correct", [1, 0])
def test_a_call_whole_ragged_and_block_by_block_equals_the_restatement(gpu_required, call, correct):
    nat = gpu_required
    x, starts, shorts = call
    rng = np.random.default_rng(34)
    # random pieces, pieces of less than one channel sample (a block of 0 symbols), runs of pieces of one symbol (83 samples)
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 40)}
    cuts |= {16 * 4000 + 5 * j for j in range(1, 14)} | {16 * 6000 + 84 * j for j in range(40)} | {16 * 9000 + 16 * 30 * j for j in range(20)}
    whole = _run_call(nat, x, [0, len(x)], correct)
    ragged = _run_call(nat, x, sorted(cuts), correct)
    blocks = _run_call(nat, x, list(range(0, len(x), BLK)) + [len(x)], correct)
    for name, r in (("whole", whole), ("ragged", ragged), ("blocks", blocks)):
        _same(r[0], r[2], name)
        assert r[1] == r[3], name
    _same(ragged[0], whole[0], "cuts"); _same(blocks[0], whole[0], "blocks")
    assert whole[1] == ragged[1] == blocks[1] == dict(n_records=8, n_frames=8, n_decoded=5, n_rs_bad=0, n_lost=0)
    units = p25.voice_units(whole[0])
    print("call (correct=%d): %s" % (correct, [(u["short"], u["k"], u["n_rs"], u["n_fixed"]) for u in units]))
    assert np.diff([u["k"] for u in units]).tolist() == np.diff(starts).tolist()
    _check_call(units, shorts, correct)


def test_the_same_call_through_the_gardner_costas_chain(gpu_required):
    nat = gpu_required
    d, starts, shorts = R.call_dibits()
    d = np.concatenate([d, np.random.default_rng(1).integers(0, 4, 256).astype(np.uint8)])    # (the AGC's window holds 200 symbols back)
    x = G.dqpsk_carrier(d, 4800, FS, OFF + 60.0, 0.4, amplitude=0.4)
    recs, st, want, want_st, _ = _run_call(nat, x, list(range(0, len(x), BLK)) + [len(x)], 1, demod=p25.cqpsk_demod)
    _same(recs, want, "cqpsk")
    assert st == want_st and st["n_lost"] == 0
    units = [u for u in p25.voice_units(recs) if u["nac"] == NAC and u["dist"] == 0]
    print("cqpsk call: %s, %s" % (st, [(u["short"], u["k"], u["n_rs"], u["n_fixed"]) for u in units]))
    _check_call(units, shorts, 1)


def test_attach_in_mid_frame_that_frame_does_not_appear(gpu_required, call):
    nat = gpu_required
    x, starts, shorts = call
    attach = int((starts[1] + 100) * FS / 4800.0) // 16 * 16       # inside the first LDU1, behind its sync word
    recs, st, want, want_st, first = _run_call(nat, x, [0, attach, len(x)], 1, attach_at=attach)
    _same(recs, want, "late attach")
    assert st == want_st and first >= 2
    assert [u["short"] for u in p25.voice_units(recs)] == shorts[2:]              # the first LDU2 is the first to appear


# ------------------------------------------------------------------------------------------------ designed errors
def test_designed_carrier_walks_every_correcting_path(gpu_required):
    """R.designed_dibits as a noise-free C4FM carrier under the strict search: 33 data units, among them HDUs, LDU1s and TLCs
    with 1 .. t + 1 planted Reed-Solomon symbol errors, inner words with 1, 2, 3 flipped bits, Hamming words with a syndrome
    that is no column's, (18,6) words next to a code word of the longer code, a frame cut short and every unit without link
    control.  Records and counters are the restatement's over the channel's own words and hits, and the census over those
    says that the kernel met what the input was built for.  tests/test_p25lc_cpu.py holds the same census on the planted
    dibits."""
    nat = gpu_required
    d, plan = R.designed_dibits(NAC)
    x = F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0)
    blk = 4 * BLK
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, lc=True)
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk])
        recs, st = fe.chan_read_p25lc(c), fe.chan_p25lc_state(c)
        by = fe.chan_read_hard(c)
        k, dist = fe.chan_read_sync(c)
    units = []
    want, want_st = R.run(by, k, dist, units=units)
    f = nat.p25lc_fields(recs)
    print("designed: %d hits, %s; n_rs %s" % (len(k), st, f["n_rs"].tolist()))
    _same(recs, want, "designed")
    assert st == want_st == dict(n_records=33, n_frames=33, n_decoded=27, n_rs_bad=3, n_lost=0)
    # the planted frames, all of them, at distance 0 and where they were put (the loop's delay moves them all alike)
    starts = [p["start"] for p in plan]
    assert len(k) == len(starts) and not np.any(dist) and np.diff(k).tolist() == np.diff(starts).tolist()
    shift = int(k[0]) - 23 - starts[0]
    R.check_census(recs, units, [dict(p, start=p["start"] + shift) for p in plan])


# ------------------------------------------------------------------------------------------------ many channels, groups
def _open_loose(nat, fe, f, j, stage="p25lc", search=None, **kw):
    """channel j at offset f: a P25 loop (Gardner / Costas on every third), the slicer with a loose search, the stage"""
    kind = "costas" if j % 3 == 1 else "fsk4"
    c = fe.chan_open(CR, f)
    if kind == "fsk4":
        fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
        fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
    else:
        fe.chan_agc(c, 64, 1.0)
        fe.chan_costas(c, **p25.costas_params(CR, 4800))
    fe.chan_slicer(c, nat.READ_FSK4 if kind == "fsk4" else nat.READ_COSTAS, nat.SLICE_FSK4, **(search or _loose(kind)))
    if stage == "p25lc":
        fe.chan_p25lc(c, **kw)
    elif stage == "tsbk":
        fe.chan_tsbk(c)
    return c


def test_five_channels_a_second_workgroup_and_noise_frames(gpu_required, call):
    """five stages in one launch: a full workgroup of four waves and a second with one.  The call's carrier under channel 0
    (strict search); the others search noise behind a C4FM or a Gardner / Costas loop, from a few hits in a hundred dibits
    (frames of some dozen dibits, all frame records) down to one in a hundred and more (frames long enough for a unit,
    which then decodes noise), one of them in the uncorrected mode"""
    nat = gpu_required
    x0, _, shorts = call
    K = (len(x0) + BLK - 1) // BLK
    x = _noise(5, BLK * K) + 0.3 * np.concatenate([x0, np.zeros(K * BLK - len(x0), np.complex64)])
    offs = [OFF, -150000.0, -60000.0, 30000.0, 160000.0]
    errors = [p25.FRAME_SYNC_MAX_ERRORS, 15, 14, 11, 17]          # (channels 1 and 4 stand behind Gardner / Costas loops)
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        cids = [_open_loose(nat, fe, f, j, search=_loose("", errors[j]), correct=j != 3) for j, f in enumerate(offs)]
        fe.timing_enable(True, classes=[nat.T_SLICE])
        for b in range(K):
            fe.push(x[b * BLK:(b + 1) * BLK])
        assert fe.timing_read(nat.T_SLICE)[1] == 2 * K            # the slicers' launch and the stages' behind it
        for j, c in enumerate(cids):
            recs, st = fe.chan_read_p25lc(c), fe.chan_p25lc_state(c)
            want, want_st = _want(fe, c, correct=int(j != 3))
            _same(recs, want, ("lane", j))
            assert st == want_st and st["n_lost"] == 0, (j, st, want_st)
            f = nat.p25lc_fields(recs)
            print("channel %d: %s, kinds %s, duids %d" % (j, st, np.bincount(f["kind"], minlength=4).tolist(), len(set(f["duid"].tolist()))))
            if j == 0:
                _check_call([u for u in p25.voice_units(recs) if u["nac"] == NAC and u["dist"] == 0], shorts, 1)
            if j in (2, 4):
                assert len(recs) > 50, j


def test_two_front_ends_in_a_group_with_mixed_stages(gpu_required):
    """a group's block: on each member one channel with the TSBK stage and one with the P25 voice stage -- the slicers' launch,
    the TSBK stages' and the voice stages', each once per block for both members"""
    nat = gpu_required
    blk, K = 16000, 10                                            # 1920 dibits: the frames of the first 1032 are decided
    xs = [_noise(40 + m, blk * K) for m in range(2)]
    offs = [(-100000.0, 60000.0), (30000.0, -150000.0)]
    fes = [nat.Frontend(FS, device=0, block_capacity=blk) for _ in range(2)]
    try:
        ids = [[_open_loose(nat, fe, f, 0, stage=("tsbk", "p25lc")[(j + m) % 2], search=_loose("fsk4", 16)) for j, f in enumerate(offs[m])]
               for m, fe in enumerate(fes)]
        lc = [(m, ids[m][j]) for m in range(2) for j in range(2) if (j + m) % 2 == 1]
        ts = [(m, ids[m][j]) for m in range(2) for j in range(2) if (j + m) % 2 == 0]
        fes[0].timing_enable(True, classes=[nat.T_SLICE])
        taken = {p: [] for p in lc + ts}
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * blk:(b + 1) * blk] for xm in xs])
                if b >= 6:                                        # rcf_group_read_many: records, the single readers' cursors
                    for pairs, what, dtype in ((lc, "p25lc", nat.P25LC_DTYPE), (ts, "tsbk", nat.TSBK_DTYPE)):
                        rows = g.read_many(pairs, what, cap_each=64)
                        assert all(row is not None and row.dtype == dtype for row in rows)
                        for p, row in zip(pairs, rows):
                            taken[p].append(row.copy())
            g.sync()
            assert fes[0].timing_read(nat.T_SLICE)[1] == 3 * K    # three launches per group block for both members
            total = 0
            for m, c in lc:
                assert len(fes[m].chan_read_p25lc(c)) == 0 and _code(nat, fes[m].chan_read_tsbk, c) == nat.RCF_ESTATE
                want, want_st = _want(fes[m], c)
                _same(np.concatenate(taken[(m, c)]), want, ("group", m, c))
                assert fes[m].chan_p25lc_state(c) == want_st
                total += len(want)
            for m, c in ts:
                assert len(fes[m].chan_read_tsbk(c)) == 0 and _code(nat, fes[m].chan_read_p25lc, c) == nat.RCF_ESTATE
                by = fes[m].chan_read_hard(c)
                k, dist = fes[m].chan_read_sync(c)
                want, want_st = T.run(by, k, dist)
                _same(np.concatenate(taken[(m, c)]), want, ("group tsbk", m, c))
                assert fes[m].chan_tsbk_state(c) == want_st and len(want) > 0
            print("group: %d voice records" % total)
            assert total > len(lc)
    finally:
        for fe in fes:
            fe.close()


# ------------------------------------------------------------------------------------------------ small rings
def test_word_ring_of_64_wraps_and_a_hit_ring_of_16_loses_hits(gpu_required, call):
    """out_capacity 64: the slicer's word ring holds 1024 dibits -- 136 more than a frame waits for -- and wraps seven times
    under the call's carrier; the frames are read across the wrap.  A block may not yield more than the rings hold (RCF_ECAP),
    so with the largest blocks such rings take the stage never meets a frame whose words a block overwrote -- that count is
    held on the kernel's header by tests/test_p25lc_cpu.py.  The other loss it does meet: a hit ring of 16 under a search that
    hits a few times in a hundred dibits fills while a frame waits for its 888 dibits; n_lost and the records are the
    restatement's, which walks the whole streams -- from a twin with large rings -- launch by launch, and the stage decodes on
    afterwards"""
    nat = gpu_required
    x = call[0]
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
        fe.chan_p25lc(c, 1024)
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk]); tw.push(x[a:a + blk])
            s = fe.chan_slicer_state(c)
            launches.append((s["n_words"], s["n_hits"]))
            parts.append(fe.chan_read_p25lc(c))
        st = fe.chan_p25lc_state(c)
        assert fe.chan_slicer_state(c) == tw.chan_slicer_state(c_t) and launches[-1][0] > 6 * 64
        by = tw.chan_read_hard(c_t)
        k, dist = tw.chan_read_sync(c_t)
        assert _code(nat, fe.push, x[:16 * 200]) == nat.RCF_ECAP  # 200 outputs do not fit rings of 64
    want, want_st = R.run(by, k, dist, launches=launches, hit_cap=16)
    whole, whole_st = R.run(by, k, dist)
    _same(np.concatenate(parts), want, "rings of 64 and 16")
    print("rings of 64 and 16: %d hits, %s; with a ring that loses nothing %s" % (len(k), st, whole_st))
    assert st == want_st and st["n_lost"] > 0 and st["n_records"] > 0 and whole_st["n_lost"] == 0 and whole.tobytes() != want.tobytes()
    assert sum(len(p) for p in parts[len(parts) // 2:]) > 0       # records still come in the stream's second half


# ------------------------------------------------------------------------------------------------ lifecycle, refusals
def test_lifecycle_refusals_the_batched_abi_and_the_pumps_refusal_of_stream_53(gpu_required):
    nat = gpu_required
    lib = nat.lib()
    blk, K = 16000, 10                                            # 1920 dibits: the frames of the first 1032 are decided
    x = _noise(77, blk * K)
    LOOSE = _loose("fsk4", 16)                                    # some thirty hits in a thousand dibits of noise
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = fe.chan_open(CR, OFF)
        assert _code(nat, fe.chan_p25lc, c) == nat.RCF_ESTATE     # no slicer
        assert _code(nat, fe.chan_p25lc, c + 1000) == nat.RCF_ENOCHAN
        fe.chan_p25lc(c, on=False)                                # off without the stage: nothing to do
        fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
        fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_BINARY, sync_word=p25.FRAME_SYNC, sync_bits=48)
        assert _code(nat, fe.chan_p25lc, c) == nat.RCF_ESTATE     # not FSK4 mode
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, sync_word=0x2D6, sync_bits=10)
        assert _code(nat, fe.chan_p25lc, c) == nat.RCF_ESTATE     # not a 48-bit word
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=4, sync_both=1)
        assert _code(nat, fe.chan_p25lc, c) == nat.RCF_ESTATE     # both polarities
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **LOOSE)
        for cap in (8, 24, -16, (1 << 20) + 1):
            assert _code(nat, fe.chan_p25lc, c, cap) == nat.RCF_EINVAL
        for correct in (2, -1):
            assert _code(nat, fe.chan_p25lc, c, 0, correct) == nat.RCF_EINVAL
        # one frame decoder per slicer: each of the two P25 stages is refused while the other is attached
        fe.chan_tsbk(c)
        assert _code(nat, fe.chan_p25lc, c) == nat.RCF_ESTATE and _code(nat, fe.chan_p25lc_state, c) == nat.RCF_ESTATE
        fe.chan_tsbk(c, on=False)
        fe.chan_p25lc(c, 64)
        assert _code(nat, fe.chan_tsbk, c) == nat.RCF_ESTATE and _code(nat, fe.chan_tsbk_state, c) == nat.RCF_ESTATE
        assert fe.chan_p25lc_ring(c)[1] == 64 and fe.chan_p25lc_ring(c)[0]
        assert fe.chan_p25lc_state(c) == dict(n_records=0, n_frames=0, n_decoded=0, n_rs_bad=0, n_lost=0)
        for i in range(K):
            fe.push(x[i * blk:(i + 1) * blk])
        n1 = fe.chan_p25lc_state(c)["n_records"]
        assert n1 > 0
        first = fe.chan_slicer_state(c)["n_hits"]
        fe.chan_p25lc(c, correct=False)                           # again: afresh, from the hits that follow
        assert fe.chan_p25lc_ring(c)[1] == 256 and fe.chan_p25lc_state(c)["n_records"] == 0
        for i in range(K):
            fe.push(x[i * blk:(i + 1) * blk])
        # the raw batched ABI: 53 is a stream of 8-word records; 50 and 52 are none
        cid, cnt = (ctypes.c_int * 1)(c), (ctypes.c_int64 * 1)()
        buf = np.zeros(4 * 8, dtype=np.uint32)
        assert lib.rcf_chan_read_many(fe._h, nat.HARD_P25LC, cid, 1, 1.0, buf.ctypes.data_as(ctypes.c_void_p), 4, cnt) == nat.RCF_OK and cnt[0] == 4
        for none in (50, 52):
            assert lib.rcf_chan_read_many(fe._h, none, cid, 1, 1.0, buf.ctypes.data_as(ctypes.c_void_p), 4, cnt) == nat.RCF_EINVAL
        rows = fe.chan_read_many([c], "p25lc", cap_each=2)
        assert rows[0].dtype == nat.P25LC_DTYPE and len(rows[0]) == 2
        recs = np.concatenate([buf.view(nat.P25LC_DTYPE), rows[0], fe.chan_read_p25lc(c)])
        want, want_st = _want(fe, c, first_hit=first, correct=0)
        _same(recs, want, "afresh")
        assert fe.chan_p25lc_state(c) == want_st and len(recs) > 6
        # the pump does not deliver it: refused at start and at subscribe, as 48, 49 and 51 are
        ring = nat.PinnedArray(2 * 2 * blk, np.uint8)
        ring.array[:] = 127
        counter = np.zeros(1, dtype=np.uint64)
        grp = nat.Group([fe])
        try:
            assert _code(nat, nat.Pump, grp, [ring], blk, FS, (), fmt=nat.FMT_U8, what="p25lc", max_read=4, written=[counter],
                         start_delay_s=0.0) == nat.RCF_EINVAL
            pump = nat.Pump(grp, [ring], blk, FS, (), fmt=nat.FMT_U8, what="fsk4", max_read=4, written=[counter], start_delay_s=0.0)
            cur = ctypes.c_int64(0)
            assert lib.rcf_pump_subscribe(pump._p, 0, c, nat.HARD_P25LC, 1.0, ctypes.byref(cur)) == nat.RCF_EINVAL
            pump.stop()
        finally:
            grp.close()
            ring.free()
        fe.chan_p25lc(c, on=False)
        assert _code(nat, fe.chan_p25lc_state, c) == nat.RCF_ESTATE and _code(nat, fe.chan_p25lc_ring, c) == nat.RCF_ESTATE
        assert _code(nat, fe.chan_read_p25lc, c) == nat.RCF_ESTATE
        fe.chan_p25lc(c)
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **LOOSE)   # the slicer attached again: the stage went with the old one
        assert _code(nat, fe.chan_p25lc_state, c) == nat.RCF_ESTATE
        fe.chan_tsbk(c)                                           # ... and left no claim on the new one
        fe.chan_tsbk(c, on=False)
        fe.chan_p25lc(c)
        fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))              # the source loop attached again: slicer and stage go
        assert _code(nat, fe.chan_p25lc_state, c) == nat.RCF_ESTATE and _code(nat, fe.chan_slicer_state, c) == nat.RCF_ESTATE
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **LOOSE)
        fe.chan_p25lc(c)
        fe.chan_slicer(c, None)                                   # slicer off
        assert _code(nat, fe.chan_p25lc_state, c) == nat.RCF_ESTATE
        fe.push(x[:blk])                                          # and the front-end runs on without either
        fe.chan_close(c)
        assert _code(nat, fe.chan_p25lc, c) == nat.RCF_ENOCHAN
