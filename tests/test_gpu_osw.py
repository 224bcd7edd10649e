"""SmartNet OSWs on the GPU (rcf_chan_osw; osw.hip): the 84-bit framing with its lock counter, deinterleave, the parity
syndrome and its correction behind a channel's binary slicer.  include/rcf.h defines the stage, tests/osw_ref.py restates it.
The yardstick is always that restatement applied to the channel's OWN packed words and sync hits as the slicer's readers
deliver them (chan_read_hard / chan_read_sync): the stage is integer work on those two streams, so every comparison --
records, counters, state -- is of bits.  Carriers are 3600-baud 2-FSK from mm_ref.fsk2_carrier on 400 kS/s front-ends with
25 kS/s channels."""
import ctypes

import numpy as np
import pytest

import mm_ref as M
import osw_ref as O
from rcf import control, p25, synth

pytestmark = pytest.mark.gpu

FS, CR = 400e3, 12500                                          # 400 kS/s front-ends, 25 kS/s channels (decimation 16)
OFFS = (50000.0, -150000.0, 150000.0, -50000.0)                # four carriers, a channel's width and more apart
BAUD, DEV = 3600.0, 1200.0
BLK = 16 * 1000                                                # 1000 channel samples: 144 symbols
LEAD = 600                                                     # quiet bits for the clock to settle


def _code(nat, fn, *a, **kw):
    with pytest.raises(nat.RcfError) as e:
        fn(*a, **kw)
    return e.value.code


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, len(got), len(want), got[:3], want[:3])


def _carrier(bits, off=OFFS[0], seed=5):
    return M.fsk2_carrier(bits, BAUD, FS, off, DEV, np.random.default_rng(seed), noise=0.0)


def clean_bits(seed, n_frames=50):
    """LEAD quiet bits, n_frames back-to-back frames none of whose packets holds the sync word, a last sync word, quiet bits
    -> (bits, the messages sent)"""
    rng = np.random.default_rng(seed)
    parts, sent = [O.quiet(LEAD)], []
    for _ in range(n_frames):
        while True:
            m = O.random_osw(rng)
            f = O.frame(*m)
            if len(O.hits(np.concatenate([f, O.SYNC_LIST[:7]]))) == 1:
                break
        parts.append(f); sent.append(m)
    parts += [np.array(O.SYNC_LIST, np.uint8), O.quiet(420, 2)]
    return np.concatenate(parts), sent


@pytest.fixture(scope="module")
def clean():
    """four clean carriers of 50 frames each at OFFS, summed -> (x, per carrier the messages sent)"""
    made = [clean_bits(36 + n) for n in range(4)]
    x = sum(_carrier(b, off, seed=n) for n, ((b, _), off) in enumerate(zip(made, OFFS))).astype(np.complex64)
    return x, [s for _, s in made]


def _open(fe, off=OFFS[0], stage=True, **kw):
    c = fe.chan_open(CR, off)
    control.smartnet_clock(fe, c, hard=True)
    if stage:
        fe.chan_osw(c, **kw)
    return c


def _want(fe, c, **kw):
    """the restatement over everything the slicer's two readers deliver (the whole streams: nobody has read them before)"""
    by = fe.chan_read_hard(c)
    k, _ = fe.chan_read_sync(c)
    return O.run(by, k, **kw)


def _run(nat, x, pieces, attach_at=None, off=OFFS[0], trace=None, **stage):
    """the signal pushed in pieces -> (records, state, the restatement's records, its state, the channel's words and hits)"""
    with nat.Frontend(FS, device=0, block_capacity=max(b - a for a, b in zip(pieces[:-1], pieces[1:]))) as fe:
        c = _open(fe, off, stage=attach_at is None, **stage)
        at = dict(pos0=0, first_hit=0)
        for a, b in zip(pieces[:-1], pieces[1:]):
            if attach_at is not None and a == attach_at:
                s = fe.chan_slicer_state(c)
                at = dict(pos0=s["n_symbols"], first_hit=s["n_hits"])
                fe.chan_osw(c, **stage)
            fe.push(x[a:b])
        recs, st = fe.chan_read_osw(c), fe.chan_osw_state(c)
        assert len(fe.chan_read_osw(c)) == 0
        by = fe.chan_read_hard(c)
        k, _ = fe.chan_read_sync(c)
    want, want_st = O.run(by, k, trace=trace, **at)
    return recs, st, want, want_st, by, k, at


def _pieces(x, blk=8 * BLK):
    return list(range(0, len(x), blk)) + [len(x)]


# ------------------------------------------------------------------------------------------------ one channel
def test_every_sent_osw_is_recovered_on_a_clean_carrier_and_is_locked_reached(gpu_required, clean):
    nat = gpu_required
    x, sent = clean
    recs, st, want, want_st, by, k, _ = _run(nat, x, _pieces(x))
    _same(recs, want, "one channel")
    got = control.smartnet_osws(recs)
    print("clean: %s, first k %d" % (st, got[0][0]))
    assert st == want_st and st["n_lost"] == 0 and st["n_records"] == st["n_frames"] >= 50 and not np.any(nat.osw_fields(recs)["bad"][:50])
    assert [(g[3], g[2], g[1]) for g in got[:50]] == [(m[0], "G" if m[1] else "I", m[2]) for m in sent[0]]
    assert [g[7] for g in got[:50]] == [False] * 5 + [True] * 45 and np.diff([g[0] for g in got[:50]]).tolist() == [84] * 49
    assert recs["locked"][:50].tolist() == [0, 1, 2, 3, 4] + [5] * 45
    for rec, m in zip(recs[:50], sent[0]):                          # the 11 bits the reference does not interpret are delivered
        assert int("".join(str(b) for b in np.unpackbits(rec["data"])[27:38]), 2) == m[3]
    assert not np.any(recs["psyn"][:50]) and not np.any(recs["data"][:, 5:])


def test_designed_carrier_every_single_flip_and_adjacent_pair_with_its_census(gpu_required):
    """O.designed_bits as a noise-free carrier: on a locked stream one frame per single flip of the packet's 76 bits and per
    adjacent pair.  Records and state are the restatement's over the channel's own words and hits; per frame the syndrome
    flag, the number of corrected bits and the bits left wrong are what the rules demand of the planted pattern: every data
    bit 0 .. 36 corrected, bit 37 and every parity bit counted bad and left.  tests/test_osw_cpu.py holds the same on the
    planted bits."""
    nat = gpu_required
    bits, sent, starts, patterns = O.designed_bits()
    x = _carrier(bits)
    trace = []
    recs, st, want, want_st, by, k, _ = _run(nat, x, _pieces(x), trace=trace)
    _same(recs, want, "designed")
    assert st == want_st and st["n_lost"] == 0 and st["n_rejects"] == 0
    frames = [t for t in trace if t["kind"] == "frame"]
    first = next(i for i, t in enumerate(frames) if (np.diff([u["s"] for u in frames[i:i + len(starts)]]) == 84).all() and t["case"] == "B")
    frames, recs = frames[first:first + len(starts)], recs[first:first + len(starts)]
    assert len(frames) == len(starts) and all(t["locked"] == 5 and not t["rel_nz"] for t in frames[8:])
    f = nat.osw_fields(recs)
    corrected, uncorrected = set(), set()
    for n, (rec, m, p) in enumerate(zip(recs, sent, patterns)):
        bad, fixed, wrong = O.designed_expect(p)
        assert bool(f["bad"][n]) == bad and f["flipped"][n] == len(fixed), (n, p)
        data = np.unpackbits(rec["data"])[:38].tolist()
        was = [int(c) for c in "{0:016b}{1:01b}{2:010b}{3:011b}".format(m[0] ^ 0xcc38, m[1], m[2] ^ 0xd5, m[3])]
        assert {i for i in range(38) if data[i] != was[i]} == wrong, (n, p)
        if len(p) == 1:
            o = 4 * (p[0] % 19) + p[0] // 19
            (corrected if fixed else uncorrected).add(o // 2 if fixed else o)
    print("designed: %s, %d hits" % (st, len(k)))
    assert corrected == set(range(37)) and uncorrected == {74} | set(range(1, 76, 2)) and st["n_bad"] >= 151


def test_lock_carrier_with_its_census(gpu_required):
    """O.lock_bits as a noise-free carrier: locked from -4 to 5, jumps with clean and with broken packets, 3 -> 2 with the
    packet taken at the hit, frames taken blindly at the cursor, rejects, a sync word inside a packet locked and unlocked --
    the census is asserted on the restatement over the channel's own streams, and the stage equals it"""
    nat = gpu_required
    bits, planted, _ = O.lock_bits()
    x = _carrier(bits)
    recs, st, _, _, by, k, _ = _run(nat, x, _pieces(x))
    first = min(planted)
    hits = set((k - 7).tolist())
    shift = next(s for s in sorted(hits) if all(s + 84 * n in hits for n in range(8))) - first      # where the carrier's bit 0 came out
    want, want_st = O.lock_census(by, k, shift=shift)
    _same(recs, want, "lock carrier")
    print("lock carrier: %s, shift %d" % (st, shift))
    assert st == want_st and st["n_lost"] == 0 and recs["locked"].min() == -4 and recs["locked"].max() == 5


def test_records_do_not_depend_on_the_cuts(gpu_required):
    nat = gpu_required
    bits, _, _ = O.lock_bits()
    x = _carrier(bits)
    rng = np.random.default_rng(34)
    # random pieces, pieces of less than one channel sample (a block of 0 symbols), runs of pieces of one symbol (112 samples)
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 40)}
    cuts |= {16 * 9000 + 5 * j for j in range(1, 14)} | {16 * 12000 + 112 * j for j in range(60)} | {16 * 20000 + 16 * 30 * j for j in range(20)}
    cuts = sorted(cuts)
    one = _run(nat, x, [0, len(x)])
    ragged = _run(nat, x, cuts)
    _same(one[0], one[2], "one push"); _same(ragged[0], ragged[2], "ragged pushes")
    _same(ragged[0], one[0], "cuts")
    assert one[1] == one[3] == ragged[1] == ragged[3] and one[1]["n_records"] > 40 and one[1]["n_rejects"] >= 8


def test_attach_in_mid_frame(gpu_required, clean):
    nat = gpu_required
    x, sent = clean
    sps = FS / BAUD
    attach = int((LEAD + 84 * 10 + 40) * sps) // 16 * 16            # inside the eleventh frame, behind its sync word
    recs, st, want, want_st, by, k, at = _run(nat, x, [0, attach, len(x)], attach_at=attach, capacity=64)
    _same(recs, want, "late attach")
    got = control.smartnet_osws(recs)
    assert st == want_st and at["pos0"] > LEAD and at["first_hit"] >= 10 and recs["locked"][0] == 0
    assert [(g[3], g[1]) for g in got[:39]] == [(m[0], m[2]) for m in sent[0][11:]]        # from the twelfth frame on
    assert int(recs["k"][0]) - at["pos0"] == nat.osw_fields(recs)["rel"][0] > 0


# ------------------------------------------------------------------------------------------------ many channels, groups
def _kind_of(j):
    return "clock" if j in (0, 63, 64, 129) or j % 3 == 2 else ("fsk4", "costas")[j % 3]


def test_130_channels_of_mixed_kinds_one_launch_behind_the_slicers(gpu_required, clean):
    nat = gpu_required
    x, sent = clean
    K = 12
    x = x[:BLK * K]
    p25_search = dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=17, hit_capacity=4096)
    edacs = {5, 65, 128}                                          # clock channels with the EDACS stage behind a 48-bit search
    bare = {2, 68}                                                # a SmartNet slicer but no stage
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        cids = []
        for j in range(130):
            off = OFFS[j % 4] + 10.0 * (j // 4 - 16)              # the four carriers, each channel a little off tune
            if _kind_of(j) == "clock" and j in edacs:
                c = fe.chan_open(CR, off)
                control.edacs_clock(fe, c)
                fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_BINARY, sync_word=control.EDACS_SYNC, sync_bits=48, sync_max_errors=17, sync_both=1)
                fe.chan_edacs(c)
            elif _kind_of(j) == "clock":
                c = _open(fe, off, stage=j not in bare)
            else:
                c = fe.chan_open(CR, off)
                if _kind_of(j) == "fsk4":
                    fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
                    fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
                    fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **p25_search)
                    fe.chan_tsbk(c)
                else:
                    fe.chan_agc(c, 64, 1.0)
                    fe.chan_costas(c, **p25.costas_params(CR, 4800))
                    fe.chan_slicer(c, nat.READ_COSTAS, nat.SLICE_FSK4, **p25_search)
            cids.append(c)
        fe.timing_enable(True, classes=[nat.T_SLICE])
        for b in range(K):
            fe.push(x[b * BLK:(b + 1) * BLK])
        assert fe.timing_read(nat.T_SLICE)[1] == 4 * K            # the slicers' launch, the TSBK, the EDACS and the OSW stages'
        n_rec = n_chan = 0
        for j, c in enumerate(cids):
            if _kind_of(j) != "clock" or j in bare or j in edacs:
                assert _code(nat, fe.chan_read_osw, c) == nat.RCF_ESTATE and _code(nat, fe.chan_osw_state, c) == nat.RCF_ESTATE
                continue
            recs, st = fe.chan_read_osw(c), fe.chan_osw_state(c)
            want, want_st = _want(fe, c)
            _same(recs, want, ("lane", j))
            assert st == want_st and st["n_lost"] == 0 and len(recs) >= 8, (j, st, want_st)
            got = [(g[3], g[1]) for g in control.smartnet_osws(recs)]
            assert got[:8] == [(m[0], m[2]) for m in sent[j % 4][:8]], j                       # its own carrier's words, nobody else's
            n_rec += len(recs); n_chan += 1
        print("130 channels: %d records on %d channels" % (n_rec, n_chan))
        assert n_chan == sum(_kind_of(j) == "clock" for j in range(130)) - len(bare) - len(edacs) >= 40


def test_two_front_ends_in_a_group_and_the_group_reader_beside_the_single_one(gpu_required, clean):
    nat = gpu_required
    x, _ = clean
    K = 12
    xs = [x[:BLK * K], x[BLK // 2:BLK // 2 + BLK * K]]            # the second member sees the carriers half a block later
    fes = [nat.Frontend(FS, device=0, block_capacity=BLK) for _ in range(2)]
    try:
        ids = [[_open(fe, f) for f in OFFS[:3]] for fe in fes]
        fes[0].timing_enable(True, classes=[nat.T_SLICE])
        pairs = [(m, c) for m in range(2) for c in ids[m]]
        taken = [[] for _ in pairs]
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * BLK:(b + 1) * BLK] for xm in xs])
                if b >= 5:                                        # rcf_group_read_many, and the single reader first on two of them
                    for i in (1, 4):
                        taken[i].append(fes[pairs[i][0]].chan_read_osw(pairs[i][1], max_records=1))
                    rows = g.read_many(pairs, "osw", cap_each=64)
                    assert all(row is not None and row.dtype == nat.OSW_DTYPE for row in rows)
                    for i, row in enumerate(rows):
                        taken[i].append(row.copy())
            g.sync()
            assert fes[0].timing_read(nat.T_SLICE)[1] == 2 * K    # two launches per group block for both members
            total = 0
            for i, (m, c) in enumerate(pairs):
                assert len(fes[m].chan_read_osw(c)) == 0
                want, want_st = _want(fes[m], c)
                _same(np.concatenate(taken[i]), want, ("group", m, c))
                assert fes[m].chan_osw_state(c) == want_st
                total += len(want)
            print("group: %d records" % total)
            assert total > 8 * len(pairs)
    finally:
        for fe in fes:
            fe.close()


def test_read_many_over_64_channels_interleaved_with_the_single_readers(gpu_required, clean):
    nat = gpu_required
    x, _ = clean
    K = 12
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        cids = [_open(fe, OFFS[j % 4] + 10.0 * (j // 4 - 8)) for j in range(64)]
        taken = [[] for _ in cids]
        for b in range(K):
            fe.push(x[b * BLK:(b + 1) * BLK])
            if b % 2 and b >= 5:                                  # the batched reader, and on every fifth channel the single one first
                for i in range(0, 64, 5):
                    taken[i].append(fe.chan_read_osw(cids[i], max_records=1))
                for i, row in enumerate(fe.chan_read_many(cids, "osw", cap_each=32)):
                    assert row is not None and row.dtype == nat.OSW_DTYPE
                    taken[i].append(row.copy())
        total = 0
        for i, c in enumerate(cids):
            taken[i].append(fe.chan_read_osw(c))
            want, _ = _want(fe, c)
            _same(np.concatenate(taken[i]), want, ("channel", i))
            total += len(want)
        print("read_many: %d records" % total)
        assert total > 8 * 64 and fe.chan_read_many(cids[:2], "osw", cap_each=4)[0].shape == (0,)


# ------------------------------------------------------------------------------------------------ small rings
def test_record_ring_of_16_wraps_and_a_reader_left_behind_loses_the_oldest(gpu_required, clean):
    nat = gpu_required
    x, _ = clean
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe, nat.Frontend(FS, device=0, block_capacity=BLK) as tw:
        c, c_t = _open(fe, capacity=16), _open(tw, capacity=1024)
        assert fe.chan_osw_ring(c)[1] == 16 and tw.chan_osw_ring(c_t)[1] == 1024 and fe.chan_osw_ring(c)[0]
        cursor = lost = 0
        n_blocks = len(x) // BLK
        for b in range(n_blocks):
            fe.push(x[b * BLK:(b + 1) * BLK]); tw.push(x[b * BLK:(b + 1) * BLK])
            if b % 16 != 15 and b != n_blocks - 1:                # every sixteenth block: about 27 records
                continue
            n = tw.chan_osw_state(c_t)["n_records"]
            assert fe.chan_osw_state(c)["n_records"] == n
            got = fe.chan_read_osw(c)
            first = max(cursor, n - 16)
            lost += first - cursor
            cursor = n
            whole = tw.chan_read_osw(c_t)                         # the twin's reader never lags: the stream's new records
            _same(got, whole[len(whole) - (n - first):], ("block", b))
        want, _ = _want(tw, c_t)
        assert lost >= 10 and len(want) == cursor >= 50


def test_a_hit_ring_of_16_loses_hits_and_they_are_counted(gpu_required):
    """random bits under the exact 8-bit search hit once in 256 bits; pushes of 6000 symbols bring about 23 such hits each, and
    seven planted ones, to a ring of 16: about 14 leave it unexamined per push.  n_lost and the records are the restatement's, which walks the whole streams -- from a twin with a large hit ring --
    launch by launch; the planted frames among the last 16 hits of a push are still decoded"""
    nat = gpu_required
    rng = np.random.default_rng(17)
    bits = rng.integers(0, 2, 6 * 6000).astype(np.uint8)
    for n in range(6):                                            # six frames back to back at the end of every push's symbols
        for q in range(6):
            at = 6000 * (n + 1) - 700 + 84 * q
            bits[at:at + 84] = O.frame(*O.random_osw(rng))
    x = _carrier(bits)
    blk = len(x) // 6
    launches, parts = [], []
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe, nat.Frontend(FS, device=0, block_capacity=blk) as tw:
        c, c_t = fe.chan_open(CR, OFFS[0]), _open(tw, stage=False)
        fe.chan_clock_mm(c, 2 * CR / BAUD, control.GAIN_OMEGA, control.MU, control.GAIN_MU, control.OMEGA_RELATIVE_LIMIT, control.QUAD_GAIN)
        fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_BINARY, sync_word=control.SMARTNET_SYNC, sync_bits=8, hit_capacity=16)
        fe.chan_osw(c)
        for b in range(6):
            fe.push(x[b * blk:(b + 1) * blk]); tw.push(x[b * blk:(b + 1) * blk])
            s = fe.chan_slicer_state(c)
            launches.append((s["n_words"], s["n_hits"]))
            parts.append(fe.chan_read_osw(c))
        st = fe.chan_osw_state(c)
        assert fe.chan_slicer_state(c) == tw.chan_slicer_state(c_t)
        by = tw.chan_read_hard(c_t)
        k, _ = tw.chan_read_sync(c_t)
    want, want_st = O.run(by, k, launches=launches, hit_cap=16)
    whole, whole_st = O.run(by, k)
    _same(np.concatenate(parts), want, "hit ring of 16")
    print("hit ring of 16: %d hits, %s; with a ring that loses nothing %s" % (len(k), st, whole_st))
    assert st == want_st and st["n_lost"] > 30 and st["n_records"] >= 4 and whole_st["n_lost"] == 0


# ------------------------------------------------------------------------------------------------ lifecycle, refusals
def test_lifecycle_refusals_and_the_pumps_refusal_of_stream_51(gpu_required, clean):
    nat = gpu_required
    lib = nat.lib()
    x, _ = clean
    B = nat.SLICE_BINARY
    S8 = dict(sync_word=control.SMARTNET_SYNC, sync_bits=8)
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        c = fe.chan_open(CR, OFFS[0])
        assert _code(nat, fe.chan_osw, c) == nat.RCF_ESTATE       # no slicer
        assert _code(nat, fe.chan_osw, c + 1000) == nat.RCF_ENOCHAN
        fe.chan_osw(c, on=False)                                  # off without the stage: nothing to do
        control.smartnet_clock(fe, c)
        fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_FSK4, sync_word=control.SMARTNET_SYNC, sync_bits=8)
        assert _code(nat, fe.chan_osw, c) == nat.RCF_ESTATE       # wrong slicer mode
        fe.chan_slicer(c, nat.READ_CLOCK, B, sync_word=control.EDACS_SYNC, sync_bits=48)
        assert _code(nat, fe.chan_osw, c) == nat.RCF_ESTATE       # a 48-bit word
        fe.chan_edacs(c)                                          # (that slicer is the EDACS stage's)
        fe.chan_slicer(c, nat.READ_CLOCK, B, sync_max_errors=1, **S8)
        assert _code(nat, fe.chan_osw, c) == nat.RCF_ESTATE       # sync_max_errors > 0
        fe.chan_slicer(c, nat.READ_CLOCK, B, sync_both=1, **S8)
        assert _code(nat, fe.chan_osw, c) == nat.RCF_ESTATE       # sync_both = 1
        fe.chan_slicer(c, nat.READ_CLOCK, B)
        assert _code(nat, fe.chan_osw, c) == nat.RCF_ESTATE       # no search at all
        fe.chan_slicer(c, nat.READ_CLOCK, B, **S8)
        fe.chan_osw(c)
        assert _code(nat, fe.chan_edacs, c) == nat.RCF_ESTATE and _code(nat, fe.chan_tsbk, c) == nat.RCF_ESTATE    # a second stage on this slicer
        assert _code(nat, fe.chan_read_edacs, c) == nat.RCF_ESTATE
        fe.chan_slicer(c, nat.READ_CLOCK, B, **S8)
        assert _code(nat, fe.chan_osw_state, c) == nat.RCF_ESTATE                        # the slicer attached again: the stage went with the old one
        for cap in (8, 24, -16, (1 << 20) + 1):
            assert _code(nat, fe.chan_osw, c, cap) == nat.RCF_EINVAL
        fe.chan_osw(c, 64)
        assert fe.chan_osw_ring(c)[1] == 64 and fe.chan_osw_state(c) == O.STATE0
        for b in range(12):
            fe.push(x[b * BLK:(b + 1) * BLK])
        st = fe.chan_osw_state(c)
        assert st["n_records"] > 8 and st["locked"] == 5 and st["is_locked"] == 1
        s = fe.chan_slicer_state(c)
        fe.chan_osw(c)                                            # again: afresh, locked = 0, from the bits that follow
        assert fe.chan_osw_ring(c)[1] == 256 and fe.chan_osw_state(c) == O.STATE0
        for b in range(12, 20):
            fe.push(x[b * BLK:(b + 1) * BLK])
        recs = fe.chan_read_osw(c)
        want, want_st = _want(fe, c, pos0=s["n_symbols"], first_hit=s["n_hits"])
        _same(recs, want, "afresh")
        assert fe.chan_osw_state(c) == want_st and len(recs) > 5 and recs["locked"][:3].tolist() == [0, 1, 2]
        # the raw batched ABI: 51 is a stream of 8-word records; 50 and 52 are none
        cid, cnt = (ctypes.c_int * 1)(c), (ctypes.c_int64 * 1)()
        buf = np.zeros(16 * 8, dtype=np.uint32)
        assert lib.rcf_chan_read_many(fe._h, nat.HARD_OSW, cid, 1, 1.0, buf.ctypes.data_as(ctypes.c_void_p), 16, cnt) == nat.RCF_OK and cnt[0] == 0
        for none in (50, 52):
            assert lib.rcf_chan_read_many(fe._h, none, cid, 1, 1.0, buf.ctypes.data_as(ctypes.c_void_p), 16, cnt) == nat.RCF_EINVAL
        # the pump does not deliver it: refused at start and at subscribe, as 32, 33, 48 and 49 are
        ring = nat.PinnedArray(2 * 2 * BLK, np.uint8)
        ring.array[:] = 127
        counter = np.zeros(1, dtype=np.uint64)
        grp = nat.Group([fe])
        try:
            assert _code(nat, nat.Pump, grp, [ring], BLK, FS, (), fmt=nat.FMT_U8, what="osw", max_read=4, written=[counter],
                         start_delay_s=0.0) == nat.RCF_EINVAL
            pump = nat.Pump(grp, [ring], BLK, FS, (), fmt=nat.FMT_U8, what="clock", max_read=4, written=[counter], start_delay_s=0.0)
            cur = ctypes.c_int64(0)
            for what in (nat.HARD_OSW, nat.HARD_EDACS):
                assert lib.rcf_pump_subscribe(pump._p, 0, c, what, 1.0, ctypes.byref(cur)) == nat.RCF_EINVAL, what
            pump.stop()
        finally:
            grp.close()
            ring.free()
        fe.chan_osw(c, on=False)
        assert _code(nat, fe.chan_osw_state, c) == nat.RCF_ESTATE and _code(nat, fe.chan_osw_ring, c) == nat.RCF_ESTATE
        fe.chan_osw(c)
        control.smartnet_clock(fe, c)                             # the source loop attached again: slicer and stage go
        assert _code(nat, fe.chan_osw_state, c) == nat.RCF_ESTATE and _code(nat, fe.chan_slicer_state, c) == nat.RCF_ESTATE
        control.smartnet_clock(fe, c, hard=True, osw=True)        # the helper: clock, slicer, stage
        assert fe.chan_osw_ring(c)[1] == 256
        fe.chan_slicer(c, None)                                   # slicer off
        assert _code(nat, fe.chan_osw_state, c) == nat.RCF_ESTATE
        fe.push(x[:BLK])                                          # and the front-end runs on without either
        fe.chan_close(c)
        assert _code(nat, fe.chan_osw, c) == nat.RCF_ENOCHAN
