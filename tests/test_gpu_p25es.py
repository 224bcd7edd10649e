"""The options of the P25 voice stage on the GPU (rcf_chan_p25lc_opt; p25lc.hip): LDU2's encryption sync as a unit of kind 4
and the inner words given up as erasures of the Reed-Solomon decoders.  include/rcf.h defines them, tests/p25es_ref.py
restates them on top of tests/p25lc_ref.py.  As in tests/test_gpu_p25lc.py the yardstick is always that restatement applied
to the channel's OWN packed words and sync hits as the slicer's readers deliver them (chan_read_hard / chan_read_sync), and
every comparison -- records, counters -- is of bits.  One 400 kS/s front-end, 25 kS/s channels, 4800 baud."""
import ctypes

import numpy as np
import pytest

import fsk4_ref as F
import p25es_ref as E
import p25lc_ref as R
import tsbk_ref as T
from rcf import p25, synth

pytestmark = pytest.mark.gpu

FS, CR, OFF = F.FS, F.CHANNEL_RATE, F.CHANNEL_OFFSET
BLK = 16 * 1000
NAC = R.CALL["nac"]
# (correct, es, erasures) of the mixed launches; None: a TSBK stage
MIX = ((1, False, False), (1, True, False), (1, True, True), (0, True, False), None)


def _options(es, erasures):
    return (E.ES if es else 0) | (E.ERASURES if erasures else 0)


def _noise(seed, n, amp=0.05):
    return (amp * synth.awgn(np.random.default_rng(seed), n)).astype(np.complex64)


def _code(nat, fn, *a, **kw):
    with pytest.raises(nat.RcfError) as e:
        fn(*a, **kw)
    return e.value.code


def _want(fe, c, **kw):
    """the restatement over everything the slicer's two readers deliver (the whole streams: nobody has read them before)"""
    by = fe.chan_read_hard(c)
    k, dist = fe.chan_read_sync(c)
    return E.run(by, k, dist, **kw)


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, len(got), len(want), got[:4], want[:4])


def _loose(errors):
    return dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=errors, hit_capacity=4096)


def _open(nat, fe, f, mix, search, capacity=0):
    """a channel at offset f behind the C4FM loop and a slicer with this search; mix: an entry of MIX"""
    c = fe.chan_open(CR, f)
    fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
    fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
    fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **search)
    if mix is None:
        fe.chan_tsbk(c)
    else:
        fe.chan_p25lc(c, capacity, correct=bool(mix[0]), es=mix[1], erasures=mix[2])
    return c


@pytest.fixture(scope="module")
def call():
    """E.call_dibits as one 4800-baud C4FM carrier at the channel's offset, 150 Hz off -> (x, the frames' starts, their names)"""
    d, starts, shorts = E.call_dibits()
    return F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0), starts, shorts


def _run_call(nat, x, pieces, correct, es=True, erasures=False, attach_at=None):
    """the carrier pushed in pieces -> (records, state, restatement's records, its state)"""
    with nat.Frontend(FS, device=0, block_capacity=max(b - a for a, b in zip(pieces[:-1], pieces[1:]))) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, lc=attach_at is None and bool(correct), es=es, erasures=erasures)
        if attach_at is None and not correct:
            fe.chan_p25lc(c, correct=False, es=es)
        first = 0
        for a, b in zip(pieces[:-1], pieces[1:]):
            if attach_at is not None and a == attach_at:
                first = fe.chan_slicer_state(c)["n_hits"]
                fe.chan_p25lc(c, correct=bool(correct), es=es, erasures=erasures)
            fe.push(x[a:b])
        recs, st = fe.chan_read_p25lc(c), fe.chan_p25lc_state(c)
        want, want_st = _want(fe, c, first_hit=first, correct=correct, options=_options(es, erasures))
    return recs, st, want, want_st


# ------------------------------------------------------------------------------------------------ one channel, a call
@pytest.mark.parametrize("correct", [1, 0])
def test_a_call_with_encryption_sync_whole_ragged_and_block_by_block(gpu_required, call, correct):
    nat = gpu_required
    x, starts, shorts = call
    rng = np.random.default_rng(34)
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 40)}
    cuts |= {16 * 4000 + 5 * j for j in range(1, 14)} | {16 * 6000 + 84 * j for j in range(40)} | {16 * 9000 + 16 * 30 * j for j in range(20)}
    whole = _run_call(nat, x, [0, len(x)], correct)
    ragged = _run_call(nat, x, sorted(cuts), correct)
    blocks = _run_call(nat, x, list(range(0, len(x), BLK)) + [len(x)], correct)
    for name, r in (("whole", whole), ("ragged", ragged), ("blocks", blocks)):
        _same(r[0], r[2], name)
        assert r[1] == r[3], name
    _same(ragged[0], whole[0], "cuts"); _same(blocks[0], whole[0], "blocks")
    assert whole[1] == dict(n_records=8, n_frames=8, n_decoded=8, n_rs_bad=0, n_lost=0)
    units = p25.voice_units(whole[0])
    print("call (correct=%d): %s" % (correct, [(u["short"], u["k"], u["n_rs"], u["n_fixed"]) for u in units]))
    c = E.CALL_ES
    assert [u["short"] for u in units] == shorts and all(u["nac"] == NAC and u["dist"] == 0 and u["decoded"] for u in units)
    assert np.diff([u["k"] for u in units]).tolist() == np.diff(starts).tolist()
    ldu2 = [u for u in units if u["short"] == "LDU2"]
    for u in ldu2 if correct else (ldu2[0], ldu2[2]):              # the second LDU2 carries errors that only the decoders remove
        assert (u["mi"], u["algid"], u["kid"], u["lsd"]) == (c["mi"], c["algid"], c["kid"], c["lsd2"])
    assert (units[0]["mi"], units[0]["algid"], units[0]["kid"]) == (c["mi"], c["algid"], c["kid"])
    if correct:
        assert [(u["n_rs"], u["n_fixed"], u["n_bad"], u["rs_bad"]) for u in ldu2] == [(0, 0, 0, 0), (1, 3, 0, 0), (0, 0, 0, 0)]
    else:
        assert not any(u["n_rs"] or u["n_fixed"] or u["n_bad"] or u["rs_bad"] for u in units) and ldu2[1]["mi"] != c["mi"]
    # es=False on the same carrier: the parent's records -- p25lc_ref's restatement itself is the yardstick here
    with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
        ch = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, lc=bool(correct))
        if not correct:
            fe.chan_p25lc(ch, correct=False)
        fe.push(x)
        recs, st = fe.chan_read_p25lc(ch), fe.chan_p25lc_state(ch)
        by = fe.chan_read_hard(ch)
        k, dist = fe.chan_read_sync(ch)
    want, want_st = R.run(by, k, dist, correct=correct)
    _same(recs, want, "es=False")
    assert st == want_st == dict(n_records=8, n_frames=8, n_decoded=5, n_rs_bad=0, n_lost=0)
    f, g = nat.p25lc_fields(recs), nat.p25lc_fields(whole[0])
    other = f["duid"] != 0xA
    assert f["kind"][~other].tolist() == [3, 3, 3] and g["kind"][~other].tolist() == [4, 4, 4] and recs[other].tobytes() == whole[0][other].tobytes()


# ------------------------------------------------------------------------------------------------ designed erasures
def test_designed_carrier_sits_on_and_beyond_every_bound(gpu_required):
    """E.designed_dibits as a noise-free C4FM carrier under the strict search, on one channel with both options and on a twin
    with es alone: LDU2s with (|E|, v) = (0,4), (2,3), (4,2), (6,1), (8,0) and, beyond the bound, (0,5), (1,4), (9,0); LDU1s,
    HDUs and TLCs on their own bound's edge, among them an HDU with 16 erasures and n_rs = 16 and TLCs with four-error (24,12)
    words.  Records and counters are the restatement's over each channel's own words and hits; the census over those says that
    the kernel met every class the input was built for and lost no frame.  tests/test_p25es_cpu.py holds the same census on
    the planted dibits."""
    nat = gpu_required
    d, plan = E.designed_dibits(NAC)
    x = F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0)
    blk = 4 * BLK
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, lc=True, es=True, erasures=True)
        c_p = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, lc=True, es=True)
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk])
        recs, st = fe.chan_read_p25lc(c), fe.chan_p25lc_state(c)
        plain, plain_st = fe.chan_read_p25lc(c_p), fe.chan_p25lc_state(c_p)
        k, dist = fe.chan_read_sync(c)
        by = fe.chan_read_hard(c)
        want_p, want_p_st = _want(fe, c_p, options=E.ES)
    want, want_st = E.run(by, k, dist, options=E.ES | E.ERASURES)
    f = nat.p25lc_fields(recs)
    print("designed: %d hits, %s, es alone %s; n_rs %s, n_bad %s" % (len(k), st, plain_st, f["n_rs"].tolist(), f["n_bad"].tolist()))
    _same(recs, want, "designed")
    _same(plain, want_p, "designed, es alone")
    assert st == want_st == dict(n_records=25, n_frames=25, n_decoded=25, n_rs_bad=9, n_lost=0) and plain_st == want_p_st
    starts = [p["start"] for p in plan]
    assert len(k) == len(starts) and not np.any(dist) and np.diff(k).tolist() == np.diff(starts).tolist()
    shift = int(k[0]) - 23 - starts[0]
    E.check_census(want, want_p, [dict(p, start=p["start"] + shift) for p in plan])


# ------------------------------------------------------------------------------------------------ many channels, groups
def test_130_channels_of_mixed_options_in_one_launch(gpu_required):
    """noise under 130 channels that search it loosely: voice stages without options, with es, with es and erasures, in the
    uncorrected mode with es, and TSBK stages, in turn -- one launch of the voice stages per block whatever their options.
    Channel 7's record ring holds 16 and its reader comes once, at the end: the last 16.  On every fifth channel the single
    reader takes three records before the batched reader takes the rest"""
    nat = gpu_required
    blk, K = 16000, 14                                             # 192 symbols a block; a frame is decided 888 dibits late
    x = _noise(132, blk * K)
    offs = [-190000.0 + 2900.0 * j for j in range(130)]
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [_open(nat, fe, f, MIX[j % 5], _loose(16 if j == 7 else 14 - j % 3), capacity=16 if j == 7 else 0) for j, f in enumerate(offs)]
        voice = [j for j in range(130) if MIX[j % 5] is not None and j != 7]
        fe.timing_enable(True, classes=[nat.T_SLICE])
        taken = {j: [] for j in voice}
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk])
            if b % 3 == 2:
                for j in voice[::5]:
                    taken[j].append(fe.chan_read_p25lc(cids[j], max_records=3))
                for j, row in zip(voice, fe.chan_read_many([cids[j] for j in voice], "p25lc", cap_each=64)):
                    assert row is not None and row.dtype == nat.P25LC_DTYPE
                    taken[j].append(row.copy())
        assert fe.timing_read(nat.T_SLICE)[1] == 3 * K             # the slicers, the TSBK stages, the voice stages
        kinds = np.zeros(5, int)
        n_rec = n_er = 0
        for j, c in enumerate(cids):
            if MIX[j % 5] is None:
                by = fe.chan_read_hard(c)
                k, dist = fe.chan_read_sync(c)
                want, want_st = T.run(by, k, dist)
                _same(fe.chan_read_tsbk(c), want, ("tsbk", j))
                assert fe.chan_tsbk_state(c) == want_st
                continue
            correct, es, erasures = MIX[j % 5]
            got = fe.chan_read_p25lc(c) if j == 7 else np.concatenate(taken[j] + [fe.chan_read_p25lc(c)])
            st = fe.chan_p25lc_state(c)
            want, want_st = _want(fe, c, correct=correct, options=_options(es, erasures))
            assert st == want_st and st["n_lost"] == 0, (j, st, want_st)
            if j == 7:
                assert len(want) > 16
                want = want[-16:]
            _same(got, want, ("lane", j))
            f = nat.p25lc_fields(got)
            kinds += np.bincount(f["kind"], minlength=5)
            assert es or not np.any(f["kind"] == 4)
            n_rec += len(got)
            n_er += int(np.sum(f["n_bad"][f["kind"] != 3] > 0)) if erasures else 0
    print("130 channels: %d voice records, kinds %s, %d units with erased words" % (n_rec, kinds.tolist(), n_er))
    assert n_rec > 104 and kinds[4] > 0 and kinds[:3].sum() > 0


def test_two_front_ends_in_a_group_with_mixed_options(gpu_required):
    """a group's block: three voice stages with different options and a TSBK stage on each member, the group's reader
    interleaved with the single one"""
    nat = gpu_required
    blk, K = 16000, 14
    xs = [_noise(50 + m, blk * K) for m in range(2)]
    offs = (-100000.0, 60000.0, 150000.0, -30000.0)
    fes = [nat.Frontend(FS, device=0, block_capacity=blk) for _ in range(2)]
    try:
        mix = [[MIX[(j + 2 * m) % 4] for j in range(3)] + [None] for m in range(2)]
        ids = [[_open(nat, fe, f, mix[m][j], _loose(13)) for j, f in enumerate(offs)] for m, fe in enumerate(fes)]
        pairs = [(m, ids[m][j]) for m in range(2) for j in range(3)]
        taken = {p: [] for p in pairs}
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * blk:(b + 1) * blk] for xm in xs])
                if b % 4 == 3:
                    m, c = pairs[b % len(pairs)]
                    taken[(m, c)].append(fes[m].chan_read_p25lc(c, max_records=2))
                    for p, row in zip(pairs, g.read_many(pairs, "p25lc", cap_each=64)):
                        assert row is not None and row.dtype == nat.P25LC_DTYPE
                        taken[p].append(row.copy())
            g.sync()
            total = 0
            for n, (m, c) in enumerate(pairs):
                correct, es, erasures = mix[m][n % 3]
                got = np.concatenate(taken[(m, c)] + [fes[m].chan_read_p25lc(c)])
                want, want_st = _want(fes[m], c, correct=correct, options=_options(es, erasures))
                _same(got, want, ("group", m, c))
                assert fes[m].chan_p25lc_state(c) == want_st
                total += len(want)
            for m in range(2):
                by = fes[m].chan_read_hard(ids[m][3])
                k, dist = fes[m].chan_read_sync(ids[m][3])
                _same(fes[m].chan_read_tsbk(ids[m][3]), T.run(by, k, dist)[0], ("group tsbk", m))
            print("group: %d voice records" % total)
            assert total > len(pairs)
    finally:
        for fe in fes:
            fe.close()


# ------------------------------------------------------------------------------------------------ lifecycle
def test_lifecycle_refusals_afresh_with_other_options_mid_frame_and_a_short_ldu2(gpu_required, call):
    nat = gpu_required
    lib = nat.lib()
    x, starts, shorts = call
    with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True)
        p = nat.P25lcParams(capacity=0, correct=1)
        p0 = nat.P25lcParams(capacity=0, correct=0)
        for options in (4, 8, 0x80000000, 7):
            assert lib.rcf_chan_p25lc_opt(fe._h, c, ctypes.byref(p), options) == nat.RCF_EINVAL       # an unknown option bit
        assert lib.rcf_chan_p25lc_opt(fe._h, c, ctypes.byref(p0), nat.P25LC_ERASURES) == nat.RCF_EINVAL     # erasures need correct = 1
        assert _code(nat, fe.chan_p25lc, c, correct=False, erasures=True) == nat.RCF_EINVAL
        assert _code(nat, fe.chan_p25lc, c, correct=False, es=True, erasures=True) == nat.RCF_EINVAL
        assert _code(nat, fe.chan_p25lc_state, c) == nat.RCF_ESTATE                                 # none of them attached a stage
        assert lib.rcf_chan_p25lc_opt(fe._h, c, None, 99) == nat.RCF_OK                               # off: nothing to do
        assert _code(nat, fe.chan_p25lc, c + 1000, es=True) == nat.RCF_ENOCHAN
        fe.chan_tsbk(c)
        assert _code(nat, fe.chan_p25lc, c, es=True) == nat.RCF_ESTATE
        fe.chan_tsbk(c, on=False)
        # attached in mid-frame, inside the first LDU1: the first LDU2 is the first to appear
        attach = int((starts[1] + 100) * FS / 4800.0) // 16 * 16
        fe.push(x[:attach])
        first = fe.chan_slicer_state(c)["n_hits"]
        fe.chan_p25lc(c, es=True, erasures=True)
        # ... and attached again with other options inside the third LDU1: afresh, the third LDU2 is the first
        again = int((starts[5] + 100) * FS / 4800.0) // 16 * 16
        fe.push(x[attach:again])
        mid, mid_st = fe.chan_read_p25lc(c), fe.chan_p25lc_state(c)
        at = fe.chan_slicer_state(c)
        second = at["n_hits"]
        fe.chan_p25lc(c, 64, correct=False, es=True)
        assert fe.chan_p25lc_ring(c)[1] == 64 and fe.chan_p25lc_state(c)["n_records"] == 0
        fe.push(x[again:])
        recs, st = fe.chan_read_p25lc(c), fe.chan_p25lc_state(c)
        by = fe.chan_read_hard(c)
        k, dist = fe.chan_read_sync(c)
    assert first >= 2 and second >= 6
    want_mid, want_mid_st = E.run(by, k, dist, options=3, first_hit=first, launches=[(at["n_words"], second)])   # what the first stage saw
    _same(mid, want_mid, "mid-frame")
    assert mid_st == want_mid_st and [u["short"] for u in p25.voice_units(mid)] == shorts[2:2 + len(mid)] and 2 <= len(mid) <= 3
    want, want_st = E.run(by, k, dist, correct=0, options=E.ES, first_hit=second)
    _same(recs, want, "afresh")
    assert st == want_st
    assert [u["short"] for u in p25.voice_units(recs)] == shorts[6:] and all(u["decoded"] for u in p25.voice_units(recs))
    # an LDU2 that the next frame's sync cuts at 788 dibits: a frame record, with es as without
    rng = np.random.default_rng(8)
    es = E.es_octets(bytes(9), 0x80, 1)
    d = np.concatenate([R.settle_dibits(), E.unit_frame(NAC, E.LDU2, es, rng)[:788], E.unit_frame(NAC, E.LDU2, es, rng, lsd=bytes(4)),
                        rng.integers(0, 4, 888).astype(np.uint8)])
    xs = F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0)
    with nat.Frontend(FS, device=0, block_capacity=len(xs)) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, lc=True, es=True, erasures=True)
        fe.push(xs)
        recs = fe.chan_read_p25lc(c)
        want, want_st = _want(fe, c, options=3)
    _same(recs, want, "short")
    units = p25.voice_units(recs)
    assert [(u["short"], u["frame_dibits"], u["decoded"]) for u in units] == [("LDU2", 788, False), ("LDU2", 864, True)]
    assert bytes(recs["payload"][0]) == bytes(16) and (units[1]["algid"], units[1]["kid"]) == (0x80, 1)
