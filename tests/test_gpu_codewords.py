"""Dense code words through the wave-form decoders on the GPU: rs_decode<false> and rs_decode<true> (p25lc.hip) and
nid_decode_wave (nid_wave.hpp) meet the streams of tests/codewords_ref.py -- every (|E|, v) pair inside the bound of all four
Reed-Solomon code paths, every symbol position as an error's and as an erasure's, both ends of the word, right erasures, full
weight; every single wrong NID bit, a dozen patterns per weight 2 .. 13 and bursts at both ends.  As in the sibling suites
the yardstick is the numpy restatement (p25es_ref, nid_ref, tsbk_ref) applied to the channel's OWN packed words and sync hits,
bit for bit; the censuses then say that the kernels met every class the input was built for.  tests/test_codewords_cpu.py holds
the same censuses on the planted dibits.
The carriers are noise-free 4800-baud C4FM on a 50 kS/s front end: a direct channel of chan_open(12500, ...) is 25 kS/s at any
front-end rate with fs / 12500 even, and synthesis costs 16 float64 passes over the samples -- 50 kS/s is the lowest such rate
and an eighth of the sibling suites' 400 kS/s."""
import numpy as np
import pytest

import codewords_ref as CW
import fsk4_ref as F
import nid_ref as N
import p25es_ref as E
import p25lc_ref as R
import tsbk_ref as T
from rcf import p25

pytestmark = pytest.mark.gpu

FS, CR, OFF = 50e3, F.CHANNEL_RATE, 6000.0
BLK = 64000
NAC = R.CALL["nac"]
BOTH = E.ES | E.ERASURES
NO_NID = dict(n_decoded=0, n_fixed=0, n_bits=0, n_bad=0)


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, len(got), len(want), got[:4], want[:4])


def _carrier(d):
    return F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0)


def _open(nat, fe, stage, nid=False, erasures=True):
    """a channel at OFF behind the C4FM loop, the strict search with rings that hold a whole dense stream, and a stage"""
    c = p25.c4fm_front_half(fe, fe.chan_open(CR, OFF), CR, 4800)
    fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
    fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, p25.SLICER_LEVELS, p25.FRAME_SYNC, p25.FRAME_SYNC_BITS, p25.FRAME_SYNC_MAX_ERRORS, hit_capacity=4096)
    if stage == "tsbk":
        fe.chan_tsbk(c, 1024, nid=nid)
    else:
        fe.chan_p25lc_ex(c, 1024, es=True, erasures=erasures, nid=nid)
    return c


def _streams(fe, c):
    by = fe.chan_read_hard(c)
    k, dist = fe.chan_read_sync(c)
    return by, k, dist


def _pieces(n, step):
    return list(range(0, n, step)) + [n]


def _ragged(n, seed):
    """cuts of at most BLK samples: random ones, runs of pushes of under one symbol (10.4 samples) and of a symbol or two"""
    rng = np.random.default_rng(seed)
    cuts = set(_pieces(n, BLK - 1)) | {int(v) for v in rng.integers(1, n, 60)}
    cuts |= {300000 + 3 * j for j in range(1, 14)} | {700000 + 21 * j for j in range(40)} | {1100000 + 16 * 30 * j for j in range(20)}
    return sorted(v for v in cuts if v <= n)


def _run_rs(nat, x, pieces):
    """the carrier pushed in pieces under two channels -> per channel (records, state, words, k, dist): the voice stage with
    es and erasures, and a twin with es alone"""
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        chans = [_open(nat, fe, "voice", erasures=True), _open(nat, fe, "voice", erasures=False)]
        for a, b in zip(pieces[:-1], pieces[1:]):
            fe.push(x[a:b])
        return [(fe.chan_read_p25lc(c), fe.chan_p25lc_state(c)) + _streams(fe, c) for c in chans]


@pytest.fixture(scope="module")
def dense_rs(gpu_required):
    """CW.dense_rs_dibits as one carrier -> (x, plan, the whole-stream run of _run_rs)"""
    d, plan = CW.dense_rs_dibits(NAC)
    x = _carrier(d)
    return x, plan, _run_rs(gpu_required, x, _pieces(len(x), BLK))


# ------------------------------------------------------------------------------------------------ Reed-Solomon
def test_dense_reed_solomon_words_on_two_stages(gpu_required, dense_rs):
    """302 units back to back: per code path (HDU: RS(36,20,17) behind (18,6) words; LDU1: RS(24,12,13) behind Hamming words;
    TLC: the same code behind (24,12) words, two symbols a word; LDU2: RS(24,16,9)) every (|E|, v) inside the bound -- 183
    units --, right erasures, two errors at j and j + n / 2 for every j, erasures over every position with symbols 0 and
    n - 1 in one unit, t errors at either end, and every pair just beyond the bound.  One workgroup decodes them on the
    channel with es and erasures (rs_decode<true>), the twin with es alone (rs_decode<false>).  Records and state are the
    restatement's over each channel's own words and hits; every planted frame is found at distance 0; the census over the
    restatement's records demands every class and lets nothing be skipped"""
    nat = gpu_required
    x, plan, ((recs, st, by, k, dist), (plain, plain_st, by_p, k_p, dist_p)) = dense_rs
    want, want_st = E.run(by, k, dist, options=BOTH)
    want_p, want_p_st = E.run(by_p, k_p, dist_p, options=E.ES)
    f = nat.p25lc_fields(recs)
    print("dense RS: %d hits, %s, es alone %s; n_rs %s" % (len(k), st, plain_st, np.bincount(f["n_rs"]).tolist()))
    _same(recs, want, "dense")
    _same(plain, want_p, "dense, es alone")
    assert st == want_st and plain_st == want_p_st and st["n_lost"] == plain_st["n_lost"] == 0
    assert st["n_records"] == st["n_frames"] == st["n_decoded"] == len(plan)
    starts = [p["start"] for p in plan]
    for kk, dd in ((k, dist), (k_p, dist_p)):
        assert len(kk) == len(plan) and not np.any(dd) and np.diff(kk).tolist() == np.diff(starts).tolist()
    shift = int(k[0]) - 23 - starts[0]
    assert int(k_p[0]) == int(k[0])
    CW.check_rs_census(want, want_p, [dict(p, start=p["start"] + shift) for p in plan])


def test_dense_reed_solomon_words_do_not_depend_on_the_cuts(gpu_required, dense_rs):
    """the same carrier in pushes of 16 000 samples and in ragged pushes, some of under one symbol: the whole-stream records"""
    nat = gpu_required
    x, plan, whole = dense_rs
    for name, pieces in (("blocks", _pieces(len(x), 16000)), ("ragged", _ragged(len(x), 36))):
        for n, (got, ref) in enumerate(zip(_run_rs(nat, x, pieces), whole)):
            _same(got[0], ref[0], (name, n))
            assert got[1] == ref[1] and got[2].tobytes() == ref[2].tobytes() and np.array_equal(got[3], ref[3]), (name, n)


# ------------------------------------------------------------------------------------------------ the NID
def test_dense_nid_words_on_both_stages(gpu_required):
    """234 frames back to back under four channels of one front end: a TSBK stage and a voice stage with nid = 1, beside each
    a twin without.  TDUs carry every single wrong bit of the 63 and the 64th bit alone, per weight 2 .. 11 twelve random
    patterns and a burst of adjacent bits at either end of the word, and per weight 12 and 13 twelve patterns beyond the
    radius; TSDUs, HDUs and LDU1s whose DUID is broken by one and by three bits decode where the twins give bare records.
    Records, state and rcf_chan_nid_state are the restatement's (nid_ref) over each channel's own words and hits, the twins'
    records tsbk_ref's and p25es_ref's; the census demands every class and that the counters are the sums over the records"""
    nat = gpu_required
    d, plan = CW.dense_nid_dibits(NAC)
    x = _carrier(d)
    mix = (("tsbk", True), ("tsbk", False), ("voice", True), ("voice", False))
    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        chans = [_open(nat, fe, stage, nid=nid) for stage, nid in mix]
        for a in range(0, len(x), BLK):
            fe.push(x[a:a + BLK])
        got = []
        for (stage, nid), c in zip(mix, chans):
            recs = fe.chan_read_tsbk(c) if stage == "tsbk" else fe.chan_read_p25lc(c)
            st = fe.chan_tsbk_state(c) if stage == "tsbk" else fe.chan_p25lc_state(c)
            got.append((recs, st, fe.chan_nid_state(c)) + _streams(fe, c))
    starts = [p["start"] for p in plan]
    want = {}
    for (stage, nid), (recs, st, nst, by, k, dist) in zip(mix, got):
        assert len(k) == len(plan) and not np.any(dist) and np.diff(k).tolist() == np.diff(starts).tolist(), (stage, nid, len(k))
        w = N.run_tsbk(by, k, dist, nid=int(nid)) if stage == "tsbk" else N.run_voice(by, k, dist, nid=int(nid), options=BOTH)
        _same(recs, w[0], (stage, nid))
        assert (st, nst) == w[1:] and st["n_lost"] == 0 and st["n_frames"] == len(plan), (stage, nid, st, nst, w[1:])
        if not nid:
            _same(recs, (T.run(by, k, dist) if stage == "tsbk" else E.run(by, k, dist, options=BOTH))[0], ("the twin", stage))
            assert nst == NO_NID
        want[(stage, nid)] = w
        shift = int(k[0]) - 23 - starts[0]
    print("dense NID: %d frames, nid %s; nid_fix %s" % (len(plan), got[0][2], np.bincount(nat.nid_fields(got[2][0])["nid_fix"]).tolist()))
    assert got[0][2] == got[2][2] == CW.nid_counters(plan)
    for stage in ("tsbk", "voice"):
        CW.check_nid_census(stage, want[(stage, True)][0], want[(stage, False)][0], [dict(p, start=p["start"] + shift) for p in plan], want[(stage, True)][2])
