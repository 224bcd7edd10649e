"""The NID option of the two P25 stages on the GPU (RCF_NID_BCH: rcf_chan_tsbk_ex, rcf_chan_p25lc_ex; nid_wave.hpp in
tsbk.hip and p25lc.hip): the NID's BCH(63,16,23) word decoded before the DUID is acted on.  include/rcf.h defines the rule,
tests/nid_ref.py restates it by exhaustive search on top of tests/tsbk_ref.py and tests/p25es_ref.py.  As in the other
suites of the hard-decision chain the yardstick is always that restatement applied to the channel's OWN packed words and sync
hits as the slicer's readers deliver them, and every comparison -- records, counters, rcf_chan_nid_state -- is of bits.  One
400 kS/s front-end, 25 kS/s channels, 4800 baud."""
import ctypes

import numpy as np
import pytest

import fsk4_ref as F
import nid_ref as N
import p25es_ref as E
import p25lc_ref as R
import tsbk_ref as T
from rcf import p25, synth

pytestmark = pytest.mark.gpu

FS, CR, OFF = F.FS, F.CHANNEL_RATE, F.CHANNEL_OFFSET
BLK = 16 * 1000
NAC = R.CALL["nac"]
VOICE = dict(correct=1, options=E.ES | E.ERASURES)
# (stage, nid, voice options) of the mixed launches
MIX = (("tsbk", 1, None), ("voice", 1, (1, True, True)), ("tsbk", 0, None), ("voice", 1, (0, True, False)), ("voice", 0, (1, True, False)),
       ("voice", 1, (1, False, False)))


def _noise(seed, n, amp=0.05):
    return (amp * synth.awgn(np.random.default_rng(seed), n)).astype(np.complex64)


def _code(nat, fn, *a, **kw):
    with pytest.raises(nat.RcfError) as e:
        fn(*a, **kw)
    return e.value.code


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, len(got), len(want), got[:4], want[:4])


def _loose(errors):
    return dict(sync_word=p25.FRAME_SYNC, sync_bits=48, sync_max_errors=errors, hit_capacity=4096)


def _attach(fe, c, stage, nid, voice=(1, True, True), capacity=0):
    if stage == "tsbk":
        fe.chan_tsbk(c, capacity, nid=nid)
    else:
        fe.chan_p25lc_ex(c, capacity, correct=bool(voice[0]), es=voice[1], erasures=voice[2], nid=nid)


def _open(nat, fe, f, mix, search, capacity=0):
    c = fe.chan_open(CR, f)
    fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
    fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
    fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, **search)
    _attach(fe, c, mix[0], mix[1], mix[2] or (1, True, True), capacity)
    return c


def _read(fe, c, stage, **kw):
    return fe.chan_read_tsbk(c, **kw) if stage == "tsbk" else fe.chan_read_p25lc(c, **kw)


def _state(fe, c, stage):
    return fe.chan_tsbk_state(c) if stage == "tsbk" else fe.chan_p25lc_state(c)


def _want(fe, c, stage, nid, voice=(1, True, True), **kw):
    """the restatement over everything the slicer's two readers deliver -> (records, counters, the NID's counters)"""
    by = fe.chan_read_hard(c)
    k, dist = fe.chan_read_sync(c)
    if stage == "tsbk":
        return N.run_tsbk(by, k, dist, nid=nid, **kw)
    return N.run_voice(by, k, dist, nid=nid, correct=voice[0], options=(E.ES if voice[1] else 0) | (E.ERASURES if voice[2] else 0), **kw)


@pytest.fixture(scope="module")
def designed():
    """N.designed_dibits of both stages as noise-free 4800-baud C4FM carriers at the channel's offset, 150 Hz off"""
    out = {}
    for stage in ("tsbk", "voice"):
        d, plan = N.designed_dibits(stage, NAC)
        out[stage] = (F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0), plan)
    return out


def _run(nat, x, pieces, stage, nid):
    with nat.Frontend(FS, device=0, block_capacity=max(b - a for a, b in zip(pieces[:-1], pieces[1:]))) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, tsbk=stage == "tsbk", lc=stage == "voice", es=True, erasures=True, nid=nid)
        for a, b in zip(pieces[:-1], pieces[1:]):
            fe.push(x[a:b])
        return _read(fe, c, stage), _state(fe, c, stage), fe.chan_nid_state(c), _want(fe, c, stage, nid)


# ------------------------------------------------------------------------------------------------ designed NIDs
@pytest.mark.parametrize("stage", ["tsbk", "voice"])
def test_designed_carrier_meets_every_class_beside_a_twin_without_the_option(gpu_required, designed, stage):
    """frames whose NID carries 0 .. 11 wrong bits (bit 0, bit 62, the two bits either side of the status symbol among them),
    the 64th bit flipped alone, a word of 12 wrong bits beyond every code word (nid_fix 15, fields as read), the crafted word
    of 12 that decodes to another code word (nid_fix 11), and data units whose received DUID is broken: each decodes where the
    twin attached with nid = 0 gives a bare frame record; a TSDU read as DUID 7 that decodes to 5 has no block decoded.  The
    census over the restatement's records demands every one of these; tests/test_nid_cpu.py holds it on the planted dibits"""
    nat = gpu_required
    x, plan = designed[stage]
    blk = 4 * BLK
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, tsbk=stage == "tsbk", lc=stage == "voice", es=True, erasures=True, nid=True)
        c_raw = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, tsbk=stage == "tsbk", lc=stage == "voice", es=True, erasures=True)
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk])
        recs, st, nst = _read(fe, c, stage), _state(fe, c, stage), fe.chan_nid_state(c)
        raw, raw_st, raw_nst = _read(fe, c_raw, stage), _state(fe, c_raw, stage), fe.chan_nid_state(c_raw)
        k, dist = fe.chan_read_sync(c)
        by = fe.chan_read_hard(c)
        want, want_st, want_nst = N.run_tsbk(by, k, dist) if stage == "tsbk" else N.run_voice(by, k, dist, **VOICE)
        want_raw, want_raw_st, want_raw_nst = _want(fe, c_raw, stage, 0)
    print("designed %s: %d hits, %s, nid %s; twin %s; nid_fix %s" % (stage, len(k), st, nst, raw_st, nat.nid_fields(recs)["nid_fix"].tolist()))
    _same(recs, want, "designed")
    _same(raw, want_raw, "twin")
    assert st == want_st and nst == want_nst and raw_st == want_raw_st and raw_nst == want_raw_nst == dict(n_decoded=0, n_fixed=0, n_bits=0, n_bad=0)
    fixes = [p["fix"] for p in plan]
    assert nst == dict(n_decoded=len(plan), n_fixed=sum(0 < f < 15 for f in fixes), n_bits=sum(f for f in fixes if f < 15), n_bad=1)
    starts = [p["start"] for p in plan]
    assert len(k) == len(starts) and not np.any(dist) and np.diff(k).tolist() == np.diff(starts).tolist()
    shift = int(k[0]) - 23 - starts[0]
    N.check_census(stage, want, want_raw, [dict(p, start=p["start"] + shift) for p in plan])
    plain = T.run if stage == "tsbk" else (lambda *a: E.run(*a, **VOICE))           # the twin's records are the parent's
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        ch = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True)
        p = nat.TsbkParams(capacity=0) if stage == "tsbk" else nat.P25lcParams(capacity=0, correct=1)
        assert (nat.lib().rcf_chan_tsbk(fe._h, ch, ctypes.byref(p)) if stage == "tsbk" else nat.lib().rcf_chan_p25lc_opt(fe._h, ch, ctypes.byref(p), 3)) == nat.RCF_OK
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk])
        old = _read(fe, ch, stage)
        by = fe.chan_read_hard(ch)
        kk, dd = fe.chan_read_sync(ch)
        assert fe.chan_nid_state(ch) == dict(n_decoded=0, n_fixed=0, n_bits=0, n_bad=0)
    _same(old, plain(by, kk, dd)[0], "the old entry point")
    _same(old, raw, "the old entry point and nid = 0")


# ------------------------------------------------------------------------------------------------ cuts
@pytest.mark.parametrize("stage", ["tsbk", "voice"])
def test_the_records_do_not_depend_on_the_cuts(gpu_required, designed, stage):
    nat = gpu_required
    x = designed[stage][0]
    rng = np.random.default_rng(35)
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 40)}
    cuts |= {16 * 4000 + 5 * j for j in range(1, 14)} | {16 * 6000 + 84 * j for j in range(40)} | {16 * 9000 + 16 * 30 * j for j in range(20)}     # blocks of 0 and 1 symbols
    whole = _run(nat, x, list(range(0, len(x), 900000)) + [len(x)], stage, True)        # (as whole as the channel's ring takes it)
    ragged = _run(nat, x, sorted(cuts), stage, True)
    blocks = _run(nat, x, list(range(0, len(x), BLK)) + [len(x)], stage, True)
    for name, r in (("whole", whole), ("ragged", ragged), ("blocks", blocks)):
        _same(r[0], r[3][0], name)
        assert (r[1], r[2]) == r[3][1:], name
    _same(ragged[0], whole[0], "cuts"); _same(blocks[0], whole[0], "blocks")
    assert ragged[1:3] == whole[1:3] == blocks[1:3] and whole[2]["n_decoded"] == len(designed[stage][1])


# ------------------------------------------------------------------------------------------------ many channels, groups
def test_130_channels_with_and_without_the_option_in_one_launch(gpu_required):
    """noise under 130 channels that search it loosely: TSBK and voice stages, with and without nid, across the voice
    options -- one launch of each stage per block whatever the flags.  Channel 7's record ring holds 16, wraps and loses;
    on every fifth channel the single reader takes three records before the batched reader takes the rest"""
    nat = gpu_required
    blk, K = 16000, 14
    x = _noise(132, blk * K)
    offs = [-190000.0 + 2900.0 * j for j in range(130)]
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        cids = [_open(nat, fe, f, MIX[j % 6], _loose(16 if j == 7 else 14 - j % 3), capacity=16 if j == 7 else 0) for j, f in enumerate(offs)]
        rest = [j for j in range(130) if j != 7]
        taken = {j: [] for j in rest}
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk])
            if b % 3 == 2:
                for j in rest[::5]:
                    taken[j].append(_read(fe, cids[j], MIX[j % 6][0], max_records=3))
                for what in ("tsbk", "p25lc"):
                    js = [j for j in rest if (MIX[j % 6][0] == "tsbk") == (what == "tsbk")]
                    for j, row in zip(js, fe.chan_read_many([cids[j] for j in js], what, cap_each=128)):
                        assert row is not None
                        taken[j].append(row.copy())
        n_rec = n_fixed = n_bad = 0
        for j, c in enumerate(cids):
            stage, nid, voice = MIX[j % 6]
            got = _read(fe, c, stage) if j == 7 else np.concatenate(taken[j] + [_read(fe, c, stage)])
            st, nst = _state(fe, c, stage), fe.chan_nid_state(c)
            want, want_st, want_nst = _want(fe, c, stage, nid, voice or (1, True, True))
            assert st == want_st and nst == want_nst and st["n_lost"] == 0, (j, st, want_st, nst, want_nst)
            if j == 7:
                assert len(want) > 16
                want = want[-16:]
            _same(got, want, ("lane", j))
            f = nat.nid_fields(got)
            assert np.all(f["nid_decoded"] == nid) and (nid or not np.any(f["nid_fix"]))
            n_rec += len(got); n_fixed += nst["n_fixed"]; n_bad += nst["n_bad"]
    print("130 channels: %d records, NIDs fixed %d, beyond the bound %d" % (n_rec, n_fixed, n_bad))
    assert n_rec > 104 and n_bad > 50


def test_two_front_ends_in_a_group(gpu_required):
    """a group's block: stages of both kinds with and without the option on each member, the group's reader interleaved with
    the single one"""
    nat = gpu_required
    blk, K = 16000, 14
    xs = [_noise(60 + m, blk * K) for m in range(2)]
    offs = (-100000.0, 60000.0, 150000.0, -30000.0)
    fes = [nat.Frontend(FS, device=0, block_capacity=blk) for _ in range(2)]
    try:
        mix = [[MIX[(j + 3 * m) % 6] for j in range(4)] for m in range(2)]
        ids = [[_open(nat, fe, f, mix[m][j], _loose(13)) for j, f in enumerate(offs)] for m, fe in enumerate(fes)]
        pairs = [(m, j) for m in range(2) for j in range(4)]
        taken = {p: [] for p in pairs}
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * blk:(b + 1) * blk] for xm in xs])
                if b % 4 == 3:
                    m, j = pairs[b % len(pairs)]
                    taken[(m, j)].append(_read(fes[m], ids[m][j], mix[m][j][0], max_records=2))
                    for what in ("tsbk", "p25lc"):
                        ps = [p for p in pairs if (mix[p[0]][p[1]][0] == "tsbk") == (what == "tsbk")]
                        for p, row in zip(ps, g.read_many([(m_, ids[m_][j_]) for m_, j_ in ps], what, cap_each=64)):
                            assert row is not None
                            taken[p].append(row.copy())
            g.sync()
            total = 0
            for m, j in pairs:
                stage, nid, voice = mix[m][j]
                c = ids[m][j]
                got = np.concatenate(taken[(m, j)] + [_read(fes[m], c, stage)])
                want, want_st, want_nst = _want(fes[m], c, stage, nid, voice or (1, True, True))
                _same(got, want, ("group", m, j))
                assert _state(fes[m], c, stage) == want_st and fes[m].chan_nid_state(c) == want_nst
                total += len(want)
            print("group: %d records" % total)
            assert total > len(pairs)
    finally:
        for fe in fes:
            fe.close()


# ------------------------------------------------------------------------------------------------ lifecycle
def test_lifecycle_refusals_and_afresh_with_the_other_value_mid_frame(gpu_required, designed):
    nat = gpu_required
    lib = nat.lib()
    x, plan = designed["voice"]
    with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True)
        pt, pv = nat.TsbkParams(capacity=0), nat.P25lcParams(capacity=0, correct=1)
        for nid in (2, 3, 0x80000000):
            assert lib.rcf_chan_tsbk_ex(fe._h, c, ctypes.byref(pt), nid) == nat.RCF_EINVAL
            assert lib.rcf_chan_p25lc_ex(fe._h, c, ctypes.byref(pv), 0, nid) == nat.RCF_EINVAL
        assert _code(nat, fe.chan_tsbk, c, nid=2) == nat.RCF_EINVAL
        assert lib.rcf_chan_p25lc_ex(fe._h, c, ctypes.byref(pv), 4, 1) == nat.RCF_EINVAL              # the existing calls' refusals stand
        assert _code(nat, fe.chan_p25lc_ex, c, correct=False, erasures=True, nid=True) == nat.RCF_EINVAL
        assert _code(nat, fe.chan_nid_state, c) == nat.RCF_ESTATE                                   # none of them attached a stage
        assert _code(nat, fe.chan_nid_state, c + 1000) == nat.RCF_ENOCHAN
        assert lib.rcf_chan_nid_state(fe._h, c, None) == nat.RCF_EINVAL
        assert lib.rcf_chan_tsbk_ex(fe._h, c, None, 1) == nat.RCF_OK                                  # off: nothing to do
        fe.chan_tsbk(c, nid=True)
        assert fe.chan_nid_state(c) == dict(n_decoded=0, n_fixed=0, n_bits=0, n_bad=0)
        assert _code(nat, fe.chan_p25lc_ex, c, nid=True) == nat.RCF_ESTATE
        fe.chan_tsbk(c, on=False)
        assert _code(nat, fe.chan_nid_state, c) == nat.RCF_ESTATE
        # attached in mid-frame with the option, then again inside a later frame without it: afresh each time
        attach = int((plan[2]["start"] + 100) * FS / 4800.0) // 16 * 16
        fe.push(x[:attach])
        first = fe.chan_slicer_state(c)["n_hits"]
        fe.chan_p25lc_ex(c, es=True, erasures=True, nid=True)
        again = int((plan[9]["start"] + 100) * FS / 4800.0) // 16 * 16
        fe.push(x[attach:again])
        mid, mid_st, mid_nst = fe.chan_read_p25lc(c), fe.chan_p25lc_state(c), fe.chan_nid_state(c)
        at = fe.chan_slicer_state(c)
        second = at["n_hits"]
        fe.chan_p25lc_ex(c, 64, es=True, erasures=True, nid=False)
        assert fe.chan_p25lc_ring(c)[1] == 64 and fe.chan_p25lc_state(c)["n_records"] == 0 and fe.chan_nid_state(c)["n_decoded"] == 0
        fe.push(x[again:])
        recs, st, nst = fe.chan_read_p25lc(c), fe.chan_p25lc_state(c), fe.chan_nid_state(c)
        by = fe.chan_read_hard(c)
        k, dist = fe.chan_read_sync(c)
    assert first >= 3 and second >= 10
    want_mid = N.run_voice(by, k, dist, nid=1, first_hit=first, launches=[(at["n_words"], second)], **VOICE)
    _same(mid, want_mid[0], "mid-frame")
    assert (mid_st, mid_nst) == want_mid[1:] and len(mid) >= 2 and np.all(nat.nid_fields(mid)["nid_decoded"] == 1)
    want = E.run(by, k, dist, first_hit=second, **VOICE)
    _same(recs, want[0], "afresh")
    assert st == want[1] and nst == dict(n_decoded=0, n_fixed=0, n_bits=0, n_bad=0) and len(recs) >= 5
    assert not np.any(nat.nid_fields(recs)["nid_decoded"]) and not np.any(nat.nid_fields(recs)["nid_fix"])
