"""The trellis option of the P25 trunking stage on the GPU (RCF_TRELLIS_VITERBI: rcf_chan_tsbk_opt; the suffix scan of min-plus
matrices in tsbk.hip): a block decoded by the least-cost path that ends in state 0 instead of the reference's word-by-word
walk.  include/rcf.h defines the rule, tests/trellis_ref.py restates it sequentially on top of tests/tsbk_ref.py and
tests/nid_ref.py.  As in the other suites of the hard-decision chain the yardstick is always that restatement applied to the
channel's OWN packed words and sync hits as the slicer's readers deliver them, and every comparison -- records, counters,
rcf_chan_trellis_state -- is of bits.  One 400 kS/s front-end, 25 kS/s channels; the helpers are the TSBK suite's."""
import ctypes

import numpy as np
import pytest

import fsk4_ref as F
import nid_ref as N
import p25es_ref as E
import test_gpu_edacs as GE
import test_gpu_hard_delivery as HD
import test_gpu_osw as GO
import test_gpu_tsbk as G
import trellis_ref as V
import tsbk_ref as T
from rcf import p25

pytestmark = pytest.mark.gpu

FS, CR, OFF, BLK, NAC = G.FS, G.CR, G.OFF, G.BLK, G.NAC
_same, _code, _noise = G._same, G._code, G._noise
NONE = V.empty_state()


def _streams(fe, c):
    """everything the slicer's two readers deliver (the whole streams: nobody has read them before, and nobody can again)"""
    by = fe.chan_read_hard(c)
    k, dist = fe.chan_read_sync(c)
    return by, k, dist


def _rule(streams, nid, viterbi, **kw):
    """the restatement over those streams -> (records, counters, the NID's, the trellis decoder's)"""
    return V.run(*streams, V.VITERBI if viterbi else V.GREEDY, nid=int(nid), **kw)


def _want(fe, c, nid, viterbi, **kw):
    return _rule(_streams(fe, c), nid, viterbi, **kw)


def _got(fe, c):
    return fe.chan_read_tsbk(c), fe.chan_tsbk_state(c), fe.chan_nid_state(c), fe.chan_trellis_state(c)


@pytest.fixture(scope="module")
def designed():
    """V.designed_dibits as a noise-free 4800-baud C4FM carrier at the channel's offset, 150 Hz off -> (x, plan, starts)"""
    d, plan, starts = V.designed_dibits(NAC)
    return F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0), plan, starts


def _run(nat, x, pieces, viterbi=True, nid=False):
    with nat.Frontend(FS, device=0, block_capacity=max(b - a for a, b in zip(pieces[:-1], pieces[1:]))) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, tsbk=True, nid=nid, viterbi=viterbi)
        for a, b in zip(pieces[:-1], pieces[1:]):
            fe.push(x[a:b])
        return _got(fe, c), _want(fe, c, nid, viterbi)


# ------------------------------------------------------------------------------------------------ designed blocks
def test_designed_carrier_beside_a_twin_without_the_option(gpu_required, designed):
    """valid TSBKs with planted channel-bit flips, in frames of 360, 288 and 180 dibits: none; single flips that do and do
    not leave the walk two tied candidates; a flip in the flushing word; doubles in one code word and in two; bursts of 4
    in channel order; 3, 4 and 8 flips; a frame cut by an early sync behind its first block, and one cut before any block
    ends (a frame record).  The census (V.check_census, held on the planted dibits by tests/test_trellis_cpu.py) fails if a
    kind is missing after demodulation; every block with at most 2 flips carries the sent octets, a good CRC and its flips as
    cost on the option's channel, and at least one of them has a bad CRC on the twin in the same launch -- which is what
    fails without the feature"""
    nat = gpu_required
    x, plan, starts = designed
    blk = 4 * BLK
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, tsbk=True, viterbi=True)
        c_raw = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True, tsbk=True)
        for a in range(0, len(x), blk):
            fe.push(x[a:a + blk])
        got, raw = _got(fe, c), _got(fe, c_raw)
        own, own_raw = _streams(fe, c), _streams(fe, c_raw)
    _, k, dist = own
    want, want_raw, plain = _rule(own, 0, True), _rule(own_raw, 0, False), T.run(*own_raw)
    print("designed: %d hits, %s, trellis %s; twin %s" % (len(k), got[1], got[3], raw[1]))
    _same(got[0], want[0], "designed"); _same(raw[0], want_raw[0], "twin"); _same(raw[0], plain[0], "the twin's records are today's")
    assert got[1:] == want[1:] and raw[1:] == want_raw[1:] and raw[1] == plain[1] and raw[3] == NONE
    assert len(k) == len(starts) and not np.any(dist) and np.diff(k).tolist() == np.diff(starts).tolist()       # the planted frames, all, and nothing else
    census = V.check_census(got[0], raw[0], plan, nat.tsbk_fields, nat.trellis_fields)
    print("designed census: %s; frame_dibits %s" % (census, sorted(set(nat.nid_fields(got[0])["frame_dibits"].tolist()))))
    assert {360, 288, 180, 200, 100} == set(nat.nid_fields(got[0])["frame_dibits"].tolist())
    v = nat.trellis_fields(got[0])
    assert got[3] == dict(n_decoded=census["blocks"], n_clean=int(np.sum((v["cost"] == 0) & (v["viterbi"] == 1))), n_bits=int(v["cost"].sum()),
                          n_words=int(nat.tsbk_fields(got[0])["n_inexact"].sum()))
    assert got[1]["n_crc_bad"] < raw[1]["n_crc_bad"] and got[1]["n_blocks"] == raw[1]["n_blocks"] == census["blocks"]


# ------------------------------------------------------------------------------------------------ cuts
def test_the_records_do_not_depend_on_the_cuts(gpu_required, designed):
    nat = gpu_required
    x = designed[0]
    rng = np.random.default_rng(36)
    cuts = {0, len(x)} | {int(v) for v in rng.integers(1, len(x), 40)}
    cuts |= {16 * 4000 + 5 * j for j in range(1, 14)} | {16 * 6000 + 84 * j for j in range(40)} | {16 * 9000 + 16 * 30 * j for j in range(20)}     # blocks of 0 and 1 symbols
    costs = []
    for nid in (False, True):                        # whole (as whole as the channel's ring takes it), ragged, block by block
        whole = _run(nat, x, list(range(0, len(x), 900000)) + [len(x)], nid=nid)
        ragged = _run(nat, x, sorted(cuts), nid=nid)
        blocks = _run(nat, x, list(range(0, len(x), BLK)) + [len(x)], nid=nid)
        for name, (got, want) in (("whole", whole), ("ragged", ragged), ("blocks", blocks)):
            _same(got[0], want[0], (name, nid))
            assert got[1:] == want[1:], (name, nid)
        _same(ragged[0][0], whole[0][0], ("cuts", nid)); _same(blocks[0][0], whole[0][0], ("blocks", nid))
        assert ragged[0][1:] == whole[0][1:] == blocks[0][1:] and whole[0][3]["n_decoded"] == whole[0][1]["n_blocks"] > 40
        assert whole[0][2]["n_decoded"] == (whole[0][1]["n_frames"] if nid else 0)
        costs.append(nat.trellis_fields(whole[0][0])["cost"])
    assert np.array_equal(costs[0], costs[1])        # the NID option leaves a clean NID's blocks as they are


# ------------------------------------------------------------------------------------------------ many channels, groups
# (nid, viterbi) of the TSBK stages of a mixed launch, by j % 4
MIX = ((0, 1), (1, 1), (0, 0), (1, 0))


def _open_tsbk(nat, fe, f, j, nid, viterbi, capacity=0):
    """channel j at offset f behind the TSBK suite's loose search (the loop by j % 3, 6000 baud on every fourth); a channel
    with a small record ring searches more loosely still, so that the ring wraps"""
    c = G._open_loose(nat, fe, f, j, tsbk=False, search=dict(G.LOOSE, sync_max_errors=17) if capacity else None)
    fe.chan_tsbk(c, capacity, nid=bool(nid), viterbi=bool(viterbi))
    return c


def _open_mixed(nat, fe, f, j, capacity=0):
    """channel j at offset f: every seventh a P25 voice, an EDACS or an OSW chain, the others a TSBK stage behind one of the
    two P25 loops under a loose search -> (channel id, kind)"""
    if j % 7 == 3:
        return GE._open_loose(nat, fe, f), "edacs"
    if j % 7 == 5:
        return GO._open(fe, f), "osw"
    if j % 7 == 6:
        c = G._open_loose(nat, fe, f, j, tsbk=False)
        fe.chan_p25lc_ex(c, es=True, erasures=True, nid=bool(j % 2))
        return c, "p25lc"
    return _open_tsbk(nat, fe, f, j, *MIX[j % 4], capacity=capacity), "tsbk"


def _check_other(nat, fe, c, kind, j, got):
    """the stages of other kinds that share the launches: their records are their own restatements'"""
    if kind == "edacs":
        want = GE._want(fe, c)
    elif kind == "osw":
        want = GO._want(fe, c)
    else:
        by = fe.chan_read_hard(c)
        k, dist = fe.chan_read_sync(c)
        want = N.run_voice(by, k, dist, nid=j % 2, correct=1, options=E.ES | E.ERASURES)
    _same(got, want[0], (kind, j))
    return len(got)


def test_130_channels_of_both_rules_in_one_launch(gpu_required):
    """noise under 130 channels that search it loosely: greedy and Viterbi TSBK stages with and without nid behind both P25
    loops, beside voice, EDACS and OSW stages -- one launch of the TSBK stages per block whatever their flags.  Channel 8's
    record ring holds 16, wraps and loses; on every fifth TSBK channel the single reader takes three records before the
    batched reader takes the rest"""
    nat = gpu_required
    blk, K = 16000, 12
    x = _noise(133, blk * K)
    offs = [-190000.0 + 2900.0 * j for j in range(130)]
    with nat.Frontend(FS, device=0, block_capacity=blk) as fe:
        opened = [_open_mixed(nat, fe, f, j, capacity=16 if j == 8 else 0) for j, f in enumerate(offs)]
        tsbk = [j for j in range(130) if opened[j][1] == "tsbk" and j != 8]
        taken = {j: [] for j in tsbk}
        for b in range(K):
            fe.push(x[b * blk:(b + 1) * blk])
            if b % 3 == 2:
                for j in tsbk[::5]:
                    taken[j].append(fe.chan_read_tsbk(opened[j][0], max_records=3))
                for j, row in zip(tsbk, fe.chan_read_many([opened[j][0] for j in tsbk], "tsbk", cap_each=128)):
                    assert row is not None
                    taken[j].append(row.copy())
        n_rec = n_other = n_changed = 0
        seen = set()
        for j, (c, kind) in enumerate(opened):
            if kind != "tsbk":
                n_other += _check_other(nat, fe, c, kind, j, {"edacs": fe.chan_read_edacs, "osw": fe.chan_read_osw, "p25lc": fe.chan_read_p25lc}[kind](c))
                assert _code(nat, fe.chan_trellis_state, c) == nat.RCF_ESTATE
                continue
            nid, viterbi = MIX[j % 4]
            recs, st, nst, vst = _got(fe, c)
            got = recs if j == 8 else np.concatenate(taken[j] + [recs])
            own = _streams(fe, c)
            want = _rule(own, nid, viterbi)
            assert (st, nst, vst) == want[1:] and st["n_lost"] == 0, (j, st, nst, vst, want[1:])
            if j == 8:
                assert len(want[0]) > 16 and MIX[8 % 4][1] == 1
            _same(got, want[0][-16:] if j == 8 else want[0], ("lane", j))
            f, v = nat.tsbk_fields(got), nat.trellis_fields(got)
            assert np.all(v["viterbi"] == (viterbi & (f["b"] != 3))) and (viterbi or (not np.any(v["cost"]) and vst == NONE))
            assert np.all(nat.nid_fields(got)["nid_decoded"] == nid)
            if viterbi:                              # where the other rule would have given other octets
                other = _rule(own, nid, 0)[0][-len(got):] if len(got) else got
                n_changed += int(np.sum(np.any(other["octets"] != got["octets"], axis=1)))
            n_rec += len(got); seen.add((G._kind_of(j), nid, viterbi))
    print("130 channels: %d TSBK records (%d blocks decoded otherwise by the walk), %d records of other kinds" % (n_rec, n_changed, n_other))
    assert len(seen) == 8 and n_rec > 90 and n_changed > 0 and n_other > 0


def test_two_front_ends_in_a_group(gpu_required):
    """a group's block: TSBK stages of both rules on each member, the group's reader interleaved with the single one"""
    nat = gpu_required
    blk, K = 16000, 12
    xs = [_noise(70 + m, blk * K) for m in range(2)]
    offs = (-100000.0, 60000.0, 150000.0, -30000.0)
    fes = [nat.Frontend(FS, device=0, block_capacity=blk) for _ in range(2)]
    try:
        mix = [[MIX[(j + m) % 4] for j in range(4)] for m in range(2)]
        ids = [[_open_tsbk(nat, fe, f, j + m, *mix[m][j]) for j, f in enumerate(offs)] for m, fe in enumerate(fes)]
        pairs = [(m, j) for m in range(2) for j in range(4)]
        taken = {p: [] for p in pairs}
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * blk:(b + 1) * blk] for xm in xs])
                if b % 4 == 3:
                    m, j = pairs[b % len(pairs)]
                    taken[(m, j)].append(fes[m].chan_read_tsbk(ids[m][j], max_records=2))
                    for p, row in zip(pairs, g.read_many([(m_, ids[m_][j_]) for m_, j_ in pairs], "tsbk", cap_each=64)):
                        assert row is not None
                        taken[p].append(row.copy())
            g.sync()
            total = 0
            for m, j in pairs:
                nid, viterbi = mix[m][j]
                c = ids[m][j]
                recs, st, nst, vst = _got(fes[m], c)
                want = _want(fes[m], c, nid, viterbi)
                _same(np.concatenate(taken[(m, j)] + [recs]), want[0], ("group", m, j))
                assert (st, nst, vst) == want[1:]
                total += len(want[0])
            print("group: %d records" % total)
            assert total > len(pairs) and {v for row in mix for _, v in row} == {0, 1}
    finally:
        for fe in fes:
            fe.close()


# ------------------------------------------------------------------------------------------------ lifecycle, refusals, delivery
def test_attach_in_mid_frame_again_with_the_other_value_and_refusals(gpu_required, designed):
    nat = gpu_required
    lib = nat.lib()
    x, plan, starts = designed
    with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
        c = p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True)
        pt = nat.TsbkParams(capacity=0)
        for trellis in (2, 3, 0x80000000):
            assert lib.rcf_chan_tsbk_opt(fe._h, c, ctypes.byref(pt), 0, trellis) == nat.RCF_EINVAL
        assert lib.rcf_chan_tsbk_opt(fe._h, c, ctypes.byref(pt), 2, 1) == nat.RCF_EINVAL              # nid's refusal stands
        assert lib.rcf_chan_tsbk_ex(fe._h, c, ctypes.byref(pt), 2) == nat.RCF_EINVAL
        assert _code(nat, fe.chan_tsbk, c, viterbi=2) == nat.RCF_EINVAL
        assert _code(nat, fe.chan_trellis_state, c) == nat.RCF_ESTATE                                # none of them attached a stage
        assert _code(nat, fe.chan_trellis_state, c + 1000) == nat.RCF_ENOCHAN
        assert lib.rcf_chan_trellis_state(fe._h, c, None) == nat.RCF_EINVAL
        assert lib.rcf_chan_tsbk_opt(fe._h, c, None, 0, 1) == nat.RCF_OK                              # off: nothing to do
        assert lib.rcf_chan_tsbk_opt(fe._h, c, None, 2, 2) == nat.RCF_OK                              # ... and neither value is looked at
        fe.chan_p25lc_ex(c)
        assert _code(nat, fe.chan_trellis_state, c) == nat.RCF_ESTATE                                # the voice stage has no trellis
        assert _code(nat, fe.chan_tsbk, c, viterbi=True) == nat.RCF_ESTATE
        fe.chan_p25lc(c, on=False)
        # attached in mid-frame with the option, then again inside a later frame without it: afresh each time
        sps = FS / 4800.0
        attach = int((starts[2] + 100) * sps) // 16 * 16
        fe.push(x[:attach])
        first = fe.chan_slicer_state(c)["n_hits"]
        fe.chan_tsbk(c, viterbi=True)
        assert fe.chan_trellis_state(c) == NONE
        again = int((starts[9] + 100) * sps) // 16 * 16
        fe.push(x[attach:again])
        mid = _got(fe, c)
        at = fe.chan_slicer_state(c)
        second = at["n_hits"]
        fe.chan_tsbk(c, 64, viterbi=False)
        assert fe.chan_tsbk_ring(c)[1] == 64 and fe.chan_tsbk_state(c)["n_records"] == 0 and fe.chan_trellis_state(c) == NONE
        fe.push(x[again:])
        late = _got(fe, c)
        by = fe.chan_read_hard(c)
        k, dist = fe.chan_read_sync(c)
    assert first >= 3 and second >= 10
    want_mid = V.run(by, k, dist, V.VITERBI, first_hit=first, launches=[(at["n_words"], second)])
    _same(mid[0], want_mid[0], "mid-frame")
    assert mid[1:] == want_mid[1:] and len(mid[0]) >= 6 and np.all(nat.trellis_fields(mid[0])["viterbi"] == 1) and mid[3]["n_decoded"] == len(mid[0])
    want = T.run(by, k, dist, first_hit=second)
    _same(late[0], want[0], "afresh")                                                                # no record mixes the rules
    assert late[1] == want[1] and late[3] == NONE and len(late[0]) >= 6 and not np.any(late[0]["frame_dibits"] >> 16)
    assert set(mid[0]["k"].tolist()).isdisjoint(late[0]["k"].tolist())


def test_old_entry_points_give_records_without_the_new_bits(gpu_required, designed):
    nat = gpu_required
    x = designed[0]
    pt = nat.TsbkParams(capacity=0)
    recs = {}
    with nat.Frontend(FS, device=0, block_capacity=len(x)) as fe:
        cs = [p25.c4fm_demod(fe, fe.chan_open(CR, OFF), CR, 4800, hard=True) for _ in range(3)]
        assert nat.lib().rcf_chan_tsbk(fe._h, cs[0], ctypes.byref(pt)) == nat.RCF_OK
        assert nat.lib().rcf_chan_tsbk_ex(fe._h, cs[1], ctypes.byref(pt), 1) == nat.RCF_OK
        assert nat.lib().rcf_chan_tsbk_opt(fe._h, cs[2], ctypes.byref(pt), 1, 1) == nat.RCF_OK
        fe.push(x)
        for i, c in enumerate(cs):
            recs[i] = _got(fe, c)
        own = [_streams(fe, c) for c in cs]
    want = [_rule(own[0], 0, 0), _rule(own[1], 1, 0), _rule(own[2], 1, 1)]
    plain = T.run(*own[0])
    for i in range(3):
        _same(recs[i][0], want[i][0], i)
        assert recs[i][1:] == want[i][1:]
    _same(recs[0][0], plain[0], "rcf_chan_tsbk")
    assert not np.any(recs[0][0]["frame_dibits"] >> 16) and not np.any((recs[1][0]["frame_dibits"] >> 21) & 0x1ff) and recs[0][3] == recs[1][3] == NONE
    assert np.all((recs[1][0]["frame_dibits"] >> 20) & 1) and np.any((recs[2][0]["frame_dibits"] >> 29) & 1) and recs[2][3]["n_decoded"] > 40


def test_the_pump_delivers_a_viterbi_stage_as_a_twins_single_reads(gpu_required):
    """delivery is unchanged, so one case: a "tsbk" slot on a Viterbi stage, whole, against the twin's reads block by block"""
    nat = gpu_required
    n_blocks = 40
    total = HD.D * HD.BLK * n_blocks
    d = V.designed_dibits(NAC)[0][:int(total * 4800 / HD.FS) + 9]
    xs = [F.c4fm_carrier(d, 4800, HD.FS, HD.F_TSDU + 150.0, 0.5, 600.0)[:total].astype(np.complex64)]

    def opener(nat_, m):
        fe = HD._frontend(nat_)
        c = HD._chain(nat_, fe, "tsbk", HD.F_TSDU, stage=False)
        fe.chan_tsbk(c, nid=True, viterbi=True)
        return fe, [c]
    f = HD._Fed(nat, xs, n_blocks, opener, max_read=8)
    try:
        e = f.pump.subscribe(0, f.ids[0][0], "tsbk")
        f.finish()
        got, written = f.pump.read(e), f.pump.written(e)
    finally:
        f.close()
    parts, vst = [], None
    for b, tw, ids_t in f.twin(0):
        parts.append(tw.chan_read_tsbk(ids_t[0]))
        vst = tw.chan_trellis_state(ids_t[0])
    s = np.concatenate(parts)
    _same(got, s, "the slot")
    v = nat.trellis_fields(s)
    print("pump: %d records, trellis %s" % (len(s), vst))
    assert written == len(s) > 8 and vst["n_decoded"] == int(v["viterbi"].sum()) > 0 and vst["n_bits"] == int(v["cost"].sum())
