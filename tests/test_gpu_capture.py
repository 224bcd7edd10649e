"""Carrier-operated capture on the GPU (radiocapture-rf_amd/csrc/capture.hip; definition: include/rcf.h at rcf_chan_capture).

Every comparison is bit for bit against the numpy restatement (tests/capture_ref.py) run on the channel's own
rcf_chan_read_iq: the captured stream, every record field and the state, after every push -- on a direct channel, a chained
one and a bin tap, whole, block by block and ragged; 130 channels in one launch; rings that wrap and a reader that lags
past them; the stage's lifecycle and every refusal; a group of two rates; a NaN-poisoned member beside a clean one; through
the counter-fed pump against a twin's direct reads; and rcf.scanner.Scanner end to end.
Shapes are those of tests/test_gpu_squelch.py: FS = 400 kS/s, blocks of 16000 inputs = 1000 channel outputs."""
import math

import numpy as np
import pytest

import capture_ref as R
import delivery_ref
import squelch_ref
from oracle import grspec as G
from rcf import scanner
from test_gpu_hard_delivery import _Fed
from test_gpu_squelch import BLK, CUTTINGS, FS, N_BLOCKS, carriers

pytestmark = pytest.mark.gpu

REC = R.REC_DTYPE
PRE_HANG = [(0, 0), (1, 64), (65, 63), (200, 300)]


def same_level(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def hold(got, ref, what):
    """captured stream (bits), records (bytes) and state against the restatement's"""
    cap, recs, st = got
    assert cap.dtype == np.complex64 and len(cap) == len(ref["captured"]), (what, len(cap), len(ref["captured"]))
    assert cap.tobytes() == ref["captured"].tobytes(), what
    assert recs.dtype == REC and recs.tobytes() == ref["records"].tobytes(), (what, recs, ref["records"])
    want = dict(ref["state"])
    st = dict(st)
    assert same_level(st.pop("level"), want.pop("level")), (what, st, ref["state"])
    assert st == want, (what, st, want)
    assert R.records_ok(recs, 0 if not len(recs) else int(recs[0]["sample"]))


class Tracker:
    """one channel's stage read after every push: the pieces add up to the streams; check() holds every prefix"""

    def __init__(self, fe, cid, db, alpha, pre, hang, a=0, first_index=0):
        """a: how many of the samples read here lie before the attach point; first_index: the attach point's channel index"""
        self.fe, self.cid, self.db, self.alpha, self.pre, self.hang, self.a, self.first_index = fe, cid, db, alpha, pre, hang, a, first_index
        self.iq, self.cap, self.recs, self.states, self.cuts = [], [], [], [], []

    def read(self):
        fe, cid = self.fe, self.cid
        self.iq.append(fe.chan_read_iq(cid))
        self.recs.append(fe.chan_read_capture_rec(cid))
        self.cap.append(fe.chan_read_capture(cid))
        self.states.append(fe.chan_capture_state(cid))
        self.cuts.append(sum(len(p) for p in self.iq) - self.a)

    def check(self, what):
        """-> the restatement of the whole stream (from the attach point a, counted in the samples read here)"""
        y = np.concatenate(self.iq)[self.a:]
        cuts = [max(c, 0) for c in self.cuts]
        refs = R.prefixes(y, squelch_ref.threshold(self.db), self.alpha, self.pre, self.hang, cuts, a=self.first_index)
        for k, ref in enumerate(refs):
            got = (np.concatenate(self.cap[:k + 1]), np.concatenate(self.recs[:k + 1]), self.states[k])
            hold(got, ref, (what, self.cid, k, cuts[k]))
        return refs[-1], cuts


def open_runs(is_open):
    """[(first, last + 1)] of the runs of open samples"""
    d = np.diff(np.concatenate(([0], is_open.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)))


# ------------------------------------------------------------------------------------------------ three channel kinds
@pytest.mark.parametrize("pre,hang", PRE_HANG)
@pytest.mark.parametrize("cutting", sorted(CUTTINGS))
def test_direct_chained_and_tap_channels_equal_the_restatement_bit_for_bit(gpu_required, cutting, pre, hang):
    nat = gpu_required
    n = N_BLOCKS * BLK
    # in channel samples (x 16 inputs): a keying across the first block cut, a second one 60 samples behind it -- muted for
    # fewer than 65 of them, so every (pre, hang) but (0, 0) merges the two --, a third far behind both
    on = [(600 * 16, 1400 * 16), (1460 * 16, 1800 * 16), (4000 * 16, 4600 * 16)]
    # the tap runs at 5 kS/s (80 inputs a sample, 200 a block): keyings at its samples 100..200 and 230..300 (a gap of 30)
    # and 900..1000 (a gap of 600 > 200 + 300)
    on_tap = [(100 * 80, 200 * 80), (230 * 80, 300 * 80), (900 * 80, 1000 * 80)]
    f_tap = 7 * FS / 160
    x = carriers(n, [(50e3, 0.1, on), (-90e3, 0.1, on), (f_tap, 0.1, on_tap)], 3)
    proto = G.low_pass_2(1.0, FS, 1000.0, 1250.0, 20.0, G.WIN_HAMMING)
    taps2 = G.low_pass_2(1.0, 50e3, 6250.0, 6250.0, 20.0, G.WIN_HAMMING)
    cuts = squelch_ref.ragged_cuts(n, CUTTINGS[cutting])
    with nat.Frontend(FS, block_capacity=n, out_capacity=1 << 14) as fe:
        direct = fe.chan_open(12500, 50e3)
        wide = fe.chan_open(25000, -90e3 + 1000.0)
        chained = fe.chan_open_taps(wide, 2, taps2, -1000.0)
        fe.pfb_open(160, 80, proto)
        tap = fe.pfb_tap_open(7, gr_phase=False)
        params = {direct: (-30.0, 0.1), chained: (-33.0, 0.5), tap: (-28.0, 1.0)}
        tr = {}
        for cid, (db, alpha) in params.items():
            fe.chan_capture(cid, db, alpha, pre=pre, hang=hang)
            tr[cid] = Tracker(fe, cid, db, alpha, pre, hang)
        for a, b in zip(cuts[:-1], cuts[1:]):
            fe.push(x[a:b])
            for t in tr.values():
                t.read()
    for cid, t in tr.items():
        ref, ccuts = t.check(cutting)
        # the census, on the restatement: the keyed carriers make every case
        w = R.census(ref, pre, hang)["windows"]
        assert len(w) >= 2, (cid, w)
        if pre + hang > 0:                      # (nothing lies closer than 0 samples: (0, 0) merges nothing)
            runs = open_runs(ref["open"])
            merged = [1 for lo, hi in w if sum(1 for r0, r1 in runs if lo <= r0 and (hi is None or r1 <= hi)) >= 2]
            assert merged, (cid, w, runs)
        if cutting != "whole":                  # a window open across a block cut
            inner = sorted(set(c for c in ccuts[:-1] if c > 0))
            assert any(lo < c <= (hi if hi is not None else 1 << 60) for lo, hi in w for c in inner), (cid, w, inner)
        assert ref["state"]["n_seen"] == t.cuts[-1] and ref["state"]["n_decided"] == t.cuts[-1] - pre


# ------------------------------------------------------------------------------------------------ 130 lanes
def test_130_channels_in_one_launch_mixed_parameters_batched_reads(gpu_required):
    """three waves, the last of two lanes; thresholds, alphas, pre and hang differ from lane to lane; lanes far from a
    carrier never open, lane 5 is open throughout.  Read through the batched readers (rcf_chan_read_many), both streams"""
    nat = gpu_required
    n_ch, n = 130, 4 * BLK
    offs = [-190e3 + 2900.0 * i for i in range(n_ch)]
    keyed = {0: 0.05, 63: 0.08, 64: 0.05, 129: 0.08, 17: 0.05, 100: 0.05}
    spec = [(offs[i], a, [(9000 + 700 * (i % 9), 30000 + 900 * (i % 5)), (41000, 52000 + 100 * (i % 13))]) for i, a in keyed.items()]
    x = carriers(n, spec, 5)
    dbs = [-34.0 - (i % 5) * 2.0 for i in range(n_ch)]
    dbs[5] = -300.0                                                   # open from its first sample on
    alphas = [(0.1, 0.01, 1.0, 0.5)[i % 4] for i in range(n_ch)]
    pres = [(0, 1, 63, 64, 65, 200, 7)[i % 7] for i in range(n_ch)]
    hangs = [(0, 64, 1, 300, 63, 5)[i % 6] for i in range(n_ch)]
    with nat.Frontend(FS, block_capacity=BLK, out_capacity=1 << 13) as fe:
        cids = [fe.chan_open(12500, f) for f in offs]
        assert cids == sorted(cids)                                   # one (D, T) class: the lanes are in id order
        for cid, db, a, p, h in zip(cids, dbs, alphas, pres, hangs):
            fe.chan_capture(cid, db, a, pre=p, hang=h)
        cap, recs = [[] for _ in cids], [[] for _ in cids]
        for b in range(4):
            fe.push(x[b * BLK:(b + 1) * BLK])
            for acc, what, ce in ((recs, "capture_rec", 64), (cap, "capture", 1024)):
                rows = fe.chan_read_many(cids, what, cap_each=ce)
                for lane, r in enumerate(rows):
                    assert r is not None
                    acc[lane].append(r.copy())
        iq = np.stack([fe.chan_read_iq(c) for c in cids], axis=1)
        states = [fe.chan_capture_state(c) for c in cids]
    assert iq.shape == (4000, n_ch)
    never = throughout = 0
    for lane in range(n_ch):
        ref = R.run(iq[:, lane], squelch_ref.threshold(dbs[lane]), alphas[lane], pres[lane], hangs[lane])
        hold((np.concatenate(cap[lane]), np.concatenate(recs[lane]), states[lane]), ref, ("lane", lane))
        never += not ref["open"].any()
        throughout += bool(ref["open"].all())
        if lane in (0, 63, 64, 129):
            assert ref["state"]["n_windows"] >= 1 and 0 < ref["state"]["n_kept"] < 4000 - pres[lane], (lane, ref["state"])
    assert never >= 1 and throughout >= 1 and never + throughout < n_ch


# ------------------------------------------------------------------------------------------------ rings that wrap
def test_rings_wrap_and_a_reader_that_lags_past_them(gpu_required):
    """capacity 2048 under more than four capacities of kept samples, rec_capacity 16 under more than 64 records: a reader
    after every block gets everything, one that reads at the end exactly the newest ring's worth (lag_clamp)"""
    nat = gpu_required
    n_blocks, period, on_len = 14, 160, 100
    n = n_blocks * BLK
    on = [(k * period * 16, (k * period + on_len) * 16) for k in range(1, n // 16 // period)]
    x = carriers(n, [(50e3, 0.1, on)], 11)
    with nat.Frontend(FS, block_capacity=BLK, out_capacity=1 << 14) as fe:
        prompt = fe.chan_open(12500, 50e3)
        lazy = fe.chan_open(12500, 50e3 + 50.0)
        for cid in (prompt, lazy):
            fe.chan_capture(cid, -30.0, 1.0, pre=2, hang=3, capacity=2048, rec_capacity=16)
        assert fe.chan_capture_rings(prompt)[1::2] == (2048, 16)
        t = Tracker(fe, prompt, -30.0, 1.0, 2, 3)
        for b in range(n_blocks):
            fe.push(x[b * BLK:(b + 1) * BLK])
            t.read()
        lazy_got = (fe.chan_read_capture(lazy), fe.chan_read_capture_rec(lazy), fe.chan_capture_state(lazy))
        lazy_iq = fe.chan_read_iq(lazy)
        again = (fe.chan_read_capture(lazy), fe.chan_read_capture_rec(lazy))
    ref, _ = t.check("prompt")
    assert ref["state"]["n_kept"] > 4 * 2048 and ref["state"]["n_records"] > 64, ref["state"]
    assert max(len(r) for r in t.recs) <= 16 and max(len(c) for c in t.cap) <= 2048      # (the prompt reader never lagged a ring)
    lref = R.run(lazy_iq, squelch_ref.threshold(-30.0), 1.0, 2, 3)
    assert len(lazy_iq) == n // 16 and lref["state"]["n_kept"] > 4 * 2048 and lref["state"]["n_records"] > 64
    hold((lazy_got[0], lazy_got[1], lazy_got[2]), dict(captured=lref["captured"][-2048:], records=lref["records"][-16:], state=lref["state"]),
         "the newest ring's worth")
    assert len(again[0]) == 0 and len(again[1]) == 0


# ------------------------------------------------------------------------------------------------ lifecycle
def test_lifecycle_late_attach_again_detach_retune_close_and_beside_the_squelch(gpu_required):
    nat = gpu_required
    n = 7 * BLK
    x = carriers(n, [(50e3, 0.1, [(0, 2 * BLK + 3000), (3 * BLK + 4000, 3 * BLK + 9000), (4 * BLK + 3000, 5 * BLK + 8000), (6 * BLK + 2000, n)])], 9)
    blk = lambda b: x[b * BLK:(b + 1) * BLK]
    with nat.Frontend(FS, block_capacity=BLK, out_capacity=1 << 13) as fe:
        cid = fe.chan_open(12500, 50e3)
        fe.chan_squelch(cid, -36.0, 0.05)                             # the reporting stage beside it, other parameters
        fe.push(blk(0)); fe.push(blk(1))
        fe.chan_capture(cid, -30.0, 0.1, pre=150, hang=40)            # two blocks late: a = 2000, inside a transmission
        late = Tracker(fe, cid, -30.0, 0.1, 150, 40, a=2000, first_index=2000)     # (its first read takes samples 0 .. 3000)
        fe.push(blk(2)); late.read()
        fe.push(blk(3)); late.read()
        fe.chan_capture(cid, -33.0, 0.5, pre=7, hang=9)               # again: everything from item 0, a = 4000
        fresh = (fe.chan_read_capture(cid), fe.chan_read_capture_rec(cid), fe.chan_capture_state(cid))
        again = Tracker(fe, cid, -33.0, 0.5, 7, 9, a=0, first_index=4000)
        fe.push(blk(4)); again.read()
        fe.chan_set_offset(cid, 50e3 + 20.0)                          # a retune keeps the stage and its streams
        fe.push(blk(5)); again.read()
        sq = fe.chan_squelch_state(cid)
        fe.chan_capture(cid, None)                                    # detached: the readers and the state refuse
        for call in (fe.chan_read_capture, fe.chan_read_capture_rec, fe.chan_capture_state, fe.chan_capture_rings):
            with pytest.raises(nat.RcfError) as e:
                call(cid)
            assert e.value.code == nat.RCF_ESTATE, call
        assert fe.chan_read_many([cid], "capture")[0] is None and fe.chan_read_many([cid], "capture_rec")[0] is None
        fe.chan_capture(cid, None)                                    # off twice: nothing to do
        fe.push(blk(6))                                               # the block goes on without the stage
        assert fe.chan_squelch_state(cid)["n_seen"] == 7000
        fe.chan_capture(cid, -30.0, 0.1)
        fe.chan_close(cid)                                            # the channel takes its stage along
        with pytest.raises(nat.RcfError) as e:
            fe.chan_capture_state(cid)
        assert e.value.code == nat.RCF_ENOCHAN
        fe.push(blk(0))
    ref, _ = late.check("late")
    assert ref["records"][0]["kind"] == R.OPEN and ref["records"][0]["sample"] == 2000      # clipped at the attach point
    assert fresh[2] == dict(level=0.0, n_seen=0, n_decided=0, n_kept=0, n_records=0, n_windows=0, last_open=-1, in_window=0, unmuted=0)
    assert len(fresh[0]) == 0 and len(fresh[1]) == 0
    ref2, _ = again.check("again")
    assert ref2["state"]["n_windows"] >= 1 and ref2["records"][0]["pos"] == 0 and ref2["records"][0]["sample"] >= 4000
    # the squelch beside it saw every sample with its own parameters
    y = np.concatenate(late.iq + again.iq)
    assert len(y) == 6000 and sq["n_seen"] == 6000
    sref = squelch_ref.run(y, squelch_ref.threshold(-36.0), 0.05)
    assert sq["n_open"] == int(sref["n_open"]) and same_level(sq["level"], float(sref["level"]))


def test_refusals(gpu_required):
    nat = gpu_required
    proto = G.low_pass_2(1.0, FS, 1000.0, 1250.0, 20.0, G.WIN_HAMMING)
    with nat.Frontend(FS, block_capacity=BLK, out_capacity=1 << 13) as fe:
        cid = fe.chan_open(12500, 0.0)
        bad = [dict(threshold_db=-30.0, alpha=0.0), dict(threshold_db=-30.0, alpha=-0.1), dict(threshold_db=-30.0, alpha=1.5),
               dict(threshold_db=-30.0, alpha=float("nan")), dict(threshold_db=float("nan"), alpha=0.1), dict(threshold_db=float("inf"), alpha=0.1),
               dict(threshold_db=-30.0, alpha=0.1, pre=-1), dict(threshold_db=-30.0, alpha=0.1, hang=-1)]
        for kw in bad:
            with pytest.raises(nat.RcfError) as e:
                fe.chan_capture(cid, **kw)
            assert e.value.code == nat.RCF_EINVAL, kw
        fe.chan_capture(cid, -30.0, 1.0)                              # alpha 1 is inside (0, 1]
        # RCF_ECAP: pre + the most outputs a block can give the channel (16000 / 16 + 1 = 1001) must fit the ring of 8192
        fe.chan_capture(cid, -30.0, 0.1, pre=8192 - 1001)
        with pytest.raises(nat.RcfError) as e:
            fe.chan_capture(cid, -30.0, 0.1, pre=8192 - 1000)
        assert e.value.code == nat.RCF_ECAP
        assert fe.chan_capture_state(cid)["n_seen"] == 0              # a refused call leaves the stage that was there
        # capacities: rounded up to powers of two, 0 the defaults, floors 64 and 16
        fe.chan_capture(cid, -30.0, 0.1, capacity=1000, rec_capacity=17)
        assert fe.chan_capture_rings(cid)[1::2] == (1024, 32)
        fe.chan_capture(cid, -30.0, 0.1, capacity=3, rec_capacity=3)
        assert fe.chan_capture_rings(cid)[1::2] == (64, 16)
        fe.chan_capture(cid, -30.0, 0.1)
        assert fe.chan_capture_rings(cid)[1::2] == (8192, 256)
        for call in (lambda: fe.chan_capture(cid + 99, -30.0, 0.1), lambda: fe.chan_capture_state(cid + 99),
                     lambda: fe.chan_read_capture(cid + 99), lambda: fe.chan_read_capture_rec(cid + 99), lambda: fe.chan_capture_rings(cid + 99)):
            with pytest.raises(nat.RcfError) as e:
                call()
            assert e.value.code == nat.RCF_ENOCHAN
        fe.pfb_open(160, 80, proto)
        tap = fe.pfb_tap_open(3, gr_phase=False)
        fe.chan_set_fm_only(tap, True)
        with pytest.raises(nat.RcfError) as e:                        # no IQ ring
            fe.chan_capture(tap, -30.0, 0.1)
        assert e.value.code == nat.RCF_ESTATE
        fe.chan_set_fm_only(tap, False)
        fe.chan_capture(tap, -30.0, 0.1)
        with pytest.raises(nat.RcfError) as e:                        # ... and none may be taken from under the stage
            fe.chan_set_fm_only(tap, True)
        assert e.value.code == nat.RCF_ESTATE
        # the tap's rule: 16000 / 80 + 1 = 201 frames, / 1 + 1 = 202 outputs
        fe.chan_capture(tap, -30.0, 0.1, pre=8192 - 202)
        with pytest.raises(nat.RcfError) as e:
            fe.chan_capture(tap, -30.0, 0.1, pre=8192 - 201)
        assert e.value.code == nat.RCF_ECAP
        fe.chan_capture(tap, None)
        fe.chan_set_fm_only(tap, True)
        # the unknown streams stay unknown to the batched reader
        for what in (21, 34, 50, 52, -1, 3, 15):
            ids = (nat.C.c_int * 1)(cid)
            counts = (nat.C.c_int64 * 1)()
            buf = np.zeros(64, np.complex64)
            assert nat.lib().rcf_chan_read_many(fe._h, what, ids, 1, nat.C.c_float(1.0), buf.ctypes.data_as(nat.C.c_void_p), 8, counts) == nat.RCF_EINVAL


# ------------------------------------------------------------------------------------------------ groups
def _member(nat, fs, blk, x, grouped_with=None):
    fe = nat.Frontend(fs, device=0, block_capacity=blk, out_capacity=1 << 13)
    cids = [fe.chan_open(12500, 50e3), fe.chan_open(12500, -70e3)]
    par = ((-30.0, 0.1, 20, 30), (-33.0, 0.5, 0, 5))
    for cid, (db, a, p, h) in zip(cids, par):
        fe.chan_capture(cid, db, a, pre=p, hang=h)
    return fe, cids, par


def _run_members(nat, specs, grouped):
    """specs: [(fs, block, x)]; three blocks each, as one group (one launch for every lane) or one by one"""
    ms = [_member(nat, fs, blk, x) for fs, blk, x in specs]
    fes = [m[0] for m in ms]
    try:
        if grouped:
            with nat.Group(fes) as g:
                for b in range(3):
                    g.push([x[b * blk:(b + 1) * blk] for _, blk, x in specs])
                g.sync()
                pairs = [(m, c) for m, (_, cids, _) in enumerate(ms) for c in cids]
                caps = g.read_many(pairs, "capture", cap_each=1 << 12)
                recs = g.read_many(pairs, "capture_rec", cap_each=256)
                out, k = [], 0
                for fe, cids, par in ms:
                    out.append([(fe.chan_read_iq(c), caps[k + i].copy(), recs[k + i].copy(), fe.chan_capture_state(c)) for i, c in enumerate(cids)])
                    k += len(cids)
                return out
        for (fe, _, _), (_, blk, x) in zip(ms, specs):
            for b in range(3):
                fe.push(x[b * blk:(b + 1) * blk])
        return [[(fe.chan_read_iq(c), fe.chan_read_capture(c), fe.chan_read_capture_rec(c), fe.chan_capture_state(c)) for c in cids]
                for fe, cids, _ in ms]
    finally:
        for fe in fes:
            fe.close()


def _carriers_at(fs, n, spec, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (1e-3 / math.sqrt(2))
    for off, amp, ranges in spec:
        env = np.zeros(n)
        for a, b in ranges:
            env[a:b] = amp
        x += env * np.exp(2j * np.pi * off * t + 2j * np.pi * rng.random())
    return x.astype(np.complex64)


def test_a_group_of_two_rates_equals_the_front_ends_alone(gpu_required):
    par = ((-30.0, 0.1, 20, 30), (-33.0, 0.5, 0, 5))
    on = [(7000, 20000), (30000, 41000)]
    specs = [(FS, BLK, _carriers_at(FS, 3 * BLK, [(50e3, 0.1, on), (-70e3, 0.1, on[1:])], 21)),
             (2 * FS, 2 * BLK, _carriers_at(2 * FS, 6 * BLK, [(50e3, 0.07, [(14000, 40000)]), (-70e3, 0.1, [(a * 2, b * 2) for a, b in on])], 22))]
    together = _run_members(gpu_required, specs, grouped=True)
    alone = _run_members(gpu_required, specs, grouped=False)
    for m in range(2):
        for (y, cap, recs, st), (y1, cap1, recs1, st1), (db, a, p, h) in zip(together[m], alone[m], par):
            assert len(y) == 3000 and y.tobytes() == y1.tobytes()
            assert cap.tobytes() == cap1.tobytes() and recs.tobytes() == recs1.tobytes() and st == st1
            ref = R.run(y, squelch_ref.threshold(db), a, p, h)
            hold((cap, recs, st), ref, ("member", m, db))
            assert ref["state"]["n_windows"] >= 1


def test_a_nan_burst_on_one_member_leaves_the_other_members_lanes_alone(gpu_required):
    """member 0's input carries a NaN burst: its lanes go NaN and muted for good, the window before the burst closes normally;
    member 1's lanes, in the same launch, are bit-identical to their run alone"""
    par = ((-30.0, 0.1, 20, 30), (-33.0, 0.5, 0, 5))
    n = 3 * BLK
    on = [(7000, 20000), (30000, 41000)]
    x0 = carriers(n, [(50e3, 0.1, [(0, BLK)]), (-70e3, 0.1, on[:1])], 21)
    x1 = carriers(n, [(50e3, 0.07, on[:1]), (-70e3, 0.1, on)], 22)
    x0[BLK + 9000:BLK + 9040] = complex(np.nan, np.nan)
    specs = [(FS, BLK, x0), (FS, BLK, x1)]
    together = _run_members(gpu_required, specs, grouped=True)
    alone = _run_members(gpu_required, specs, grouped=False)
    for (y, cap, recs, st), (db, a, p, h) in zip(together[0], par):
        ref = R.run(y, squelch_ref.threshold(db), a, p, h)
        hold((cap, recs, st), ref, ("nan lane", db))
        first_nan = int(np.flatnonzero(np.isnan(y.real) | np.isnan(y.imag))[0])
        assert math.isnan(st["level"]) and st["unmuted"] == 0 and st["in_window"] == 0 and st["last_open"] < first_nan
        assert len(recs) >= 2 and recs[-1]["kind"] == R.CLOSE and recs[-1]["sample"] <= first_nan + h + 1     # closed normally
        assert not np.isnan(cap.view(np.float32)).any()
    for (y, cap, recs, st), (y1, cap1, recs1, st1) in zip(together[1], alone[1]):
        assert y.tobytes() == y1.tobytes() and cap.tobytes() == cap1.tobytes() and recs.tobytes() == recs1.tobytes() and st == st1
        assert not math.isnan(st["level"]) and st["n_windows"] >= 1


# ------------------------------------------------------------------------------------------------ the pump
P_BLK = 1000
P_PRE, P_HANG = 6, 9


def _pump_signal(n_blocks, seed, period=125, on_len=60):
    n = n_blocks * P_BLK * 16
    on = [(k * period * 16, (k * period + on_len) * 16) for k in range(1, n // 16 // period)]
    return carriers(n, [(50e3, 0.1, on), (-70e3, 0.1, on[::3])], seed)


def _pump_opener(rec_capacity=256, capacity=0):
    def opener(nat, m):
        fe = nat.Frontend(FS, 0.0, device=0, block_capacity=16 * P_BLK, out_capacity=1 << 12)
        ids = [fe.chan_open(12500, 50e3), fe.chan_open(12500, -70e3), fe.chan_open(12500, 10e3)]
        fe.chan_capture(ids[0], -30.0, 1.0, pre=P_PRE, hang=P_HANG, capacity=capacity, rec_capacity=rec_capacity)
        fe.chan_capture(ids[1], -30.0, 0.5, pre=P_PRE, hang=P_HANG, capacity=capacity, rec_capacity=rec_capacity)
        return fe, ids                                                # (ids[2] carries no stage: its slot starves)
    return opener


def _twin_streams(f, m, keys, reattach_at=None):
    parts, counters = {key: [] for key in keys}, {key: [] for key in keys}
    for b, tw, ids_t in f.twin(m):
        for (k, what) in keys:
            parts[(k, what)].append(tw.chan_read_capture(ids_t[k]) if what == "capture" else tw.chan_read_capture_rec(ids_t[k]))
            st = tw.chan_capture_state(ids_t[k])
            counters[(k, what)].append(st["n_kept"] if what == "capture" else st["n_records"])
        if reattach_at is not None and b + 1 == reattach_at:
            tw.chan_capture(ids_t[0], -30.0, 1.0, pre=P_PRE, hang=P_HANG)
    return parts, counters


def test_pump_delivers_both_streams_late_subscription_small_ring_and_bounds(gpu_required):
    """slots "capture" and "capture_rec" against a twin's direct reads: subscribed when the pump has run two blocks (the
    channel's reader still stands at item 0, the rings hold everything: the streams are whole), host rings of 64 x 8 bytes
    (64 samples, 16 records) under blocks that make hundreds of samples -- the reader after every block gets what
    delivery_ref's replay of the documented gather says, with the stated per-block bounds (rcf_streams.h: n_k samples,
    2 (n_k / (pre + hang + 2)) + 4 records) -- and a channel without the stage starves its slot"""
    nat = gpu_required
    n_blocks, late = 10, 2
    xs = [_pump_signal(n_blocks, 31), _pump_signal(n_blocks, 32, period=200, on_len=90)]
    keys = [(0, "capture"), (0, "capture_rec"), (1, "capture"), (1, "capture_rec")]
    rec_bound = 2 * (P_BLK // (P_PRE + P_HANG + 2)) + 4
    for ring in (1 << 13, 64):
        f = _Fed(nat, xs, n_blocks, _pump_opener(), out_ring_samples=ring, max_read=12, blk=P_BLK)
        reads = {}
        try:
            pump = f.pump
            for b in range(n_blocks):
                f.feed(b + 1)
                if b + 1 == late:
                    slots = {(m, key): pump.subscribe(m, f.ids[m][key[0]], key[1]) for m in range(2) for key in keys}
                    starved = pump.subscribe(0, f.ids[0][2], "capture")
                    assert all(pump._cursors[e].value == 0 for e in slots.values())
                    reads = {k: [] for k in slots}
                if b + 1 > late:
                    for k, e in slots.items():
                        before = pump._cursors[e].value
                        r = pump.read(e)
                        reads[k].append((b, before, pump._cursors[e].value, r, pump.written(e)))
            assert pump.written(starved) == 0
            for what in ("capture", "capture_rec"):                   # the pump cannot be STARTED with either
                with pytest.raises(nat.RcfError) as e:
                    nat.Pump(f.grp, f.rings, 16 * P_BLK, FS, [(0, f.ids[0][0])], fmt=nat.FMT_CF32, what=what, written=f.counters)
                assert e.value.code == nat.RCF_EINVAL
            cur = nat.C.c_int64(0)                                    # ... and each entry point takes its own of the two only
            assert nat.lib().rcf_pump_subscribe(pump._p, 0, f.ids[0][0], nat.HARD_CAPTURE, nat.C.c_float(1.0), nat.C.byref(cur)) == nat.RCF_EINVAL
            assert nat.lib().rcf_pump_subscribe_hard(pump._p, 0, f.ids[0][0], nat.READ_CAPTURE, nat.C.byref(cur)) == nat.RCF_EINVAL
        finally:
            f.close()
        for m in range(2):
            parts, counters = _twin_streams(f, m, keys)
            for key in keys:
                s = np.concatenate(parts[key])
                c = counters[key]
                room = ring if key[1] == "capture" else ring // 4
                bounds = [P_BLK if key[1] == "capture" else rec_bound] * n_blocks
                cap = 1 << 12 if key[1] == "capture" else 256
                idx, items, per, w = delivery_ref.replay_slot(s, c, bounds, cap=cap, room=room, first=late)
                taken = s[np.asarray(idx, dtype=np.int64)]
                assert c[-1] == len(s) > (300 if key[1] == "capture" else 20), (key, c)
                if ring >= 1 << 13:
                    assert idx == list(range(len(s)))                 # whole, from item 0: the late subscription lost nothing
                else:
                    assert len(idx) < len(s) or key[1] == "capture_rec"
                got = []
                for b, before, after, r, written in reads[(m, key)]:
                    n_at_b = sum(n for _, n in per[:b - late + 1])
                    assert written == n_at_b, (m, key, b, written, n_at_b)          # the bounds held in every gather
                    lo = max(before, written - room)
                    assert after == written and after - len(r) == lo, (m, key, b, before, after, len(r), written)
                    assert r.tobytes() == taken[lo:written].tobytes(), (m, key, b)
                    got.append(r)
                assert w == len(taken)
                if ring >= 1 << 13:
                    assert np.concatenate(got).tobytes() == s.tobytes()
                # the steady-state gathers stay inside the stated bounds
                assert all(n <= bounds[0] for _, n in per[1:])


def test_pump_stage_attached_again_under_a_subscription_is_appended_without_a_gap(gpu_required):
    nat = gpu_required
    n_blocks, again_at = 8, 4
    xs = [_pump_signal(n_blocks, 41)]
    keys = [(0, "capture"), (0, "capture_rec")]
    f = _Fed(nat, xs, n_blocks, _pump_opener(), out_ring_samples=1 << 13, max_read=4, blk=P_BLK)
    try:
        pump = f.pump
        slots = {key: pump.subscribe(0, f.ids[0][key[0]], key[1]) for key in keys}
        f.feed(again_at)
        f.fes[0].chan_capture(f.ids[0][0], -30.0, 1.0, pre=P_PRE, hang=P_HANG)         # a fresh stage: both streams at item 0
        f.finish()
        got = {key: pump.read(e) for key, e in slots.items()}
        written = {key: pump.written(e) for key, e in slots.items()}
    finally:
        f.close()
    parts, counters = _twin_streams(f, 0, keys, reattach_at=again_at)
    for key in keys:
        want = np.concatenate(parts[key])
        assert len(parts[key][again_at]) > 0 and counters[key][again_at] < counters[key][again_at - 1]     # (the count restarted)
        assert written[key] == len(want) and got[key].tobytes() == want.tobytes(), key


# ------------------------------------------------------------------------------------------------ the scanner, end to end
def test_scanner_hands_over_every_transmission_on_grid_and_off_grid(gpu_required):
    nat = gpu_required
    n_blocks = 10
    n = n_blocks * BLK
    fc = 155e6
    f_on, f_off = fc + 7 * FS / 160, fc + 51300.0                    # a bin of the 160-bin bank; off its 2.5 kHz grid
    tx = [(16000, 40000), (70000, 90000), (120000, 140000)]
    x = carriers(n, [(f_on - fc, 0.1, tx), (f_off - fc, 0.1, tx)], 17)
    proto = G.low_pass_2(1.0, FS, 1000.0, 1250.0, 20.0, G.WIN_HAMMING)
    calls, iq = [], {}
    with nat.Frontend(FS, fc, block_capacity=BLK, out_capacity=1 << 14) as fe:
        fe.pfb_open(160, 80, proto)
        sc = scanner.Scanner({"id": 1, "channels": {"a": f_on, "b": f_off}, "threshold": -30.0, "modulation": "analog"}, fe,
                             lambda f: None, n_bins=160, capture=dict(pre_s=0.010, hang_s=0.020),
                             on_call=lambda f, rec, w: calls.append((f, rec, w)))
        assert sc.bins == {f_on: 7} and list(sc.chans) == [f_off]
        assert (sc.cap[f_on]["pre"], sc.cap[f_on]["hang"], sc.cap[f_off]["pre"], sc.cap[f_off]["hang"]) == (50, 100, 250, 500)
        cids = {f: k["cid"] for f, k in sc.cap.items()}
        iq = {f: [] for f in cids}
        for b in range(n_blocks):
            fe.push(x[b * BLK:(b + 1) * BLK])
            sc.poll()
            for f, cid in cids.items():
                iq[f].append(fe.chan_read_iq(cid))
        sc.close()
    for f in (f_on, f_off):
        y = np.concatenate(iq[f])
        mine = [(rec, w) for g, rec, w in calls if g == f]
        assert len(mine) == 3, (f, [r for r, _ in mine])              # once per transmission
        rate = 5000.0 if f == f_on else 25000.0
        for (rec, w), (t0, t1) in zip(mine, tx):
            assert rec["lost"] == 0 and rec["rate"] == rate and rec["n_open"] > 0 and rec["peak"] > 0
            assert w.tobytes() == y[rec["sample"]:rec["end"]].tobytes() and len(w) == rec["end"] - rec["sample"]
            # the head is there: the window begins pre samples before the detector opened, near the key-on
            k0, k1 = t0 * rate / FS, t1 * rate / FS
            assert k0 - rec["rate"] * 0.010 - 8 <= rec["sample"] <= k0 and k1 <= rec["end"] <= k1 + rec["rate"] * 0.020 + 40, (f, rec, k0, k1)
