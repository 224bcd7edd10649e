"""Carrier detect on the GPU (radiocapture-rf_amd/csrc/squelch.hip; definition: include/rcf.h at rcf_chan_squelch).

Behind a channel the stage is exact: its state equals the numpy restatement (tests/squelch_ref.py) of the channel's own
rcf_chan_read_iq bit for bit -- whole, ragged and block by block, 130 channels in one launch, on a direct channel, a chained
one and a bin tap, attached late, attached again, in a group, and beside a lane that has gone NaN.
On every bin of a filterbank the recurrence is cut in time: per bin the level stays within the derived bound
64 x 2^-53 / alpha of the restatement of rcf_pfb_read_bin's own samples, and n_open, last_open and the mask are equal -- for one
bank per kernel family (one of them tiled), blocks of 0, 1, S-1, S, S+1 and 5S+3 frames, a ring that wraps, and a designed
keying whose census demands every way a bin can open and close against the segments."""
import math

import numpy as np
import pytest

import squelch_ref as R
from oracle import grspec as G

pytestmark = pytest.mark.gpu

FS, BLK = 400e3, 16000                    # a 12.5 kHz channel: D = 16, 1000 samples a block


def same_level(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def hold_state(st, ref, what, n=None, first_index=0):
    """the stage's state against the restatement's after its first n samples (all of them by default), bit for bit"""
    o = ref["open"] if n is None else ref["open"][:n]
    n = len(o)
    idx = np.flatnonzero(o)
    want = dict(n_seen=n, n_open=len(idx), first_open=int(idx[0]) + first_index if len(idx) else -1,
                last_open=int(idx[-1]) + first_index if len(idx) else -1, unmuted=int(o[-1]) if n else 0)
    level = float(ref["levels"][n - 1]) if n else 0.0
    got = dict(st)
    assert same_level(got.pop("level"), level), (what, st, level)
    assert got == want, (what, st, want)


def carriers(n, spec, seed, noise=1e-3):
    """wideband noise + carriers [(offset Hz, amplitude, [(on, off) in input samples])]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (noise / math.sqrt(2))
    for off, amp, ranges in spec:
        env = np.zeros(n)
        for a, b in ranges:
            env[a:b] = amp
        x += env * np.exp(2j * np.pi * off * t + 2j * np.pi * rng.random())
    return x.astype(np.complex64)


# ------------------------------------------------------------------------------------------------ behind a channel
N_BLOCKS = 6
CUTTINGS = {"whole": [N_BLOCKS * BLK], "blocks": [BLK] * N_BLOCKS,
            "ragged": [5, BLK, 7, 15, 16, 17, 1, 2 * BLK + 333, 31, BLK - 1, 1, 1024 + 9]}


@pytest.mark.parametrize("cutting", sorted(CUTTINGS))
def test_direct_chained_and_tap_channels_equal_the_restatement_bit_for_bit(gpu_required, cutting):
    """three channel kinds, three thresholds and alphas, the state held after every push (block by block)"""
    nat = gpu_required
    n = N_BLOCKS * BLK
    on = [(n // 7, n // 3), (n // 2, n // 2 + 700), (2 * n // 3, n - 5000)]
    f_tap = 7 * FS / 160
    x = carriers(n, [(50e3, 0.1, on), (-90e3, 0.1, on[1:]), (f_tap, 0.1, on[:2])], 3)
    proto = G.low_pass_2(1.0, FS, 1000.0, 1250.0, 20.0, G.WIN_HAMMING)
    taps2 = G.low_pass_2(1.0, 50e3, 6250.0, 6250.0, 20.0, G.WIN_HAMMING)
    cuts = R.ragged_cuts(n, CUTTINGS[cutting])
    with nat.Frontend(FS, block_capacity=n, out_capacity=1 << 14) as fe:
        direct = fe.chan_open(12500, 50e3)
        wide = fe.chan_open(25000, -90e3 + 1000.0)
        chained = fe.chan_open_taps(wide, 2, taps2, -1000.0)
        fe.pfb_open(160, 80, proto)
        tap = fe.pfb_tap_open(7, gr_phase=False)
        params = {direct: (-30.0, 0.1), chained: (-33.0, 0.01), tap: (-28.0, 1.0)}
        for cid, (db, alpha) in params.items():
            fe.chan_squelch(cid, db, alpha)
        iq = {cid: [] for cid in params}
        states = {cid: [] for cid in params}
        for a, b in zip(cuts[:-1], cuts[1:]):
            fe.push(x[a:b])
            for cid in params:
                iq[cid].append(fe.chan_read_iq(cid))
                states[cid].append(fe.chan_squelch_state(cid))
    for cid, (db, alpha) in params.items():
        y = np.concatenate(iq[cid])
        ref = R.run(y, R.threshold(db), alpha)
        assert 0 < ref["n_open"] < len(y), (cid, int(ref["n_open"]), len(y))
        at = 0
        for part, st in zip(iq[cid], states[cid]):
            at += len(part)
            hold_state(st, ref, (cutting, cid, at), n=at)
        assert at == len(y) == states[cid][-1]["n_seen"]


def test_130_channels_in_one_launch_mixed_thresholds_and_alphas(gpu_required):
    """three waves, the last of two lanes: every lane against the restatement, lanes 0, 63, 64 and 129 by name"""
    nat = gpu_required
    n_ch, n = 130, 4 * BLK
    offs = [-190e3 + 2900.0 * i for i in range(n_ch)]
    keyed = {0: 0.05, 63: 0.08, 64: 0.05, 129: 0.08, 17: 0.05, 100: 0.05}
    spec = [(offs[i], a, [(9000 + 700 * (i % 9), 30000 + 900 * (i % 5)), (41000, 52000 + 100 * (i % 13))]) for i, a in keyed.items()]
    x = carriers(n, spec, 5)
    dbs = [-34.0 - (i % 5) * 2.0 for i in range(n_ch)]
    alphas = [(0.1, 0.01, 1.0, 0.5)[i % 4] for i in range(n_ch)]
    with nat.Frontend(FS, block_capacity=BLK, out_capacity=1 << 13) as fe:
        cids = [fe.chan_open(12500, f) for f in offs]
        assert cids == sorted(cids)                                   # one (D, T) class: the lanes are in id order
        for cid, db, a in zip(cids, dbs, alphas):
            fe.chan_squelch(cid, db, a)
        for b in range(4):
            fe.push(x[b * BLK:(b + 1) * BLK])
        iq = np.stack([fe.chan_read_iq(c) for c in cids], axis=1)
        states = [fe.chan_squelch_state(c) for c in cids]
    assert iq.shape == (4000, n_ch)
    ref = R.run(iq, np.array([R.threshold(d) for d in dbs]), np.array(alphas))
    for lane in list(range(n_ch)):
        one = dict(levels=ref["levels"][:, lane], open=ref["open"][:, lane])
        hold_state(states[lane], one, ("lane", lane))
    for lane in (0, 63, 64, 129):
        assert 0 < states[lane]["n_open"] < 4000 and states[lane]["first_open"] > 0, (lane, states[lane])


def test_attached_two_blocks_late_and_attached_again(gpu_required):
    nat = gpu_required
    n = 5 * BLK
    x = carriers(n, [(50e3, 0.1, [(0, 3 * BLK + 5000), (4 * BLK + 3000, n)])], 9)
    with nat.Frontend(FS, block_capacity=BLK, out_capacity=1 << 13) as fe:
        cid = fe.chan_open(12500, 50e3)
        early = fe.chan_open(12500, 50e3 + 100.0)
        fe.chan_squelch(early, -30.0, 0.1)
        fe.push(x[:BLK]); fe.push(x[BLK:2 * BLK])
        fe.chan_squelch(cid, -30.0, 0.1)                              # two blocks late: level 0 at sample 2000
        fe.push(x[2 * BLK:3 * BLK]); fe.push(x[3 * BLK:4 * BLK])
        late = fe.chan_squelch_state(cid)
        fe.chan_squelch(cid, -36.0, 0.05)                             # again: a new state from sample 4000 on
        fresh = fe.chan_squelch_state(cid)
        fe.push(x[4 * BLK:])
        again = fe.chan_squelch_state(cid)
        y = fe.chan_read_iq(cid)
        fe.chan_squelch(cid, None)
        with pytest.raises(nat.RcfError) as e:
            fe.chan_squelch_state(cid)
        assert e.value.code == nat.RCF_ESTATE
        fe.push(x[:BLK])                                              # the launch goes on without the detached lane
        assert fe.chan_squelch_state(early)["n_seen"] == 6000
    assert len(y) == 5000
    hold_state(late, R.run(y[2000:4000], R.threshold(-30.0), 0.1), "late", first_index=2000)
    # the carrier is there: open within two samples (0.1 x its power sits right at this threshold), closed after it has gone
    assert 2000 <= late["first_open"] <= 2001 and 0 < late["n_open"] < 2000
    assert fresh == dict(level=0.0, n_seen=0, n_open=0, first_open=-1, last_open=-1, unmuted=0)
    hold_state(again, R.run(y[4000:], R.threshold(-36.0), 0.05), "again", first_index=4000)
    assert again["first_open"] > 4000


def _two_members(nat, x0, x1, grouped, nan_at=None):
    """two front ends, two channels each with the stage; pushed as a group (one launch for the four lanes) or one by one"""
    fes, cids = [], []
    for m in range(2):
        fe = nat.Frontend(FS, device=0, block_capacity=BLK, out_capacity=1 << 13)
        cids.append([fe.chan_open(12500, 50e3), fe.chan_open(12500, -70e3)])
        for cid, (db, a) in zip(cids[m], ((-30.0, 0.1), (-33.0, 0.01))):
            fe.chan_squelch(cid, db, a)
        fes.append(fe)
    xs = [x0, x1]
    try:
        if grouped:
            with nat.Group(fes) as g:
                for b in range(3):
                    g.push([xm[b * BLK:(b + 1) * BLK] for xm in xs])
                g.sync()
        else:
            for fe, xm in zip(fes, xs):
                for b in range(3):
                    fe.push(xm[b * BLK:(b + 1) * BLK])
        return [[(fe.chan_read_iq(c), fe.chan_squelch_state(c)) for c in cs] for fe, cs in zip(fes, cids)]
    finally:
        for fe in fes:
            fe.close()


def test_a_group_of_two_front_ends(gpu_required):
    n = 3 * BLK
    on = [(7000, 20000), (30000, 41000)]
    x0 = carriers(n, [(50e3, 0.1, on), (-70e3, 0.1, on[1:])], 21)
    x1 = carriers(n, [(50e3, 0.07, on[:1]), (-70e3, 0.1, on)], 22)
    out = _two_members(gpu_required, x0, x1, grouped=True)
    for m in range(2):
        for (y, st), (db, a) in zip(out[m], ((-30.0, 0.1), (-33.0, 0.01))):
            ref = R.run(y, R.threshold(db), a)
            assert len(y) == 3000 and 0 < ref["n_open"] < 3000
            hold_state(st, ref, ("member", m, db))


def test_a_nan_burst_on_one_lane_leaves_its_neighbours_alone(gpu_required):
    """member 0's input carries a NaN burst: its lanes go NaN and muted for good; member 1's lanes, in the same launch, are
    bit-identical to their run alone"""
    n = 3 * BLK
    on = [(7000, 20000), (30000, 41000)]
    x0 = carriers(n, [(50e3, 0.1, [(0, n)]), (-70e3, 0.1, on[1:])], 21)
    x1 = carriers(n, [(50e3, 0.07, on[:1]), (-70e3, 0.1, on)], 22)
    x0[BLK + 4000:BLK + 4040] = complex(np.nan, np.nan)
    together = _two_members(gpu_required, x0, x1, grouped=True)
    alone = _two_members(gpu_required, x0, x1, grouped=False)
    for (y, st), (db, a) in zip(together[0], ((-30.0, 0.1), (-33.0, 0.01))):
        ref = R.run(y, R.threshold(db), a)
        assert np.isnan(y).any() and math.isnan(st["level"]) and st["unmuted"] == 0
        hold_state(st, ref, ("nan lane", db))
        first_nan = int(np.flatnonzero(np.isnan(y.real) | np.isnan(y.imag))[0])
        assert st["last_open"] < first_nan and st["n_seen"] == 3000
    assert together[0][0][1]["n_open"] > 0                           # it was open before the burst
    for (y, st), (y1, st1) in zip(together[1], alone[1]):
        assert np.array_equal(y, y1) and st == st1 and not math.isnan(st["level"]) and st["n_open"] > 0


def test_refusals(gpu_required):
    nat = gpu_required
    proto = G.low_pass_2(1.0, FS, 1000.0, 1250.0, 20.0, G.WIN_HAMMING)
    with nat.Frontend(FS, block_capacity=BLK, out_capacity=1 << 13) as fe:
        cid = fe.chan_open(12500, 0.0)
        for db, alpha in ((-30.0, 0.0), (-30.0, -0.1), (-30.0, 1.5), (-30.0, float("nan")), (float("nan"), 0.1), (float("inf"), 0.1)):
            with pytest.raises(nat.RcfError) as e:
                fe.chan_squelch(cid, db, alpha)
            assert e.value.code == nat.RCF_EINVAL, (db, alpha)
        fe.chan_squelch(cid, -30.0, 1.0)                              # alpha 1 is inside (0, 1]
        with pytest.raises(nat.RcfError) as e:
            fe.chan_squelch(cid + 99, -30.0, 0.1)
        assert e.value.code == nat.RCF_ENOCHAN
        with pytest.raises(nat.RcfError) as e:
            fe.chan_squelch_state(cid + 99)
        assert e.value.code == nat.RCF_ENOCHAN
        fe.pfb_open(160, 80, proto)
        tap = fe.pfb_tap_open(3, gr_phase=False)
        fe.chan_set_fm_only(tap, True)
        with pytest.raises(nat.RcfError) as e:                        # no IQ ring
            fe.chan_squelch(tap, -30.0, 0.1)
        assert e.value.code == nat.RCF_ESTATE
        with pytest.raises(nat.RcfError) as e:
            fe.chan_squelch_state(tap)
        assert e.value.code == nat.RCF_ESTATE
        fe.chan_set_fm_only(tap, False)
        fe.chan_squelch(tap, -30.0, 0.1)
        with pytest.raises(nat.RcfError) as e:                        # ... and none may be taken from under the stage
            fe.chan_set_fm_only(tap, True)
        assert e.value.code == nat.RCF_ESTATE
        fe.chan_squelch(tap, None)
        fe.chan_squelch(tap, None)                                    # off twice: nothing to do
        fe.chan_set_fm_only(tap, True)


# ------------------------------------------------------------------------------------------------ every bin of a bank
S = 256                                     # held to rcf_pfb_squelch_segment() below
LEAD = 40                                   # frames before the detector is switched on
FRAMES = [1, 0, S - 1, S, S + 1, 5 * S + 3, 0, S + 7, 1]
OUT_CAP = 2048                              # < LEAD + sum(FRAMES) = 2356: the bins ring wraps
BANKS = {64: 0.8e6, 160: 2e6, 400: 5e6}     # bins -> fs at the reference's channel rule (D = bins / 2): families 1 (tiled), 3, 2
ALPHA = 0.1


def bank_plan(nb):
    """{bin: (threshold dB, [(on, off) in frames since rcf_pfb_open])}: thresholds that differ from bin to bin; twelve bins
    keyed on one frame apart around the first segment edge of the long block (some bin opens on a segment's last frame, some
    on the next one's first) and off again inside it; one keyed inside the short blocks; one in mid-segment; one on
    throughout; one whose carrier never rises.  Carriers stand three bins apart and reach into the negative frequencies."""
    step = 3 if nb == 64 else 5
    bins = [(2 + step * j) % nb for j in range(17)]
    assert len(set(bins)) == 17
    thr = lambda k: -40.0 - 3.0 * (k % 7)
    total = LEAD + sum(FRAMES)
    long0 = LEAD + sum(FRAMES[:5])                                    # first frame of the 5S + 3 block
    plan = {}
    for j in range(12):
        plan[bins[j]] = (thr(bins[j]), [(long0 + S - 7 + j, long0 + S + 90 + 3 * j)])
    plan[bins[12]] = (thr(bins[12]), [(LEAD + 300, LEAD + 420)])
    plan[bins[13]] = (thr(bins[13]), [(long0 + 131, long0 + 3 * S + 40)])
    plan[bins[14]] = (thr(bins[14]), [(0, total)])
    plan[bins[15]] = (thr(bins[15]), [])
    plan[bins[16]] = (thr(bins[16]), [(long0 + 5 * S - 2, total)])    # into the long block's last, short segment
    thr_db = np.array([thr(k) for k in range(nb)])
    return plan, thr_db


class Feeder:
    """pushes x so that every block holds a given number of frames (a block of 0 frames still pushes samples).  The bank was
    opened at sample 0: N samples in are floor((N - 1) / D) + 1 frames"""

    def __init__(self, fe, x, D):
        self.fe, self.x, self.D, self.at, self.calls = fe, x, D, 0, 0

    def push_frames(self, f):
        done = self.fe.pfb_produced() + f
        self.calls += 1
        assert done > 0 and 2 * self.calls < self.D
        upto = (done - 1) * self.D + 1 + 2 * self.calls
        assert upto > self.at
        self.fe.push(self.x[self.at:upto])
        self.at = upto
        assert self.fe.pfb_produced() == done, (f, done)


def census(is_open, starts):
    """how the bins opened and closed against the blocks' segments.  is_open [frames, bins] from the detector's first frame
    on; starts: the first frame of every block with frames, and the end"""
    seen = dict(mid_segment=0, segment_first=0, segment_last=0, closes_mid_block=0,
                throughout=int(is_open.all(axis=0).sum()), never=int((~is_open).all(axis=0).sum()))
    up = np.argwhere(is_open[1:] & ~is_open[:-1])
    down = np.argwhere(~is_open[1:] & is_open[:-1])
    for f, _ in up + [1, 0]:
        b = np.searchsorted(starts, f, side="right") - 1
        rel, length = f - starts[b], starts[b + 1] - starts[b]
        last = rel % S == S - 1 or rel == length - 1
        first = rel % S == 0
        seen["segment_first"] += first
        seen["segment_last"] += last
        seen["mid_segment"] += not first and not last
    for f, _ in down + [1, 0]:
        b = np.searchsorted(starts, f, side="right") - 1
        seen["closes_mid_block"] += f - starts[b] > 0
    return seen


@pytest.mark.parametrize("nb", sorted(BANKS))
def test_every_bin_of_a_bank_level_within_the_bound_counters_equal(gpu_required, nb):
    nat = gpu_required
    assert nat.pfb_squelch_segment() == S
    fs = BANKS[nb]
    D, proto = G.channel_params(fs, 12500)
    assert D == nb // 2 and nat.lib().rcf_pfb_shape_family(nb, D, len(proto)) == {64: 1, 160: 3, 400: 2}[nb]
    plan, thr_db = bank_plan(nb)
    total = LEAD + sum(FRAMES)
    x = R.designed_keying(np.random.default_rng(4000 + nb), fs, nb, D, total + 1, plan, float(np.sum(proto, dtype=np.float64)))
    states, bins = [], [[] for _ in range(nb)]
    with nat.Frontend(fs, block_capacity=(5 * S + 8) * D, hist_capacity=max(1 << 14, len(proto) + 2 * nb), out_capacity=OUT_CAP) as fe:
        fe.pfb_open(nb, D, proto)
        feed = Feeder(fe, x, D)
        feed.push_frames(LEAD)
        fe.pfb_squelch(thr_db, ALPHA)
        for k in range(nb):
            bins[k].append(fe.pfb_read_bin(k, 4096))
        for f in FRAMES:                                              # (the ring holds less than the run: read as it goes)
            feed.push_frames(f)
            states.append(fe.pfb_squelch_read(nb))
            for k in range(nb):
                bins[k].append(fe.pfb_read_bin(k, 4096))
    y = np.stack([np.concatenate(b) for b in bins], axis=1)
    assert y.shape == (total, nb) and total > OUT_CAP
    thr = np.array([R.threshold(d) for d in thr_db])
    ref = R.run(y[LEAD:], thr, ALPHA, first_index=LEAD)
    # a condition on the input, not a measurement: no level of any bin at any frame within rounding of its threshold
    margin = R.margin(ref["levels"], thr)
    assert margin >= 1e-6, margin
    ends = np.cumsum(FRAMES)
    starts = np.unique(np.concatenate([[0], ends]))
    seen = census(ref["open"], starts)
    assert min(seen.values()) > 0 and len(set(thr_db)) > 1, seen
    worst = 0.0
    for st, end in zip(states, ends):
        o = ref["open"][:end]
        assert st["frames_seen"] == end
        lev = ref["levels"][end - 1]
        worst = max(worst, float(np.max(np.abs(st["level"] - lev) / lev)))
        assert np.array_equal(st["n_open"], o.sum(axis=0)), end
        idx = np.arange(LEAD, LEAD + end)[:, None]
        assert np.array_equal(st["last_open"], np.where(o, idx, -1).max(axis=0)), end
        assert np.array_equal(st["unmuted"], o[-1]), end
        assert not (st["mask"][-1] >> np.uint32(nb % 32)) or nb % 32 == 0            # no bit beyond the last bin
    print("%d bins: largest relative distance of a level %.3g (bound %.3g), margin %.3g, census %s" % (nb, worst, R.bound(ALPHA), margin, seen))
    assert worst <= R.bound(ALPHA)


def test_bank_refusals_and_the_fused_discriminator(gpu_required):
    nat = gpu_required
    fs, nb = 5e6, 400
    D, proto = G.channel_params(fs, 12500)
    x = R.designed_keying(np.random.default_rng(77), fs, nb, D, 130, {9: (-40.0, [(10, 130)])}, float(np.sum(proto, dtype=np.float64)))
    with nat.Frontend(fs, block_capacity=40 * D, out_capacity=OUT_CAP) as fe:
        for call in (lambda: fe.pfb_squelch(-40.0, 0.1), lambda: fe.pfb_squelch_read(nb)):
            with pytest.raises(nat.RcfError) as e:                    # no bank
                call()
            assert e.value.code == nat.RCF_ESTATE
        fe.pfb_open(nb, D, proto)
        with pytest.raises(nat.RcfError) as e:                        # never on
            fe.pfb_squelch_read(nb)
        assert e.value.code == nat.RCF_ESTATE
        for thr, alpha in (([-40.0] * 3, 0.1), (-40.0, 0.0), (-40.0, 1.01), (float("nan"), 0.1), ([-40.0] * (nb - 1) + [float("inf")], 0.1)):
            with pytest.raises(nat.RcfError) as e:
                fe.pfb_squelch(thr, alpha)
            assert e.value.code == nat.RCF_EINVAL, (thr, alpha)
        fe.pfb_squelch(-40.0, 0.1)
        with pytest.raises(nat.RcfError) as e:
            fe.pfb_squelch_read(nb - 1)
        assert e.value.code == nat.RCF_EINVAL
        feed = Feeder(fe, x, D)
        feed.push_frames(30)
        fe.pfb_fm_enable(1)                                           # beside the bins ring: fine
        feed.push_frames(30)
        st = fe.pfb_squelch_read(nb)
        y = fe.pfb_read_bin(9, 4096)
        ref = R.run(y, R.threshold(-40.0), 0.1)
        assert st["frames_seen"] == 60 and st["n_open"][9] == ref["n_open"] > 0 and st["unmuted"][9]
        assert abs(st["level"][9] - ref["level"]) <= R.bound(0.1) * ref["level"]
        with pytest.raises(nat.RcfError) as e:                        # instead of it: refused while the detector is on
            fe.pfb_fm_enable(2)
        assert e.value.code == nat.RCF_ESTATE
        fe.pfb_squelch(None)
        fe.pfb_fm_enable(2)
        with pytest.raises(nat.RcfError) as e:                        # ... and the detector while there are no bins to read
            fe.pfb_squelch(-40.0, 0.1)
        assert e.value.code == nat.RCF_ESTATE
        feed.push_frames(5)
        off = fe.pfb_squelch_read(nb)                                 # off: the last state, the count stands
        assert off["frames_seen"] == 60 and np.array_equal(off["n_open"], st["n_open"]) and np.array_equal(off["level"], st["level"])


def test_bank_off_and_on_again_resets(gpu_required):
    nat = gpu_required
    fs, nb = 0.8e6, 64
    D, proto = G.channel_params(fs, 12500)
    x = R.designed_keying(np.random.default_rng(78), fs, nb, D, 400, {5: (-40.0, [(0, 400)])}, float(np.sum(proto, dtype=np.float64)))
    with nat.Frontend(fs, block_capacity=300 * D, out_capacity=OUT_CAP) as fe:
        fe.pfb_open(nb, D, proto)
        fe.pfb_squelch(-40.0, 0.1)
        feed = Feeder(fe, x, D)
        feed.push_frames(100)
        a = fe.pfb_squelch_read(nb)
        fe.pfb_squelch(None)
        feed.push_frames(20)
        fe.pfb_squelch([-40.0] * nb, 0.5)
        z = fe.pfb_squelch_read(nb)
        feed.push_frames(S + 3)
        b = fe.pfb_squelch_read(nb)
        y = fe.pfb_read_bin(5, 4096)
    assert a["frames_seen"] == 100 and a["n_open"][5] > 90
    assert z["frames_seen"] == 0 and not z["n_open"].any() and not z["level"].any() and (z["last_open"] == -1).all() and not z["mask"].any()
    ref = R.run(y[120:], R.threshold(-40.0), 0.5, first_index=120)
    assert b["frames_seen"] == S + 3 == b["n_open"][5] == ref["n_open"] and b["last_open"][5] == 120 + S + 2
    assert abs(b["level"][5] - ref["level"]) <= R.bound(0.5) * ref["level"]


def test_a_group_of_two_unequal_banks(gpu_required):
    """a 64-bin tiled bank and a 160-bin frame-major one, blocks of different frame counts, one group"""
    nat = gpu_required
    members = []
    for nb, frames in ((64, [S + 5, 3, 2 * S]), (160, [40, S, S + 1])):
        fs = BANKS[nb]
        D, proto = G.channel_params(fs, 12500)
        n_frames = sum(frames) + 1
        plan = {7: (-40.0, [(20, n_frames)]), nb - 9: (-46.0, [(S - 1, S + 60)])}
        x = R.designed_keying(np.random.default_rng(90 + nb), fs, nb, D, n_frames, plan, float(np.sum(proto, dtype=np.float64)))
        fe = nat.Frontend(fs, device=0, block_capacity=(2 * S + 8) * D, hist_capacity=1 << 14, out_capacity=OUT_CAP)
        fe.pfb_open(nb, D, proto)
        thr_db = np.full(nb, -40.0)
        thr_db[nb - 9] = -46.0
        fe.pfb_squelch(thr_db, ALPHA)
        members.append(dict(fe=fe, nb=nb, D=D, x=x, frames=frames, thr_db=thr_db))
    try:
        with nat.Group([m["fe"] for m in members]) as g:
            at = [0, 0]
            for j in range(3):
                blocks = []
                for i, m in enumerate(members):
                    done = sum(m["frames"][:j + 1])
                    upto = (done - 1) * m["D"] + 1 + j
                    blocks.append(m["x"][at[i]:upto])
                    at[i] = upto
                g.push(blocks)
            g.sync()
        for m in members:
            fe, nb = m["fe"], m["nb"]
            st = fe.pfb_squelch_read(nb)
            total = sum(m["frames"])
            assert st["frames_seen"] == total == fe.pfb_produced()
            y = np.stack([fe.pfb_read_bin(k, 4096) for k in range(nb)], axis=1)
            thr = np.array([R.threshold(d) for d in m["thr_db"]])
            ref = R.run(y, thr, ALPHA)
            assert R.margin(ref["levels"], thr) >= 1e-6
            assert ref["n_open"][7] > 0 and ref["n_open"][nb - 9] > 0
            assert np.array_equal(st["n_open"], ref["n_open"]) and np.array_equal(st["last_open"], ref["last_open"])
            assert np.array_equal(st["unmuted"], ref["unmuted"])
            assert float(np.max(np.abs(st["level"] - ref["level"]) / ref["level"])) <= R.bound(ALPHA)
    finally:
        for m in members:
            m["fe"].close()
