"""-m gpu: the analog NBFM voice chain with MANY chains per launch -- its production case, and the
shape its kernels are written for: audio_gate_kernel / audio_deemph_kernel give a wave 64 chains, one lane each, the four
index-parallel kernels run on a grid (blocks of the longest item, items).

Reference: oracle/audio.py's stages on the channel's OWN IQ (chan_read_iq) from the chain's attachment on.  The channelizer
is held to the oracle elsewhere; feeding the device's IQ isolates the audio kernels and makes the gate exactly reproducible
(float |x|^2, then a double one-pole filter in a fixed order: pwr_squelch_cc restates it operation for operation), so the
number of samples that pass the gate is EQUAL, not close.  Audio: rms error < 1e-4 (BASELINE.json north star), and bit for
bit the chain run alone on the same front-end with the same channels open.

Lanes: the planner emits a block's voice chains by (decimation, taps) class in ascending order and by channel id inside a
class (rcf_plan.cpp: plan cache), so the lane of a chain is its rank in that order; `_lane_order` restates it."""
import numpy as np
import pytest

from oracle import audio as A
from oracle import grspec as G
from rcf import audio as host_audio
from rcf import synth

pytestmark = pytest.mark.gpu

FS = 2.4e6
BLK = 48000
AMP = 0.1                     # featured carriers: -20 dB in their channel
NOISE = 0.01                  # wideband noise: about -58 dB in the widest channel (37.5 kHz of 2.4 MHz at 1e-4)
OPEN_DB = -100.0              # the reference's own threshold: the noise keeps it open
GATED_DB = -40.0              # 20 dB under a carrier, 18 dB over the noise: closes ~460 samples into a gap (0.99^n = 0.01)
NEVER_DB = 0.0                # the whole wideband input carries < 0.1 of power: no channel ever reads 1.0
BAR = 1e-4


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))) if len(a) else 0.0


def analog(db):
    return dict(kind="analog", db=db)


DSD = dict(kind="dsd", gain=0.4)


def _attach(fe, cid, rate, spec):
    """rate: the channel's sample rate (twice chan_open's channel_rate)"""
    if spec["kind"] == "dsd":
        fe.chan_audio_open(cid, **host_audio.dsd_feed_params(rate, spec["gain"]))
    else:
        fe.chan_audio_open(cid, **host_audio.analog_chain_params(rate, squelch_db=spec["db"]))


def _reference(iq, rate, spec):
    """-> (samples that pass the gate, output stream) of the chain on `iq`, a flowgraph started at iq[0]"""
    if spec["kind"] == "dsd":
        fm = G.quadrature_demod_cf(iq, np.float32(spec["gain"]))
        return len(iq), A.rational_resampler_fff(fm, 48000, int(rate))
    st = A.analog_chain(iq, float(rate), stages=True, squelch_db=spec["db"], squelch_alpha=0.01)
    return len(st["gated"]), st["audio"]


def _check(what, audio, counts, iq, rate, spec):
    """counts and length exactly, values within the bar -> (rms error, samples the reference's gate passed)"""
    n_ref, ref = _reference(iq, rate, spec)
    n_audio, n_ungated = counts
    assert n_ungated == n_ref, (what, n_ungated, n_ref, len(iq),
                                A.pwr_squelch_margin(iq, spec["db"], 0.01) if spec["kind"] == "analog" else None)
    assert len(audio) == n_audio == len(ref), (what, len(audio), n_audio, len(ref))
    e = rms(audio, ref)
    print("%s: %d of %d pass the gate, %d out, rms error %.3e" % (what, n_ref, len(iq), len(ref), e))
    assert e < BAR, (what, e)
    return e, n_ref


def _signal(n, carriers, seed):
    """wideband noise + NBFM carriers dict(off, tone, dev, gaps=[(a, b), ...]): keyed off over input samples [a, b)"""
    rng = np.random.default_rng(seed)
    x = NOISE * synth.awgn(rng, n).astype(np.complex128)
    for j, c in enumerate(carriers):
        s = synth.nbfm_carrier(n, FS, c["off"], c["tone"], c["dev"], AMP, phase0=0.7 * j)
        for a, b in c["gaps"]:
            s[a:b] = 0
        x += s
    return x.astype(np.complex64)


def _lane_order(fe, cids):
    """indices into cids in the order the planner emits their chains: class (D, T) ascending, channel id inside a class"""
    info = [fe.chan_info(c) for c in cids]
    return sorted(range(len(cids)), key=lambda i: (info[i]["decim"], info[i]["ntaps"], cids[i]))


def _push_blocks(fe, x, blk=BLK):
    for a in range(0, len(x), blk):
        fe.push(x[a:a + blk])


# ---------------------------------------------------------------------------------------------------------------- 1
N1, K1 = 67, 12
CR1 = (6250, 12500, 25000)                    # channel i: CR1[i % 3] -> D = 192, 96, 48: 250, 500, 1000 samples a block
FEATURED1 = (0, 1, 2, 3, 4, 5, 65, 66)


def _plan1():
    """-> (offsets, specs, carriers) of test 1.  Channel slots lie 30 kHz apart; the featured channels take every
    eighth slot (240 kHz apart), whatever their place in the channel list."""
    slots = [-1.0e6 + 30e3 * k for k in range(N1)]
    f_slots = [slots[8 * j] for j in range(len(FEATURED1))]
    rest = [s for s in slots if s not in f_slots]
    offs, specs, carriers = [], [], []
    for i in range(N1):
        if i in FEATURED1:
            j = FEATURED1.index(i)
            offs.append(f_slots[j])
            specs.append(analog(GATED_DB))
            # gaps of four blocks (1000 / 2000 / 4000 channel samples), staggered by 7013 inputs: the gates close
            # and open in different 64-sample chunks, at different places in them; carrier 5 starts late instead
            g0 = 2 * BLK + 7013 * j
            gaps = [(0, 150001)] if i == 5 else [(g0, g0 + 4 * BLK)]
            carriers.append(dict(off=f_slots[j], tone=300.0 + 150.0 * j, dev=800.0 + 150.0 * j, gaps=gaps))
            continue
        offs.append(rest.pop(0))
        q = (i // 3) % 4
        if i == 63:
            specs.append(DSD)                                   # at 12.5 kS/s: 96/25, the largest ratio on the smallest n_k
        elif q == 0 or i == 57:                                 # (57: lane 63, the first wave's last, carries a live chain)
            specs.append(analog(OPEN_DB))
        elif q == 1:
            specs.append(analog(NEVER_DB))
        elif q == 2:
            specs.append(DSD if i % 3 == 1 else analog(OPEN_DB))   # at 25 kS/s: 48/25
        else:
            specs.append(analog(OPEN_DB) if i % 3 == 1 else analog(NEVER_DB))
    return offs, specs, carriers


def test_67_chains_three_rates_one_launch_per_block(gpu_required):
    """64 items in the first workgroup, 3 in the second; n_k = 1000, 500 and 250 in one wave (lanes leave the chunk loop
    at trips 16, 8 and 4), three sets of filters, ratios 4/25, 8/25, 16/25, 48/25 and 96/25; gates that close and open
    beside lanes that keep everything and lanes that keep nothing.
    Measured on an MI355X: worst rms error 1.3e-6 (bar 1e-4)."""
    nat = gpu_required
    offs, specs, carriers = _plan1()
    feat = sorted(c["off"] for c in carriers)
    assert min(b - a for a, b in zip(feat[:-1], feat[1:])) >= 50e3
    assert sum(s is DSD for s in specs) >= 5
    x = _signal(BLK * K1, carriers, 67)
    rate = [2 * CR1[i % 3] for i in range(N1)]

    def run(only=None):
        """every channel open; every chain attached, or channel `only`'s alone -> {i: (counts, audio, iq)}, lane order"""
        with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
            cids = [fe.chan_open(CR1[i % 3], offs[i]) for i in range(N1)]
            who = range(N1) if only is None else [only]
            for i in who:
                _attach(fe, cids[i], rate[i], specs[i])
            fe.timing_enable(True, classes=[nat.T_AUDIO])
            _push_blocks(fe, x)
            assert fe.timing_read(nat.T_AUDIO)[1] == K1                # one launch carries all chains
            return ({i: (fe.chan_audio_produced(cids[i]), fe.chan_read_audio(cids[i]), fe.chan_read_iq(cids[i])) for i in who},
                    _lane_order(fe, cids))

    got, order = run()
    assert order[0] == 2 and order[-1] == 66 and [rate[i] for i in (order[21], order[22], order[43], order[44])] == [50000, 25000, 25000, 12500]
    worst, gated = 0.0, {}
    for lane, i in enumerate(order):
        counts, audio, iq = got[i]
        assert len(iq) == K1 * BLK * CR1[i % 3] * 2 // int(FS)
        e, gated[i] = _check("lane %d (channel %d, %d S/s, %s)" % (lane, i, rate[i], specs[i]), audio, counts, iq, rate[i], specs[i])
        worst = max(worst, e)
    print("67 chains: worst rms error %.3e" % worst)
    # the shape did not degenerate: the featured gates closed for a good part of their gap (and not for ever), the
    # never-open ones passed nothing, everything else passed (nearly) everything
    for i in range(N1):
        n = len(got[i][2])
        if i in FEATURED1:
            assert n // 8 < gated[i] < n - n // 8, (i, gated[i], n)
        elif specs[i] == analog(NEVER_DB):
            assert gated[i] == 0 and len(got[i][1]) == 0, i
        else:
            assert gated[i] >= n - 8, (i, gated[i], n)
    # bit for bit the chain run alone: lane 0, lane 63, the second workgroup's first lane, the last item, one featured
    # lane of each channel rate, two DSD feeds (48/25 and 96/25)
    alone = {order[0], order[63], order[64], order[66], 2, 4, 66, 7, 63}
    assert {rate[i] for i in alone} == {12500, 25000, 50000} and specs[7] is DSD and specs[63] is DSD
    for i in sorted(alone):
        counts, audio, iq = run(only=i)[0][i]
        assert iq.tobytes() == got[i][2].tobytes(), i
        assert counts == got[i][0], (i, counts, got[i][0])
        assert audio.tobytes() == got[i][1].tobytes(), ("lane %d (channel %d) differs from the chain run alone" % (order.index(i), i))
    print("bit for bit alone: lanes %s" % sorted(order.index(i) for i in alone))


# ---------------------------------------------------------------------------------------------------------------- 2
def test_lanes_move_state_does_not(gpu_required):
    """chains attached at three block boundaries, two closed mid-stream (one of them the first item: every later chain
    changes lane), one of those reopened (zero state from that sample on), a whole channel closed under its chain:
    every chain's audio is the reference started at its own attachment sample
    Measured on an MI355X: worst rms error 4.3e-7 (bar 1e-4)."""
    nat = gpu_required
    n_ch, K = 10, 12
    offs = [-900e3 + 200e3 * i for i in range(n_ch)]
    specs = [analog(GATED_DB) if i % 2 == 0 else (DSD if i == 7 else analog(OPEN_DB)) for i in range(n_ch)]
    carriers = [dict(off=offs[i], tone=350.0 + 100.0 * i, dev=900.0 + 100.0 * i,
                     gaps=[(BLK * 3 + 9001 * i, BLK * 6 + 9001 * i)]) for i in range(0, n_ch, 2)]
    x = _signal(BLK * K, carriers, 10)
    rate = [2 * CR1[i % 3] for i in range(n_ch)]
    done = []                                                            # (what, i, audio, counts, k0, k1)

    def code(fn, *a):
        with pytest.raises(nat.RcfError) as e:
            fn(*a)
        return e.value.code

    with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
        cids = [fe.chan_open(CR1[i % 3], offs[i]) for i in range(n_ch)]
        order = _lane_order(fe, cids)
        first = order[0]
        assert first == 2
        k0 = {}

        def attach(i):
            k0[i] = fe.chan_produced(cids[i])
            _attach(fe, cids[i], rate[i], specs[i])

        def retire(i, what, close):
            done.append((what, i, fe.chan_read_audio(cids[i]), fe.chan_audio_produced(cids[i]), k0.pop(i), fe.chan_produced(cids[i])))
            close(cids[i])

        iq1 = None
        fe.timing_enable(True, classes=[nat.T_AUDIO])
        for b in range(K):
            if b == 0:
                for i in range(6):
                    attach(i)
            if b == 3:
                attach(6)
                attach(7)
            if b == 5:
                retire(first, "closed (the first item)", fe.chan_audio_close)
                retire(4, "closed", fe.chan_audio_close)
                assert code(fe.chan_read_audio, cids[4]) == nat.RCF_ESTATE
                assert code(fe.chan_audio_produced, cids[first]) == nat.RCF_ESTATE
            if b == 7:
                for i in (8, 9, first):
                    attach(i)
                assert fe.chan_audio_produced(cids[first]) == (0, 0)
            if b == 9:
                iq1 = fe.chan_read_iq(cids[1])
                retire(1, "its channel closed", fe.chan_close)
                assert code(fe.chan_read_audio, cids[1]) == nat.RCF_ENOCHAN
            fe.push(x[b * BLK:(b + 1) * BLK])
        assert fe.timing_read(nat.T_AUDIO)[1] == K
        iqs = {i: fe.chan_read_iq(cids[i]) for i in range(n_ch) if i != 1}
        iqs[1] = iq1
        for i in sorted(k0):
            done.append(("open to the end", i, fe.chan_read_audio(cids[i]), fe.chan_audio_produced(cids[i]), k0[i], len(iqs[i])))
        assert code(fe.chan_read_audio, cids[4]) == nat.RCF_ESTATE
    assert len(done) == 11 and {d[4] > 0 for d in done} == {False, True}
    worst = 0.0
    for what, i, audio, counts, a, b in done:
        assert 0 <= a < b <= len(iqs[i])
        e, _ = _check("channel %d, %s, samples [%d, %d)" % (i, what, a, b), audio, counts, iqs[i][a:b], rate[i], specs[i])
        worst = max(worst, e)
    print("lanes move: worst rms error %.3e" % worst)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_small_rings_ragged_pushes_incremental_reads_six_chains(gpu_required):
    """out_capacity 4096, six chains at 25 and 12.5 kS/s, IQ and audio read after every push: every ring of every lane
    wraps (three times at 25 kS/s, more than once at 12.5 kS/s; the compacted rings behind the gates at their own samples)
    and the concatenations are the reference
    Measured on an MI355X: worst rms error 3.1e-7 (bar 1e-4)."""
    nat = gpu_required
    cap, step, n_push = 4096, 96 * 1500 + 31, 9                          # 1500 (750) channel samples a push
    crs = [12500, 6250, 12500, 6250, 12500, 6250]
    offs = [-500e3 + 200e3 * i for i in range(6)]
    specs = [analog(GATED_DB), analog(GATED_DB), DSD, analog(OPEN_DB), analog(OPEN_DB), analog(GATED_DB)]
    carriers = [dict(off=offs[i], tone=400.0 + 90.0 * i, dev=1000.0, gaps=[(step * (1 + i % 3) + 5000 * i, step * (3 + i % 3) + 5000 * i),
                                                                            (step * 6 + 3000 * i, step * 7)]) for i in (0, 1, 5)]
    x = _signal(step * n_push, carriers, 3)
    rate = [2 * c for c in crs]
    reach = len(host_audio.analog_chain_params(25000)["hpf_taps"])       # the longest filter of the fastest chain
    assert 1501 + reach <= cap < 2100 + reach
    got_a, got_iq = [[] for _ in crs], [[] for _ in crs]
    with nat.Frontend(FS, device=0, block_capacity=96 * 2200, out_capacity=cap) as fe:
        cids = [fe.chan_open(crs[i], offs[i]) for i in range(6)]
        for i in range(6):
            _attach(fe, cids[i], rate[i], specs[i])
        # a block whose channel samples + the chain's reach pass the ring: refused, nothing queued
        with pytest.raises(nat.RcfError) as e:
            fe.push(x[:96 * 2100])
        assert e.value.code == nat.RCF_ECAP
        assert all(fe.chan_produced(c) == 0 for c in cids)
        for at in range(0, len(x), step):
            fe.push(x[at:at + step])
            for i, c in enumerate(cids):
                got_iq[i].append(fe.chan_read_iq(c))
                got_a[i].append(fe.chan_read_audio(c))
        counts = [fe.chan_audio_produced(c) for c in cids]
    worst = 0.0
    for i in range(6):
        iq, audio = np.concatenate(got_iq[i]), np.concatenate(got_a[i])
        assert len(iq) > (3 if crs[i] == 12500 else 1.5) * cap
        e, n_pass = _check("small rings, channel %d (%d S/s, %s)" % (i, rate[i], specs[i]), audio, counts[i], iq, rate[i], specs[i])
        if i in (0, 1, 5):
            assert len(iq) // 8 < n_pass < len(iq) - len(iq) // 8           # the gate did close, and open again
        worst = max(worst, e)
    print("small rings: worst rms error %.3e" % worst)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_two_front_ends_in_a_group_three_chains_each(gpu_required):
    """launch_member_audio for both members of a Group: each chain bit for bit the same front-end pushed alone, and the
    reference within the bar
    Measured on an MI355X: worst rms error 4.2e-7 (bar 1e-4)."""
    nat = gpu_required
    K = 8
    crs = [(12500, 12500, 6250), (25000, 6250, 25000)]
    offs = [(-300e3, 100e3, 500e3), (-700e3, -100e3, 300e3)]
    specs = [(analog(GATED_DB), DSD, analog(OPEN_DB)), (analog(OPEN_DB), analog(GATED_DB), analog(NEVER_DB))]
    xs = [_signal(BLK * K, [dict(off=offs[0][0], tone=500.0, dev=1500.0, gaps=[(BLK * 2 + 777, BLK * 5)])], 40),
          _signal(BLK * K, [dict(off=offs[1][1], tone=700.0, dev=1000.0, gaps=[(BLK * 1 + 4321, BLK * 5 + 99)])], 41)]

    def open_member(m):
        fe = nat.Frontend(FS, device=0, block_capacity=BLK)
        cids = [fe.chan_open(crs[m][j], offs[m][j]) for j in range(3)]
        for j, c in enumerate(cids):
            _attach(fe, c, 2 * crs[m][j], specs[m][j])
        return fe, cids

    def read_all(fe, cids):
        return [(fe.chan_audio_produced(c), fe.chan_read_audio(c), fe.chan_read_iq(c)) for c in cids]

    members = [open_member(m) for m in range(2)]
    fes = [fe for fe, _ in members]
    try:
        fes[0].timing_enable(True, classes=[nat.T_AUDIO])
        fes[1].timing_enable(True, classes=[nat.T_AUDIO])
        with nat.Group(fes) as g:
            for b in range(K):
                g.push([xm[b * BLK:(b + 1) * BLK] for xm in xs])
            g.sync()
            assert [fe.timing_read(nat.T_AUDIO)[1] for fe in fes] == [K, K]      # one launch per member per group block
            grouped = [read_all(fe, cids) for fe, cids in members]
    finally:
        for fe in fes:
            fe.close()
    worst = 0.0
    for m in range(2):
        fe, cids = open_member(m)
        try:
            _push_blocks(fe, xs[m])
            alone = read_all(fe, cids)
        finally:
            fe.close()
        for j in range(3):
            (counts, audio, iq), (c1, a1, iq1) = grouped[m][j], alone[j]
            assert iq.tobytes() == iq1.tobytes(), (m, j)
            assert counts == c1, (m, j, counts, c1)
            assert audio.tobytes() == a1.tobytes(), (m, j)
            e, _ = _check("group member %d chain %d (%d S/s, %s)" % (m, j, 2 * crs[m][j], specs[m][j]), audio, counts, iq,
                          2 * crs[m][j], specs[m][j])
            worst = max(worst, e)
    print("group: worst rms error %.3e" % worst)
