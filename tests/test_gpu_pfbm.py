"""The mixed-radix filterbank family (radiocapture-rf_amd/csrc/pfbm.hip): 160, 192, 480, 640, 960 and 1280 bins at
D = NB / 2 -- the reference's 2, 2.4, 6, 8, 12 and 16 Msps sources on the 12.5 kHz raster, with the reference's own channel
filter as the prototype.  Every comparison goes through the C ABI: every bin of every shape against the exact-phase
oracle, cut invariance to the bit, taps, the grouped launch of ten 2.4 Msps sources, and the receiver end to end at
2.4 Msps against the GR-faithful oracle."""
import json
import math
import types

import numpy as np
import pytest

from oracle import cbind as OC
from oracle import grspec as G
from rcf import synth

from test_gpu_round3 import _dump          # the per-bin table goes where the 1600-bin one goes

pytestmark = pytest.mark.gpu

# fs -> bins (rc_frontend/channel.py:31-33: D = int(fs / 12500) / 2 = bins / 2, T = odd(int(fs / 6875)))
SHAPES = [(2.0e6, 160), (2.4e6, 192), (6e6, 480), (8e6, 640), (12e6, 960), (16e6, 1280)]
# frames per chunk of each shape's kernel (PfbShape::chunk_frames): the ragged cuts below are sized against it
CHUNK = {160: 16, 192: 16, 480: 8, 640: 8, 960: 4, 1280: 4}


def rel_rms(a, b):
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2) / np.mean(np.abs(b) ** 2)))


def rms(a, b):
    return float(np.sqrt(np.mean(np.abs(np.asarray(a, dtype=np.float64) - b) ** 2)))


def _stream(fs, nb):
    """unit noise + a few tones (one on a bin centre, one off it, one near -fs/2), a lead-in before the bank is opened that
    is no multiple of D, 150 frames and a ragged tail.
    The tones stand 20 dB over a bin's noise (amplitude 10 sqrt(sum h^2)), not more: the bar is a RELATIVE error per bin,
    and a float32 transform's rounding -- butterflies and binary-powered twiddles, a few 1e-7 -- is relative to the strongest
    bin that shares a butterfly with the one looked at, so a bin of bare noise beside a tone d times its amplitude reads a
    few 1e-7 x d.  d = 10 leaves the 1e-5 bar a factor of three or more."""
    D, proto = G.channel_params(fs, 12500)
    assert D == nb // 2
    rng = np.random.default_rng(7000 + nb)
    lead = D + int(rng.integers(1, D))
    n = lead + D * 150 + int(rng.integers(1, D))
    x = synth.awgn(rng, n).astype(np.complex128)
    t = np.arange(n) / fs
    floor = float(np.sqrt(np.sum(proto.astype(np.float64) ** 2)))
    for f, a in ((7 * fs / nb, 10.0), (-20.37 * fs / nb, 10.0), (-(nb // 2 - 1) * fs / nb, 10.0)):
        x += a * floor * np.exp(2j * np.pi * f * t)
    return D, proto, lead, x.astype(np.complex64)


_runs = {}


def _run(nat, fs, nb, ragged):
    """all bins of one shape, the stream in one push or in ragged pieces; computed once per (shape, cutting)"""
    key = (nb, ragged)
    if key in _runs:
        return _runs[key]
    D, proto, lead, x = _stream(fs, nb)
    n = len(x)
    if ragged:
        # pieces shorter than D (no frame at all), shorter than one chunk, a few chunks and a bit, the rest
        F = CHUNK[nb]
        sizes = [D // 3, D - 1, 1, 2 * D + 5, F * D - 7, 3, 3 * F * D + D // 2, D // 2, 5 * D]
        cuts = [lead]
        for s in sizes:
            cuts.append(cuts[-1] + s)
        assert cuts[-1] < n
        cuts.append(n)
    else:
        cuts = [lead, n]
    with nat.Frontend(fs, block_capacity=n + 16, hist_capacity=max(1 << 14, len(proto) + 2 * nb), out_capacity=1 << 10) as fe:
        fe.push(x[:lead])
        fe.pfb_open(nb, D, proto)
        for a, b in zip(cuts[:-1], cuts[1:]):
            fe.push(x[a:b])
        produced = fe.pfb_produced()
        bins = np.stack([fe.pfb_read_bin(k) for k in range(nb)])
    _runs[key] = (produced, bins)
    return _runs[key]


def _exact_all_bins(x, D, proto, nb, fs):
    """G.xlating_fir_exact for all nb on-grid offsets at once: the same composite taps h[i] e^{j w0 i}, the same products and
    the same output rotation, with the gather of the input done once instead of once per bin (1280 calls would take a
    quarter of a minute).  Held to G.xlating_fir_exact itself on a handful of bins by the caller."""
    T = len(proto)
    n_out = (len(x) - 1) // D + 1
    xp = np.concatenate([np.zeros(T - 1, dtype=np.complex128), x.astype(np.complex128)])
    idx = (np.arange(n_out) * D)[:, None] + np.arange(T)[None, :]
    X = xp[idx]                                               # [n_out, T]
    ks = np.array([k if k <= nb // 2 else k - nb for k in range(nb)], dtype=np.float64)
    w0 = 2.0 * math.pi * (ks * fs / nb) / fs
    i = np.arange(T, dtype=np.float64)
    out = np.empty((nb, n_out), dtype=np.complex128)
    for k0 in range(0, nb, 160):
        ct = proto.astype(np.float64)[None, :] * np.exp(1j * w0[k0:k0 + 160, None] * i[None, :])
        out[k0:k0 + 160] = (X @ ct[:, ::-1].T).T
    return out * np.exp(-1j * w0[:, None] * D * np.arange(n_out, dtype=np.float64)[None, :])


@pytest.mark.parametrize("fs,nb", SHAPES, ids=[str(nb) for _, nb in SHAPES])
def test_every_bin_of_every_shape_equals_the_exact_phase_channel(gpu_required, fs, nb):
    """Bin k of the bank against freq_xlating_fir_filter_ccc(D, h, k fs / NB, fs) with exact phases on the stream zeroed
    before the sample the bank was opened at (zero history from the opening sample): relative rms < 1e-5 for EVERY bin --
    the project's IQ bar; float32 butterflies and binary-powered twiddles sit near 2e-7."""
    nat = gpu_required
    D, proto, lead, x = _stream(fs, nb)
    produced, bins = _run(nat, fs, nb, False)
    k0 = -(-lead // D)
    assert produced == (len(x) - 1) // D + 1 - k0 and produced >= 150
    assert bins.shape == (nb, produced)
    xz = x.copy()
    xz[:lead] = 0
    ref = _exact_all_bins(xz, D, proto, nb, fs)[:, k0:]
    for k in (0, 1, 7, nb // 2 - 1, nb // 2, nb // 2 + 1, nb - 1):
        one = G.xlating_fir_exact(xz, D, proto, (k if k <= nb // 2 else k - nb) * fs / nb, fs)[k0:]
        assert rel_rms(ref[k], one) < 1e-12, (nb, k)
    errs = np.array([rel_rms(bins[k], ref[k]) for k in range(nb)])
    print("pfbm %d bins: rel rms max %.3e (bin %d) median %.3e" % (nb, errs.max(), int(errs.argmax()), float(np.median(errs))))
    assert errs.max() < 1e-5, (nb, int(errs.argmax()), float(errs.max()))


@pytest.mark.parametrize("fs,nb", SHAPES, ids=[str(nb) for _, nb in SHAPES])
def test_ragged_pushes_give_the_same_bits_as_one_push(gpu_required, fs, nb):
    """pieces shorter than D, shorter than one chunk, a few chunks and a bit: every bin bit for bit what one push gives (the
    first launches still see zero history and run that instantiation; the later ones do not)"""
    nat = gpu_required
    n_one, one = _run(nat, fs, nb, False)
    n_cut, cut = _run(nat, fs, nb, True)
    assert n_one == n_cut
    np.testing.assert_array_equal(one, cut)


def _rotator_residual(y, b):
    """how far y is from b times a rotator r0 inc^n: the phase of y conj(b) against its straight-line fit (rad, max) and the
    magnitude ratio's distance from 1 (max), over the samples where the bin is not tiny"""
    keep = np.abs(b) > 0.05 * np.sqrt(np.mean(np.abs(b) ** 2))
    r = (y.astype(np.complex128) * np.conj(b.astype(np.complex128)))[keep]
    n = np.arange(len(y))[keep]
    ph = np.unwrap(np.angle(r))
    fit = np.polyfit(n, ph, 1)
    mag = np.abs(y.astype(np.complex128))[keep] / np.abs(b.astype(np.complex128))[keep]
    return float(np.max(np.abs(ph - np.polyval(fit, n)))), float(np.max(np.abs(mag - 1.0)))


@pytest.mark.parametrize("fs,nb", [(2.4e6, 192), (12e6, 960)], ids=["192", "960"])
def test_every_bin_as_a_tap_and_fm_only_taps(gpu_required, fs, nb):
    """Every bin opened as a tap (all runs of 16 are full: tap_finalize reads them from the ring), every second one with GNU
    Radio's rotator.  An idle-rotator tap is its bin bit for bit and its discriminator gr's quadrature_demod of the bin; a
    gr_phase tap is its bin times a rotator (a phase that is a straight line in n, magnitude 1); a discriminator-only tap
    gives an ordinary tap's discriminator to 1e-6."""
    nat = gpu_required
    D, taps = G.channel_params(fs, 12500)
    rng = np.random.default_rng(900 + nb)
    x = synth.awgn(rng, D * 170 + 41)
    with nat.Frontend(fs, block_capacity=len(x), out_capacity=1 << 10) as fe:
        fe.pfb_open(nb, D, taps)
        ids = [fe.pfb_tap_open(k, gr_phase=bool(k & 1)) for k in range(nb)]
        only_bins = [1, 2, nb // 2 + 3, nb - 2]
        only = [fe.pfb_tap_open(k, gr_phase=bool(k & 1)) for k in only_bins]
        for c in only:
            fe.chan_set_fm_only(c, True)
        cut = D * 61 + 17
        fe.push(x[:cut])
        fe.push(x[cut:cut + D // 2])
        fe.push(x[cut + D // 2:])
        n_out = fe.pfb_produced()
        assert n_out == 171
        fms = {}
        for k in range(nb):
            y = fe.chan_read_iq(ids[k])
            b = fe.pfb_read_bin(k)
            fms[k] = fe.chan_read_fm(ids[k], 1.0)
            assert len(y) == len(b) == len(fms[k]) == n_out
            if not (k & 1):
                np.testing.assert_array_equal(y, b, err_msg="tap of bin %d" % k)
                np.testing.assert_array_equal(fms[k], G.quadrature_demod_cf(b.astype(np.complex64), 1.0))
            else:
                dphi, dmag = _rotator_residual(y, b)
                assert dphi < 2e-5 and dmag < 1e-4, (k, dphi, dmag)
        for k, c in zip(only_bins, only):
            f = fe.chan_read_fm(c, 1.0)
            assert len(f) == n_out
            assert np.max(np.abs(f - fms[k])) <= 1e-6, (k, float(np.max(np.abs(f - fms[k]))))


def test_pfb192_tap_slots_full_runs_partial_runs_and_duplicates(gpu_required):
    """The tap slot order on a 192-bin bank (tests/test_gpu_round3.py holds the same for 1600 bins): full aligned runs of 16
    (one opened in reverse, one at the last 16 bins) are read from the bank's own ring, a run with one bin missing, an
    unaligned run of 16, scattered bins and a bin opened twice go through the tap matrix; a full run opened between two
    pushes; closing a tap of a full run changes nothing for the others.  Every tap stream is its bin bit for bit."""
    nat = gpu_required
    fs, nb = 2.4e6, 192
    D, taps = G.channel_params(fs, 12500)
    rng = np.random.default_rng(322)
    x = synth.awgn(rng, D * 400 + 55)
    bins = list(range(32, 48)) + list(range(79, 63, -1)) + list(range(176, 192))        # three full runs
    bins += list(range(96, 111))                                                        # 15 of 16
    bins += list(range(120, 136))                                                       # 16 consecutive, unaligned
    bins += [3, 101, 17, 150, 40, 40, 191]                                              # scattered + duplicates of run bins
    with nat.Frontend(fs, block_capacity=len(x), out_capacity=1 << 10) as fe:
        fe.pfb_open(nb, D, taps)
        ids = [fe.pfb_tap_open(k, gr_phase=False) for k in bins]
        cuts = [D * 90 + 31, D * 170 + 7, D * 280]
        fe.push(x[:cuts[0]])
        n_late0 = fe.pfb_produced()
        late = [fe.pfb_tap_open(k, gr_phase=False) for k in range(144, 160)]            # a full run that starts later
        fe.push(x[cuts[0]:cuts[1]])
        fe.chan_close(ids[5])                                                           # bin 37: run 32..47 is no longer full
        fe.push(x[cuts[1]:cuts[2]])
        fe.push(x[cuts[2]:])
        n_out = fe.pfb_produced()
        assert n_out > 390
        ring = {}

        def bin_of(k):
            if k not in ring:
                ring[k] = fe.pfb_read_bin(k)
            return ring[k]

        for j, k in enumerate(bins):
            if j == 5:
                continue
            y = fe.chan_read_iq(ids[j])
            b = bin_of(k)
            assert len(y) == len(b) == n_out, (j, k)
            np.testing.assert_array_equal(y, b, err_msg="tap %d bin %d" % (j, k))
            fm = fe.chan_read_fm(ids[j], 1.0)
            np.testing.assert_array_equal(fm, G.quadrature_demod_cf(b.astype(np.complex64), 1.0))
        for j, k in enumerate(range(144, 160)):
            y = fe.chan_read_iq(late[j])
            b = bin_of(k)[n_late0:]
            assert len(y) == len(b) == n_out - n_late0
            np.testing.assert_array_equal(y, b)


def test_group_of_ten_2p4_msps_banks_same_bits_one_launch_per_block(gpu_required):
    """The production shape: ten 2.4 Msps sources in one process, 20 ms blocks (48 000 samples = 500 frames = 32 chunks per
    member).  Driven through rcf_group_push every bin of every member is bit for bit what the member gives driven alone,
    and once the banks are past their zero-history launch the group issues ONE filterbank launch per block."""
    nat = gpu_required
    fs, nb, G_, blk, n_blk = 2.4e6, 192, 10, 48000, 4
    D, taps = G.channel_params(fs, 12500)
    xs = [synth.awgn(np.random.default_rng(4100 + m), blk * n_blk) for m in range(G_)]

    def open_one():
        fe = nat.Frontend(fs, 0.0, device=0, block_capacity=blk, hist_capacity=1 << 12, out_capacity=1 << 11)
        fe.pfb_open(nb, D, taps)
        return fe

    alone = []
    for m in range(G_):
        fe = open_one()
        try:
            for b in range(n_blk):
                fe.push(xs[m][b * blk:(b + 1) * blk])
            alone.append(np.stack([fe.pfb_read_bin(k) for k in range(nb)]))
        finally:
            fe.close()
    fes = [open_one() for _ in range(G_)]
    try:
        grp = nat.Group(fes)
        try:
            for fe in fes:
                fe.timing_enable(True, classes=[nat.T_PFB])
            launches = []
            for b in range(n_blk):
                grp.push([xs[m][b * blk:(b + 1) * blk] for m in range(G_)])
                grp.sync()
                launches.append(sum(fe.timing_read(nat.T_PFB)[1] for fe in fes))
            # block 0 reaches before the banks' opening sample: ten launches of the zero-history kernel, one by one
            assert launches[0] == G_ and launches[1:] == [1] * (n_blk - 1), launches
            for fe in fes:
                fe.timing_enable(False)
        finally:
            grp.close()
        for m, fe in enumerate(fes):
            got = np.stack([fe.pfb_read_bin(k) for k in range(nb)])
            assert got.shape == alone[m].shape == (nb, blk * n_blk // D)
            np.testing.assert_array_equal(got, alone[m], err_msg="member %d" % m)
    finally:
        for fe in fes:
            fe.close()


def test_fm_enable_is_refused_on_a_192_bin_bank_and_the_bank_runs_on(gpu_required):
    """rcf_pfb_fm_enable has no fused form for this family: RCF_EINVAL, and the bank is what it was"""
    nat = gpu_required
    fs, nb = 2.4e6, 192
    D, taps = G.channel_params(fs, 12500)
    x = synth.awgn(np.random.default_rng(5), D * 120)
    with nat.Frontend(fs, block_capacity=len(x), out_capacity=1 << 10) as fe:
        fe.pfb_open(nb, D, taps)
        fe.push(x[:D * 50])
        for mode in (1, 2):
            with pytest.raises(nat.RcfError) as ei:
                fe.pfb_fm_enable(mode, gr_phase=True)
            assert ei.value.code == nat.RCF_EINVAL
        fe.push(x[D * 50:])
        assert fe.pfb_produced() == 120
        b = fe.pfb_read_bin(5)
    ref = G.xlating_fir_exact(x, D, taps, 5 * fs / nb, fs)
    assert len(b) == 120 and rel_rms(b, ref) < 1e-5


def test_one_tap_per_branch_prototype_is_zero_padded(gpu_required):
    """a prototype of at most NB taps (one per branch) runs the two-taps-per-branch kernel with a row of zeros: the bins are
    still the exact-phase channel of THAT prototype, however the stream is cut"""
    nat = gpu_required
    fs, nb = 2.4e6, 192
    D = nb // 2
    proto = G.low_pass_2(1.0, fs, 6250.0, 12500.0, 20.0, G.WIN_HAMMING)
    assert nb // 2 < len(proto) <= nb, len(proto)
    assert nat.pfb_shape_family(nb, D, len(proto)) == 3
    rng = np.random.default_rng(77)
    x = synth.awgn(rng, D * 160 + 13)
    ks = [0, 5, 95, 96, 97, 191]
    outs = []
    for cuts in ([0, len(x)], [0, 7, D * 3 + 1, D * 40, len(x)]):
        with nat.Frontend(fs, block_capacity=len(x), out_capacity=1 << 10) as fe:
            fe.pfb_open(nb, D, proto)
            for a, b in zip(cuts[:-1], cuts[1:]):
                fe.push(x[a:b])
            assert fe.pfb_produced() == 161
            outs.append([fe.pfb_read_bin(k) for k in ks])
    for k, a, b in zip(ks, outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)
        ref = G.xlating_fir_exact(x, D, proto, (k if k <= nb // 2 else k - nb) * fs / nb, fs)
        assert rel_rms(a, ref) < 1e-5, (k, rel_rms(a, ref))


def test_receiver_2p4_msps_every_on_grid_request_meets_the_fm_bar(gpu_required):
    """frontend_mode = 'pfb' with pfb_mixed_radix at 2.4 Msps: all 191 requestable on-grid channels through
    receiver.connect_channel against the GR-faithful oracle channel (P25 discriminator gain), as
    tests/test_gpu_round3.py does at 1600 bins.  Unit noise + 8 NBFM carriers of +30 dB per pass, 24 passes, so every bin
    carries a carrier once: wideband over carrier power 10 log10((1 + 8 x 5.2) / 5.2) = 9.1 dB, under the default
    pfb_parity_env_db of 15.3.  Discriminator < 1e-4 rms for every served stream; at least 180 served by the bank; the
    direct-served ones hold the IQ bar.  For the table every bin is also opened as a bank tap whatever the routing."""
    from rcf import native, receiver
    nat = gpu_required
    fs, nb, fc_hz = 2.4e6, 192, 855000000
    D, taps = G.channel_params(fs, 12500)
    gain = G.p25_fm_gain(25000.0)
    n_out, skip, n_pass = 600, 8, 24
    per = nb // n_pass
    rows = {}
    metrics = {"bank": 0, "parity": 0}
    for p in range(n_pass):
        rng = np.random.default_rng(3300 + p)
        x = synth.awgn(rng, D * n_out).astype(np.complex128)
        bins = [p + n_pass * m for m in range(per)]
        offs = [(k if k < nb // 2 else k - nb) * fs / nb for k in bins]
        for f in offs:
            x += synth.nbfm_carrier(len(x), fs, f, 300.0 + 2700.0 * rng.random(), 2500.0,
                                    synth.snr_amp(30.0, 12500.0, fs))
        x = x.astype(np.complex64)
        cfg = types.SimpleNamespace(sources={0: dict(type="synthetic", center_freq=fc_hz, samp_rate=int(fs))},
                                    frontend_mode="pfb", pfb_mixed_radix=True)
        tb = receiver.receiver(cfg, frontend_factory=lambda sr, cf, dev: native.Frontend(sr, cf, device=dev,
                                                                                          block_capacity=len(x)))
        try:
            plan = tb.sources[0]["pfb"]
            assert plan is not None and plan["n_bins"] == nb
            fe = tb.sources[0]["block"]
            served = []
            for k, f in zip(bins, offs):
                if abs(f) >= fs / 2:                       # bin 96 = -fs/2: not requestable (|offset| < fs/2)
                    served.append(None)
                    continue
                bid, _ = tb.connect_channel(12500, int(fc_hz + f))
                served.append(tb.channels[bid])
            extra = [None if (ch is None or ch.pfb_bin is not None) else fe.pfb_tap_open(k, gr_phase=True)
                     for k, ch in zip(bins, served)]
            m = tb.metrics()
            metrics["bank"] += m["rcf_pfb_served_by_bank"]
            metrics["parity"] += m["rcf_pfb_direct_parity_budget"]
            tb.feed(0, x)
            got = [None if ch is None else (ch.read_iq(), ch.read_fm(gain)) for ch in served]
            got_tap = [None if t is None else (fe.chan_read_iq(t), fe.chan_read_fm(t, gain)) for t in extra]
        finally:
            tb.close()
        cts, incs = [], []
        for f in offs:
            ct, incr = OC.xlating_composite(taps, D, f, fs)
            cts.append(ct)
            incs.append(incr)
        yo, fo = OC.channel_bank(x, D, np.array(cts), np.array(incs), gains=[gain] * per)
        for m, (k, f, ch) in enumerate(zip(bins, offs, served)):
            if ch is None:
                continue
            y, fm = got[m]
            assert len(y) == n_out and len(fm) == n_out
            row = {"bin": k, "offset_hz": f, "served_by": "bank" if ch.pfb_bin is not None else "direct",
                   "predicted_fm_rms": receiver.receiver.pfb_predicted_fm_error(plan, k),
                   "leak_l2": plan["leak"][k % nb],
                   "served_fm_rms": rms(fm[skip:], fo[m][skip:]),
                   "served_iq_rel_rms": rel_rms(y[skip:], yo[m][skip:])}
            yt, ft = got[m] if ch.pfb_bin is not None else got_tap[m]
            row["bank_tap_fm_rms"] = rms(ft[skip:], fo[m][skip:])
            row["bank_tap_iq_rel_rms"] = rel_rms(yt[skip:], yo[m][skip:])
            rows[k] = row
    table = [rows[k] for k in sorted(rows)]
    assert len(table) == nb - 1
    served_bank = [r for r in table if r["served_by"] == "bank"]
    worst = max(table, key=lambda r: r["served_fm_rms"])
    worst_bank = max(served_bank, key=lambda r: r["served_fm_rms"])
    margin = plan["parity"]["margin"]
    ratios = [r["bank_tap_fm_rms"] / (r["predicted_fm_rms"] / margin) for r in table if r["predicted_fm_rms"] / margin > 1e-5]
    summary = {
        "requests": len(table), "served_by_bank": len(served_bank), "served_by_direct": len(table) - len(served_bank),
        "served_fm_rms_max": worst["served_fm_rms"], "served_fm_rms_max_bin": worst["bin"],
        "bank_served_fm_rms_max": worst_bank["served_fm_rms"], "bank_served_fm_rms_max_bin": worst_bank["bin"],
        "served_iq_rel_rms_max": max(r["served_iq_rel_rms"] for r in table),
        "bank_tap_fm_rms_max_all_bins": max(r["bank_tap_fm_rms"] for r in table),
        "bank_tap_bins_over_1e-4": sum(1 for r in table if r["bank_tap_fm_rms"] > 1e-4),
        # (below a prediction of 1e-5 the float32 floor dominates; None: no bin predicts more than that)
        "measured_over_predicted_max_margin_removed": max(ratios) if ratios else None,
        "metrics_served_by_bank": metrics["bank"], "metrics_direct_parity_budget": metrics["parity"],
    }
    _dump("pfbm_192_allbins_vs_gr.json", {
        "fs": fs, "bins": nb, "decim": D, "taps": len(taps), "outputs": n_out, "fm_gain": gain,
        "environment": "unit-variance noise + 8 NBFM carriers (+30 dB in 12.5 kHz) per pass, 24 passes",
        "parity": plan["parity"], "summary": summary, "rows": table})
    print("pfbm 192 all bins vs GR:", json.dumps(summary))
    assert metrics["bank"] == len(served_bank) and metrics["parity"] == len(table) - len(served_bank)
    # the bar, for every request
    assert worst["served_fm_rms"] < 1e-4, worst
    assert len(served_bank) >= 180, len(served_bank)
    assert all(r["served_iq_rel_rms"] < 1e-5 for r in table if r["served_by"] == "direct")
