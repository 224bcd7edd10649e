"""What stands behind the mixed-radix filterbanks (radiocapture-rf_amd/csrc/pfbm.hip: 160, 192, 480, 640, 960 and 1280 bins
at D = NB / 2), which tests/test_gpu_pfbm.py leaves out: an output ring that wraps under the chunks, lagging and keeping-up
readers, every consumer of a bin (stage-2 channels, symbol filter, AGC, voice chain, source shift, raw ingest) at the smallest
and the largest row pitch, grouped launches whose members differ, seeded fuzz over this family's shapes, and the limits of
the wideband buffer and the prototype.  References are float64 exact-phase arithmetic (oracle.grspec.xlating_fir_exact), or
the GNU-Radio-faithful oracle where a discriminator, an AGC or the voice chain is compared; "the same bits" is
assert_array_equal.  Per-bin relative bars are taken on noise-only streams; where a carrier is needed only the bins that
carry one are compared (tests/test_gpu_pfbm.py::_stream says why)."""
import math

import numpy as np
import pytest

import agc_ref as A
from oracle import audio as OA
from oracle import grspec as G
from rcf import audio as host_audio
from rcf import synth

from test_gpu_cqpsk import _assert_same_bits, _fades
from test_gpu_fuzz import _oracle_life, _seeds
from test_gpu_pfbm import CHUNK, SHAPES, _rotator_residual, rel_rms, rms

pytestmark = pytest.mark.gpu

_IDS = [str(nb) for _, nb in SHAPES]
_ENDS = [SHAPES[0], SHAPES[-1]]                 # the smallest and the largest row pitch: 160 and 1280 bins
_END_IDS = [str(nb) for _, nb in _ENDS]


def _f_bin(k, nb, fs):
    return (k if k <= nb // 2 else k - nb) * fs / nb


def _bank_frames(S0, S1, D, start):
    """(first, count) of the frames a push of samples [S0, S1) yields on a bank opened at sample `start`: frames sit on the
    absolute decimation grid n D, from the first multiple of D at or after `start`"""
    n_lo = max(-(-S0 // D), -(-start // D))
    n_hi = (S1 - 1) // D
    return n_lo, max(n_hi - n_lo + 1, 0)


def _pieces(total, sizes):
    """`sizes` over and over until `total` samples are cut up (the last piece takes what is left)"""
    out, i = [], 0
    while total > 0:
        out.append(min(sizes[i % len(sizes)], total))
        total -= out[-1]
        i += 1
    return out


# ------------------------------------------------------------------ 1. ring wrap, mid-stream open, lagging reader

_WRAP_CAP = 64
_wrap_runs = {}


def _wrap_case(fs, nb):
    D, proto = G.channel_params(fs, 12500)
    assert nb == 2 * D
    F = CHUNK[nb]
    rng = np.random.default_rng(8100 + nb)
    lead = 2 * D + int(rng.integers(1, D))                       # no multiple of D
    n = lead + D * 300 + int(rng.integers(1, D))
    x = synth.awgn(rng, n)
    # one sample, nothing, no frame at all, a chunk less a few samples, several chunks and a bit, a few frames, a chunk and
    # a bit: launches begin anywhere in the ring, so their chunks keep landing across its end
    pieces = _pieces(n - lead, [1, 0, D - 1, F * D - 5, 3 * F * D + D // 3, 2 * D + 7, F * D + 3])
    runs = [list(range(16, 32)), list(range(nb - 16, nb))]       # full aligned runs of 16: tap_finalize reads them from the ring
    tap_bins = runs[0] + runs[1] + [5]
    return D, proto, F, lead, x, pieces, tap_bins


def _wrap_run(nat, fs, nb, out_cap):
    """the stream read as it goes: bins and taps after every push.  Computed once per (shape, ring)"""
    key = (nb, out_cap)
    if key in _wrap_runs:
        return _wrap_runs[key]
    D, proto, F, lead, x, pieces, tap_bins = _wrap_case(fs, nb)
    watch = sorted(set(tap_bins) | {0, nb // 2 + 1, nb - 1})
    bins = {k: [] for k in watch}
    iq = [[] for _ in tap_bins]
    fm = [[] for _ in tap_bins]
    with nat.Frontend(fs, block_capacity=max(pieces) + 16, hist_capacity=1 << 14, out_capacity=out_cap) as fe:
        fe.push(x[:lead])
        fe.pfb_open(nb, D, proto)
        ids = [fe.pfb_tap_open(k, gr_phase=False) for k in tap_bins]
        at = lead
        for s in pieces:
            fe.push(x[at:at + s])
            at += s
            for k in watch:
                bins[k].append(fe.pfb_read_bin(k))
            for j, a in enumerate(fe.chan_read_many(ids, "iq", cap_each=2 * _WRAP_CAP)):
                iq[j].append(a.copy())
            for j, a in enumerate(fe.chan_read_many(ids, "fm", 1.0, cap_each=2 * _WRAP_CAP)):
                fm[j].append(a.copy())
        assert at == len(x)
        produced = fe.pfb_produced()
        lag = fe.pfb_read_bin(7)                                  # a bin nobody has read so far
    _wrap_runs[key] = dict(produced=produced, lag=lag, bins={k: np.concatenate(v) for k, v in bins.items()},
                           iq=[np.concatenate(v) for v in iq], fm=[np.concatenate(v) for v in fm])
    return _wrap_runs[key]


@pytest.mark.parametrize("fs,nb", SHAPES, ids=_IDS)
def test_ring_wrap_midstream_open_and_lagging_reader(gpu_required, fs, nb):
    """A 64-frame output ring under a 300-frame stream (tests/test_gpu_round2.py holds the same for 1600 bins): the bank
    opened after a lead-in that is no multiple of D, ragged pushes whose chunks land on both sides of the ring's end, three
    bins and 33 taps (two full aligned runs of 16, which tap_finalize reads from the bank's ring, and a scattered one) read
    after every push.  The frame count is that of the absolute decimation grid, the bins meet the 1e-5 bar against the
    exact-phase channel on the stream zeroed before the opening sample, every idle-rotator tap is its bin bit for bit (and
    its discriminator gr's quadrature_demod of it), a bin nobody has read returns the newest 64 frames, and on 192 and
    1280 bins all of it is bit for bit what a ring that never wraps gives."""
    nat = gpu_required
    D, proto, F, lead, x, pieces, tap_bins = _wrap_case(fs, nb)
    k0 = -(-lead // D)
    total = (len(x) - 1) // D + 1 - k0
    # the schedule does what it is meant to: chunks of one launch on both sides of the ring's end, more than once
    straddles, at = 0, lead
    for s in pieces:
        n_lo, cnt = _bank_frames(at, at + s, D, lead)
        assert cnt <= _WRAP_CAP
        for c0 in range(0, cnt, F):
            slot = (n_lo + c0 - k0) % _WRAP_CAP
            straddles += slot + min(F, cnt - c0) > _WRAP_CAP
        at += s
    assert straddles >= 2 and 1 in pieces and 0 in pieces, (nb, straddles)
    got = _wrap_run(nat, fs, nb, _WRAP_CAP)
    assert got["produced"] == total and total > 4 * _WRAP_CAP
    xz = x.copy()
    xz[:lead] = 0
    worst = 0.0
    for k in (0, nb // 2 + 1, nb - 1):
        want = G.xlating_fir_exact(xz, D, proto, _f_bin(k, nb, fs), fs)[k0:]
        assert len(got["bins"][k]) == len(want) == total, (nb, k)
        e = rel_rms(got["bins"][k], want)
        worst = max(worst, e)
        assert e < 1e-5, (nb, k, e)
    for j, k in enumerate(tap_bins):
        b = got["bins"][k]
        assert len(b) == total
        np.testing.assert_array_equal(got["iq"][j], b, err_msg="%d bins: tap of bin %d" % (nb, k))
        np.testing.assert_array_equal(got["fm"][j], G.quadrature_demod_cf(b, 1.0), err_msg="%d bins: fm of bin %d" % (nb, k))
    want7 = G.xlating_fir_exact(xz, D, proto, _f_bin(7, nb, fs), fs)[k0:][-_WRAP_CAP:]
    assert len(got["lag"]) == _WRAP_CAP
    e = rel_rms(got["lag"], want7)
    worst = max(worst, e)
    assert e < 1e-5, (nb, "lagging reader", e)
    print("pfbm %d bins, 64-frame ring: %d chunks across the ring's end, rel rms max %.3e" % (nb, straddles, worst))
    if nb in (192, 1280):
        flat = _wrap_run(nat, fs, nb, 1 << 10)
        assert flat["produced"] == total
        for k in got["bins"]:
            np.testing.assert_array_equal(got["bins"][k], flat["bins"][k], err_msg="%d bins: bin %d" % (nb, k))
        for j, k in enumerate(tap_bins):
            np.testing.assert_array_equal(got["iq"][j], flat["iq"][j], err_msg="%d bins: tap of bin %d" % (nb, k))
            np.testing.assert_array_equal(got["fm"][j], flat["fm"][j], err_msg="%d bins: fm of bin %d" % (nb, k))
        np.testing.assert_array_equal(got["lag"], flat["lag"][-_WRAP_CAP:])


# ------------------------------------------------------------------ 2. consumers of a bin

_LEAD_FRAMES = 5            # the banks below are opened 5 D + 17 samples in: their first frame is 6, no multiple of any chunk


def _n_for(frames, D):
    """a stream length that gives `frames` frames from a bank opened _LEAD_FRAMES D + 17 samples in, with a ragged tail"""
    return (frames + _LEAD_FRAMES + 1) * D - 40


@pytest.mark.parametrize("fs,nb", _ENDS, ids=_END_IDS)
def test_stage2_channels_and_symbol_filter_on_a_bin(gpu_required, fs, nb):
    """rcf_pfb_chan_open on bins of this family (tests/test_gpu_round2.py holds the same for 1600 bins): channel.py's rule at
    the bin rate (25 kS/s: D = 1, 3 taps) with a +2 kHz residual offset on a bin that carries an NBFM carrier 2 kHz off its
    centre, a second one on bin NB - 1 (carrier 1.5 kHz below its centre), and a symbol filter behind a plain tap; the
    stream in two pieces, cut inside a chunk.  IQ < 2e-5 against xlating_fir_ccc over the exact-phase bin, discriminator
    < 1e-4 rms, the tap the bin itself (< 1e-5), its symbol stream np.convolve of the oracle discriminator (< 1e-4)."""
    nat = gpu_required
    D, taps = G.channel_params(fs, 12500)
    F = CHUNK[nb]
    rng = np.random.default_rng(8200 + nb)
    lead, n_frames = _LEAD_FRAMES * D + 17, 400
    ka, da, kb, db = nb // 4 + 3, 2000.0, nb - 1, -1500.0
    n = _n_for(n_frames, D)
    x = synth.awgn(rng, n).astype(np.complex128)
    for k, d in ((ka, da), (kb, db)):
        x += synth.nbfm_carrier(n, fs, _f_bin(k, nb, fs) + d, 800.0, 2500.0, synth.snr_amp(30.0, 12500.0, fs))
    x = x.astype(np.complex64)
    bin_rate = fs / D
    with nat.Frontend(fs, block_capacity=n, hist_capacity=1 << 14, out_capacity=1 << 10) as fe:
        fe.push(x[:lead])
        fe.pfb_open(nb, D, taps)
        ca = fe.pfb_chan_open(ka, 12500, da)
        cb = fe.pfb_chan_open(kb, 12500, db)
        tap = fe.pfb_tap_open(ka, gr_phase=False)
        fe.chan_fm_filter(tap, 5.0, np.full(5, 0.2, dtype=np.float32))
        half = D * (_LEAD_FRAMES + 1 + 10 * F + F // 2 + 1) + 5               # 10 chunks and a half from the first frame
        fe.push(x[lead:half])
        fe.push(x[half:])
        infos = [fe.chan_info(ca), fe.chan_info(cb)]
        got = [(fe.chan_read_iq(c), fe.chan_read_fm(c, 5.0)) for c in (ca, cb)]
        yt, sym = fe.chan_read_iq(tap), fe.chan_read_sym(tap)
    k0 = _LEAD_FRAMES + 1
    xz = x.copy()
    xz[:lead] = 0
    D2, taps2 = G.channel_params(bin_rate, 12500)
    assert D2 == 1
    for (k, d), info, (y2, fm2) in zip(((ka, da), (kb, db)), infos, got):
        assert (info["decim"], info["ntaps"]) == (D2, len(taps2)), info
        stage1 = G.xlating_fir_exact(xz, D, taps, _f_bin(k, nb, fs), fs)[k0:].astype(np.complex64)
        yo = G.xlating_fir_ccc(stage1, D2, taps2, d, bin_rate)
        fo = G.quadrature_demod_cf(yo, 5.0)
        assert len(y2) == len(yo) == len(fm2) == n_frames
        e_iq, e_fm = rel_rms(y2, yo), rms(fm2[4:], fo[4:])
        print("pfbm %d bins: stage-2 channel on bin %d: iq rel rms %.3e, fm rms %.3e" % (nb, k, e_iq, e_fm))
        assert e_iq < 2e-5 and e_fm < 1e-4, (nb, k, e_iq, e_fm)
    stage1 = G.xlating_fir_exact(xz, D, taps, _f_bin(ka, nb, fs), fs)[k0:].astype(np.complex64)
    assert len(yt) == n_frames and rel_rms(yt, stage1) < 1e-5, (nb, rel_rms(yt, stage1))
    so = np.convolve(G.quadrature_demod_cf(stage1, 5.0).astype(np.float64), np.full(5, 0.2))[:n_frames]
    assert len(sym) == n_frames and rms(sym[8:], so[8:]) < 1e-4, (nb, rms(sym[8:], so[8:]))


@pytest.mark.parametrize("fs,nb", _ENDS, ids=_END_IDS)
def test_consumers_ragged_pushes_equal_one_push(gpu_required, fs, nb):
    """three stage-2 channels and three taps (one idle, one with GNU Radio's rotator, one discriminator-only) behind a bank
    opened in mid-stream: one push and eight ragged ones give the same bits, IQ and discriminator (tests/test_gpu_round3.py
    holds the same for the 256-bin bank)."""
    nat = gpu_required
    D, taps = G.channel_params(fs, 12500)
    F = CHUNK[nb]
    rng = np.random.default_rng(8300 + nb)
    lead = _LEAD_FRAMES * D + 17
    n = _n_for(260, D)
    x = synth.awgn(rng, n)
    sizes = [1, D - 1, F * D - 3, 2 * D + 5, 5 * F * D + D // 2, 3, D // 2]
    cuts = [lead]
    for s in sizes:
        cuts.append(cuts[-1] + s)
    assert cuts[-1] < n
    cuts.append(n)                                             # eight pieces

    def run(edges):
        with nat.Frontend(fs, block_capacity=n, hist_capacity=1 << 14, out_capacity=1 << 10) as fe:
            fe.push(x[:lead])
            fe.pfb_open(nb, D, taps)
            s2 = [fe.pfb_chan_open(k, 12500, d) for k, d in ((3, 0.0), (nb // 2 + 2, 2000.0), (nb - 1, -3125.0))]
            t_idle = fe.pfb_tap_open(nb // 4, gr_phase=False)
            t_gr = fe.pfb_tap_open(nb // 4 + 1, gr_phase=True)
            t_only = fe.pfb_tap_open(nb - 2, gr_phase=True)
            fe.chan_set_fm_only(t_only, True)
            for a, b in zip(edges[:-1], edges[1:]):
                fe.push(x[a:b])
            out = [fe.pfb_produced()]
            for c in s2 + [t_idle, t_gr]:
                out += [fe.chan_read_iq(c), fe.chan_read_fm(c, 1.0)]
            out.append(fe.chan_read_fm(t_only, 1.0))
        return out

    one, cut = run([lead, n]), run(cuts)
    assert one[0] == cut[0] == 260 and len(one) == len(cut) == 12
    for i, (a, b) in enumerate(zip(one[1:], cut[1:])):
        assert len(a) == 260
        np.testing.assert_array_equal(a, b, err_msg="%d bins: output %d" % (nb, i))


@pytest.mark.parametrize("fs,nb", _ENDS, ids=_END_IDS)
def test_agc_on_a_bank_tap(gpu_required, fs, nb):
    """analog.feedforward_agc_cc(1024, 1.0) behind a tap of this family, under 20 dB fades: bit for bit the restatement
    (tests/agc_ref.py) of the same tap's IQ, as tests/test_gpu_cqpsk.py holds it for the 1600-bin bank"""
    nat = gpu_required
    D, taps = G.channel_params(fs, 12500)
    rng = np.random.default_rng(8400 + nb)
    lead = _LEAD_FRAMES * D + 17
    n = _n_for(3000, D)
    f_k = 21 * fs / nb + 1500.0
    x = (0.02 * synth.awgn(rng, n) + synth.nbfm_carrier(n, fs, f_k, 800.0, 2000.0, 0.5)).astype(np.complex64)
    x = _fades(x, fs, 0.02)
    with nat.Frontend(fs, 0.0, device=0, block_capacity=D * 1000, hist_capacity=1 << 15, out_capacity=1 << 13) as fe:
        fe.push(x[:lead])
        fe.pfb_open(nb, D, taps)
        tap = fe.pfb_tap_open(21, gr_phase=True)
        other = fe.pfb_tap_open(22, gr_phase=True)
        fe.chan_agc(tap, 1024, 1.0)
        for a in range(lead, n, D * 1000):
            fe.push(x[a:a + D * 1000])
        agc = fe.chan_read_agc(tap)
        iq = fe.chan_read_iq(tap)
        fe.chan_read_iq(other)
    assert len(agc) == len(iq) == 3000
    _assert_same_bits(agc, A.feedforward_agc(iq, 1024, 1.0), nb)
    assert float(np.abs(agc[1500:]).max()) > 0.5


def test_voice_chain_on_a_192_bin_tap(gpu_required):
    """rcf_chan_audio_open on a tap of a bin with an NBFM carrier (1 kHz tone, 2.5 kHz deviation), ragged pushes: the 8 kHz
    audio against oracle/audio.py's chain on the exact-phase bin, < 1e-4 rms -- parameters and bar of
    tests/test_gpu_audio.py::test_analog_voice_chain_equals_oracle"""
    nat = gpu_required
    fs, nb = 2.4e6, 192
    D, taps = G.channel_params(fs, 12500)
    rng = np.random.default_rng(8500)
    lead, n_frames, k = _LEAD_FRAMES * D + 17, 6000, 57
    n = _n_for(n_frames, D)
    x = synth.nbfm_carrier(n, fs, _f_bin(k, nb, fs), 1000.0, 2500.0, 0.4) + 0.01 * synth.awgn(rng, n)
    x = x.astype(np.complex64)
    cuts = [lead, lead + 100000, lead + 100000 + D * 2000 + 17, lead + 450001, n]
    with nat.Frontend(fs, block_capacity=n, out_capacity=1 << 13) as fe:
        fe.push(x[:lead])
        fe.pfb_open(nb, D, taps)
        tap = fe.pfb_tap_open(k, gr_phase=False)
        host_audio.open_analog_voice(fe, tap, 25000)
        fe.timing_enable(True)
        for a, b in zip(cuts[:-1], cuts[1:]):
            fe.push(x[a:b])
        assert fe.timing_read(nat.T_AUDIO)[1] == 4
        n_audio, n_ungated = fe.chan_audio_produced(tap)
        audio = fe.chan_read_audio(tap)
    xz = x.copy()
    xz[:lead] = 0
    y = G.xlating_fir_exact(xz, D, taps, _f_bin(k, nb, fs), fs)[_LEAD_FRAMES + 1:].astype(np.complex64)
    assert len(y) == n_frames
    st = OA.analog_chain(y, 25000.0, stages=True)
    assert n_ungated == len(st["gated"]) == len(y)                         # the noise keeps the squelch open
    assert len(audio) == n_audio == len(st["audio"]) == (len(y) * 8 + 24) // 25
    e = rms(audio, st["audio"])
    print("pfbm 192 bins: voice chain on a tap, audio rms error %.3e (signal rms %.3f)" % (e, rms(audio, 0 * audio)))
    assert e < 1e-4
    seg = audio[1500:].astype(np.float64)
    c = 2 * np.mean(seg * np.exp(-2j * math.pi * 1000.0 * np.arange(len(seg)) / 8000.0))
    assert 1.0 < abs(c) < 1.35


def test_source_shift_reaches_192_bin_taps(gpu_required):
    """rcf_source_shift on a 192-bin bank (tests/test_gpu_round2.py holds the same for 1600 bins): the taps' rotators apply
    the Hz correction; the discriminator mean of a tapped bin and of a direct channel at the same offset both move by
    -2 pi 150 / 25000, within 2e-3"""
    nat = gpu_required
    fs, nb, k = 2.4e6, 192, 40
    D, taps = G.channel_params(fs, 12500)
    rng = np.random.default_rng(8600)
    n_frames = 600
    x = synth.awgn(rng, D * n_frames).astype(np.complex128) * 0.05
    x += synth.nbfm_carrier(len(x), fs, k * fs / nb, 1000.0, 1500.0, 1.0)
    x = x.astype(np.complex64)
    with nat.Frontend(fs, block_capacity=len(x), out_capacity=1 << 10) as fe:
        fe.pfb_open(nb, D, taps)
        tap = fe.pfb_tap_open(k, gr_phase=False)
        direct = fe.chan_open(12500, k * fs / nb)
        fe.push(x[: D * 300])
        fm_a, fd_a = fe.chan_read_fm(tap, 1.0), fe.chan_read_fm(direct, 1.0)
        fe.source_shift(150.0)
        fe.push(x[D * 300:])
        fm_b, fd_b = fe.chan_read_fm(tap, 1.0), fe.chan_read_fm(direct, 1.0)
    assert len(fm_a) == len(fd_a) == len(fm_b) == len(fd_b) == 300
    want = -2 * math.pi * 150.0 / 25000.0               # NCO moved up by 150 Hz: the carrier sits 150 Hz lower
    assert abs((np.mean(fm_b[50:]) - np.mean(fm_a[50:])) - want) < 2e-3
    assert abs((np.mean(fd_b[50:]) - np.mean(fd_a[50:])) - want) < 2e-3


@pytest.mark.parametrize("fmt_name,dtype,scale,offset", [
    ("FMT_U8", np.uint8, 1.0 / 128.0, 127.4),          # rtl-sdr wire format: the 2 and 2.4 Msps sources
    ("FMT_S16", np.int16, 1.0 / 2048.0, 0.0),
])
def test_raw_ingest_feeds_a_192_bin_bank(gpu_required, fmt_name, dtype, scale, offset):
    """rcf_push_raw into a 192-bin bank: every bin bit for bit what rcf_push_iq of the host conversion
    (float(raw) - offset) * scale gives (tests/test_gpu_parity.py::test_wire_format_ingest_equals_host_conversion)"""
    nat = gpu_required
    fs, nb = 2.4e6, 192
    D, taps = G.channel_params(fs, 12500)
    rng = np.random.default_rng(8700)
    info = np.iinfo(dtype)
    n = D * 300 + 1                                          # odd length: the converter's tail path
    raw = rng.integers(info.min, info.max + 1, size=2 * n).astype(dtype)
    x = ((raw.astype(np.float32) - np.float32(offset)) * np.float32(scale)).view(np.complex64)
    cut = 7001
    with nat.Frontend(fs, block_capacity=n, out_capacity=1 << 10) as fe:
        fe.pfb_open(nb, D, taps)
        fe.push_raw(raw[: 2 * cut], getattr(nat, fmt_name), scale, offset)
        fe.push_raw(raw[2 * cut:], getattr(nat, fmt_name), scale, offset)
        got = np.stack([fe.pfb_read_bin(k) for k in range(nb)])
    with nat.Frontend(fs, block_capacity=n, out_capacity=1 << 10) as fe:
        fe.pfb_open(nb, D, taps)
        fe.push(x[:cut])
        fe.push(x[cut:])
        want = np.stack([fe.pfb_read_bin(k) for k in range(nb)])
    assert got.shape == want.shape == (nb, 301)
    np.testing.assert_array_equal(got.view(np.float32), want.view(np.float32))
    ref = G.xlating_fir_exact(x, D, taps, 5 * fs / nb, fs)
    assert rel_rms(got[5], ref) < 1e-5


# ------------------------------------------------------------------ 3. a group whose members differ

def test_mixed_group_with_unequal_members(gpu_required):
    """Eight front-ends in one rcf_group: two 192-bin banks, a 160-bin one, two 480-bin ones, a 1280-bin one, a 400-bin one
    (5 Msps) and a member without a bank that holds a direct channel; every bank with a full run of 16 taps, scattered taps
    and a gr_phase one.  Five blocks whose lengths differ per member and per block (chunk counts differ inside the
    two-member launches), one 192-bin member with fewer than D samples in block 2 (no frame), the second 480-bin member
    opening its bank only before block 2 (its zero-history launch beside a sibling in steady state).  Every bin, every tap
    stream and the direct channel are bit for bit what the same member gives driven alone with the same cuts, and the
    filterbank launches per block are what the grouping rule gives for this schedule: members of one shape whose launch
    no longer reaches before their opening sample share one launch, everyone else launches alone."""
    nat = gpu_required
    #           fs     bins  bank opened before block   frames per block
    members = [(2.4e6, 192,  0,                          [40, 37, 50, 21, 33]),
               (2.4e6, 192,  0,                          [40, 52, 0, 45, 18]),
               (2.0e6, 160,  0,                          [30, 30, 41, 12, 25]),
               (6.0e6, 480,  0,                          [20, 17, 26, 9, 30]),
               (6.0e6, 480,  2,                          [20, 23, 19, 26, 11]),
               (16e6,  1280, 0,                          [10, 13, 7, 9, 12]),
               (5.0e6, 400,  0,                          [30, 28, 33, 20, 25]),
               (2.4e6, None, None,                       None)]
    extra = [[7, 11, 0, 5, 40], [7, 11, 0, 0, 3], [1, 0, 33, 2, 9], [100, 3, 0, 77, 5], [0, 9, 130, 1, 60],
             [300, 0, 17, 5, 1], [9, 0, 150, 3, 11]]
    n_blk, f_direct = 5, 150000.0
    lens, xs = [], []
    for m, (fs, nb, _, frames) in enumerate(members):
        if nb is None:
            lens.append([5000, 3001, 4096, 777, 6000])
        else:
            lens.append([nb // 2 * f + e if f else nb // 4 for f, e in zip(frames, extra[m])])
        xs.append(synth.awgn(np.random.default_rng(9000 + m), sum(lens[m])))
    edges = [np.concatenate([[0], np.cumsum(l)]) for l in lens]

    # ---- what the grouping rule gives for this schedule: (bins) -> members in steady state, and the ones that go alone
    expected, chunks = [], []
    for b in range(n_blk):
        steady, alone, ch = {}, 0, {}
        for m, (fs, nb, opened, _) in enumerate(members):
            if nb is None or b < opened:
                continue
            D, start = nb // 2, int(edges[m][opened])
            n_lo, cnt = _bank_frames(int(edges[m][b]), int(edges[m][b + 1]), D, start)
            ch[m] = (cnt, n_lo * D - (2 * nb - 1) < start)      # two taps per branch: the window reaches 2 NB - 1 samples back
            if cnt == 0:
                continue
            if ch[m][1]:
                alone += 1
            else:
                steady.setdefault(nb, []).append(m)
        expected.append(alone + sum(1 for v in steady.values()))
        chunks.append(ch)
    F192, F480 = CHUNK[192], CHUNK[480]
    assert all(z for _, z in chunks[0].values()) and not any(z for _, z in chunks[1].values())
    assert -(-chunks[1][0][0] // F192) != -(-chunks[1][1][0] // F192)          # unequal chunk counts inside one launch
    assert chunks[2][1] == (0, False) and chunks[2][0][0] > 0                  # a member without a frame
    assert chunks[2][4][1] and not chunks[2][3][1]                             # zero history beside a steady sibling
    assert not chunks[3][4][1] and -(-chunks[3][3][0] // F480) != -(-chunks[3][4][0] // F480)

    def open_all():
        fes = []
        for fs, nb, _, _ in members:
            fes.append(nat.Frontend(fs, 0.0, device=0, block_capacity=1 << 16, hist_capacity=1 << 14, out_capacity=1 << 10))
        return fes

    def open_bank(fe, fs, nb):
        D, taps = G.channel_params(fs, 12500)
        assert nb == 2 * D
        fe.pfb_open(nb, D, taps)
        tb = list(range(16, 32)) + [3, nb // 2 + 1, nb - 1]
        return [fe.pfb_tap_open(k, gr_phase=False) for k in tb] + [fe.pfb_tap_open(7, gr_phase=True)]

    def drive(grouped):
        fes = open_all()
        ids = [None] * len(members)
        launches = []
        try:
            grp = nat.Group(fes) if grouped else None
            try:
                direct = fes[-1].chan_open(12500, f_direct)
                if grouped:
                    for fe in fes:
                        fe.timing_enable(True, classes=[nat.T_PFB])
                for b in range(n_blk):
                    for m, (fs, nb, opened, _) in enumerate(members):
                        if opened == b:
                            ids[m] = open_bank(fes[m], fs, nb)
                    blocks = [xs[m][int(edges[m][b]):int(edges[m][b + 1])] for m in range(len(members))]
                    if grouped:
                        grp.push(blocks)
                        grp.sync()
                        launches.append(sum(fe.timing_read(nat.T_PFB)[1] for fe in fes))
                    else:
                        for fe, blk in zip(fes, blocks):
                            fe.push(blk)
                if grouped:
                    for fe in fes:
                        fe.timing_enable(False)
            finally:
                if grp is not None:
                    grp.close()
            out = []
            for m, (fs, nb, _, _) in enumerate(members):
                if nb is None:
                    out.append((fes[m].chan_read_iq(direct), fes[m].chan_read_fm(direct, 1.0)))
                    continue
                bins = np.stack([fes[m].pfb_read_bin(k) for k in range(nb)])
                out.append((bins, [fes[m].chan_read_iq(c) for c in ids[m]], [fes[m].chan_read_fm(c, 1.0) for c in ids[m]]))
            return out, launches
        finally:
            for fe in fes:
                fe.close()

    alone, _ = drive(False)
    got, launches = drive(True)
    assert launches == expected, (launches, expected)
    for m, (fs, nb, opened, _) in enumerate(members):
        if nb is None:
            assert len(got[m][0]) == (sum(lens[m]) - 1) // 96 + 1
            np.testing.assert_array_equal(got[m][0], alone[m][0], err_msg="direct channel iq")
            np.testing.assert_array_equal(got[m][1], alone[m][1], err_msg="direct channel fm")
            continue
        D, start = nb // 2, int(edges[m][opened])
        total = (sum(lens[m]) - 1) // D + 1 - -(-start // D)
        assert got[m][0].shape == alone[m][0].shape == (nb, total), (m, got[m][0].shape, total)
        np.testing.assert_array_equal(got[m][0], alone[m][0], err_msg="member %d bins" % m)
        for j in range(len(got[m][1])):
            assert len(got[m][1][j]) == total
            np.testing.assert_array_equal(got[m][1][j], alone[m][1][j], err_msg="member %d tap %d iq" % (m, j))
            np.testing.assert_array_equal(got[m][2][j], alone[m][2][j], err_msg="member %d tap %d fm" % (m, j))
        # (what the bits are is held elsewhere; one bin per member all the same)
        xz = xs[m].copy()
        xz[:start] = 0
        want = G.xlating_fir_exact(xz, D, G.channel_params(fs, 12500)[1], _f_bin(3, nb, fs), fs)[-(-start // D):]
        assert rel_rms(got[m][0][3], want) < 1e-5, (m, rel_rms(got[m][0][3], want))


# ------------------------------------------------------------------ 4. fuzz over this family

def _stretch(taps, T):
    """any low-pass of exactly T taps (the comparison is against the same taps): the design stretched or squeezed"""
    return np.interp(np.linspace(0, len(taps) - 1, T), np.arange(len(taps)), taps).astype(np.float32)


@pytest.mark.parametrize("seed", _seeds())
def test_random_mixed_radix_shapes_prototypes_and_cuts(gpu_required, seed):
    """tests/test_gpu_fuzz.py::test_random_filterbank_shapes_and_cuts for this family: a random shape; the channel filter, a
    low-pass of NB / 2 < T <= NB taps (one per branch: the zero-padded row), of exactly NB + 1 or of exactly 2 NB taps; a
    random lead-in (possibly none), 40 to 200 frames, random cuts.  Three random bins against the float64 exact-phase
    channel (< 1e-5 on noise) and bit for bit against one push."""
    nat = gpu_required
    rng = np.random.default_rng(31000 + seed)
    fs, nb = SHAPES[int(rng.integers(0, len(SHAPES)))]
    D, chan = G.channel_params(fs, 12500)
    kind = int(rng.integers(0, 4))
    proto = [chan, _stretch(chan, int(rng.integers(nb // 2 + 1, nb + 1))), _stretch(chan, nb + 1), _stretch(chan, 2 * nb)][kind]
    assert nat.pfb_shape_family(nb, D, len(proto)) == 3, (nb, len(proto))
    n_frames = int(rng.integers(40, 201))
    lead = int(rng.integers(1, 3 * D)) if rng.random() < 0.5 else 0
    n = lead + D * n_frames + int(rng.integers(0, D))
    x = synth.awgn(rng, n)
    cuts = sorted({lead, n} | {int(v) for v in rng.integers(lead + 1, n, int(rng.integers(0, 8)))})
    ks = sorted({int(v) for v in rng.integers(0, nb, 3)})

    def run(pieces):
        with nat.Frontend(fs, block_capacity=n + 16, hist_capacity=1 << 14, out_capacity=1 << 10) as fe:
            if lead:
                fe.push(x[:lead])
            fe.pfb_open(nb, D, proto)
            for a, b in pieces:
                fe.push(x[a:b])
            return fe.pfb_produced(), [fe.pfb_read_bin(k) for k in ks]

    n_one, one = run([(lead, n)])
    n_cut, cut = run(list(zip(cuts[:-1], cuts[1:])))
    k0 = -(-lead // D)
    assert n_one == n_cut == (n - 1) // D + 1 - k0
    xz = x.copy()
    xz[:lead] = 0
    for k, a, b in zip(ks, one, cut):
        np.testing.assert_array_equal(a, b, err_msg="cut invariance, seed %d bins %d taps %d bin %d" % (seed, nb, len(proto), k))
        ref = G.xlating_fir_exact(xz, D, proto, _f_bin(k, nb, fs), fs)[k0:]
        assert len(a) == len(ref), (seed, nb, len(a), len(ref))
        assert rel_rms(a, ref) < 1e-5, (seed, nb, len(proto), k, rel_rms(a, ref))


@pytest.mark.parametrize("seed", _seeds())
def test_random_mixed_radix_tap_lifecycles(gpu_required, seed):
    """tests/test_gpu_fuzz.py::test_random_filterbank_tap_lifecycles for this family, on a 64- or 128-frame ring: taps opened
    and closed at random block boundaries -- whole aligned runs of 16 (read from the bank's ring) and scattered ones (tap
    matrix), idle, with GNU Radio's rotator, discriminator-only with flips -- everything read after every push.  An idle tap
    is its bin from its opening on, bit for bit, and its discriminator gr's quadrature_demod of that; a gr_phase tap is its
    bin times a rotator (_rotator_residual, the bounds of tests/test_gpu_pfbm.py); a discriminator-only tap gives the
    discriminator of an ordinary tap opened with it, to 1e-6, through every flip."""
    nat = gpu_required
    rng = np.random.default_rng(33000 + seed)
    fs, nb = SHAPES[int(rng.integers(0, len(SHAPES)))]
    D, taps = G.channel_params(fs, 12500)
    cap = int(rng.choice([64, 128]))
    sizes = []
    while len(sizes) < 6 or sum(sizes) < (2 * cap + 10) * D:         # the ring wraps twice at least
        sizes.append(int(rng.integers(1, 2 * D)) if rng.random() < 0.25 else int(rng.integers(2 * D, 30 * D)))
    n_blocks = len(sizes)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    x = synth.awgn(rng, int(cuts[-1]))
    plan = []                                    # per block: (kind, bins) drawn up front, so the tapped bins are followed from frame 0
    for b in range(n_blocks):
        opens = []
        for _ in range(int(rng.integers(0, 4)) if b else 3):
            u = rng.random()
            if u < 0.3:
                lo = 16 * int(rng.integers(0, nb // 16))     # a whole aligned run of 16
                opens.append(("idle", list(range(lo, lo + 16))))
            elif u < 0.5:
                opens.append(("idle", [int(v) for v in rng.integers(0, nb, int(rng.integers(1, 6)))]))
            elif u < 0.75:
                opens.append(("gr", [int(v) for v in rng.integers(0, nb, int(rng.integers(1, 4)))]))
            else:
                opens.append(("only", [int(v) for v in rng.integers(0, nb, int(rng.integers(1, 3)))]))
        plan.append(opens)
    ever = sorted({k for opens in plan for _, bins in opens for k in bins})
    ring = {k: [] for k in ever}
    lives = []
    with nat.Frontend(fs, block_capacity=int(max(sizes)) + 16, hist_capacity=1 << 14, out_capacity=cap) as fe:
        fe.pfb_open(nb, D, taps)
        live = []
        for b in range(n_blocks):
            produced = fe.pfb_produced()
            for kind, bins in plan[b]:
                for k in bins:
                    gr = kind == "gr" or (kind == "only" and bool(rng.integers(0, 2)))
                    L = dict(id=fe.pfb_tap_open(k, gr_phase=gr), bin=k, kind=kind, first=produced, iq=[], fm=[], flips=0)
                    if kind == "only":                       # the ordinary tap it is held against, and the tap that is flipped
                        L["twin"] = fe.pfb_tap_open(k, gr_phase=gr)
                        L["on"] = bool(rng.integers(0, 2))
                        L["twin_fm"] = []
                        fe.chan_set_fm_only(L["twin"], L["on"])
                    live.append(L)
            for L in list(live):
                if L["kind"] == "only" and rng.random() < 0.35:
                    L["on"] = not L["on"]
                    L["flips"] += 1
                    fe.chan_set_fm_only(L["twin"], L["on"])
                elif rng.random() < 0.08:                    # (everything was read after the last push)
                    fe.chan_close(L["id"])
                    if L["kind"] == "only":
                        fe.chan_close(L["twin"])
                    L["last"] = produced
                    live.remove(L)
                    lives.append(L)
            fe.push(x[int(cuts[b]):int(cuts[b + 1])])
            for k in ever:
                ring[k].append(fe.pfb_read_bin(k))
            for L in live:
                L["iq"].append(fe.chan_read_iq(L["id"]))
                L["fm"].append(fe.chan_read_fm(L["id"], 1.0))
                if L["kind"] == "only":
                    L["twin_fm"].append(fe.chan_read_fm(L["twin"], 1.0))
                    if L["on"]:
                        with pytest.raises(nat.RcfError):
                            fe.chan_read_iq(L["twin"])
        n_out = fe.pfb_produced()
        for L in live:
            L["last"] = n_out
            lives.append(L)
    assert n_out == (len(x) - 1) // D + 1 and n_out > 2 * cap
    assert lives
    full = {k: np.concatenate(ring[k]) for k in ever}
    for L in lives:
        y = np.concatenate(L["iq"]) if L["iq"] else np.zeros(0, np.complex64)
        fm = np.concatenate(L["fm"]) if L["fm"] else np.zeros(0, np.float32)
        assert len(full[L["bin"]]) == n_out
        want = full[L["bin"]][L["first"]:L["last"]]
        what = (seed, nb, L["kind"], L["bin"], L["first"], L["last"])
        assert len(y) == len(fm) == len(want), what + (len(y), len(want))
        if L["kind"] == "idle":
            np.testing.assert_array_equal(y, want, err_msg=str(what))
            if len(want):
                np.testing.assert_array_equal(fm, G.quadrature_demod_cf(want, 1.0), err_msg="fm " + str(what))
        elif L["kind"] == "gr" and len(want) >= 32:
            dphi, dmag = _rotator_residual(y, want)
            assert dphi < 2e-5 and dmag < 1e-4, what + (dphi, dmag)
        if L["kind"] == "only":
            f2 = np.concatenate(L["twin_fm"]) if L["twin_fm"] else np.zeros(0, np.float32)
            assert len(f2) == len(fm), what
            if len(fm):
                assert np.max(np.abs(f2 - fm)) <= 1e-6, what + (L["flips"], float(np.max(np.abs(f2 - fm))))
    for k in ever[:2]:                            # and the bins themselves, through all the wraps, against the exact-phase channel
        ref = G.xlating_fir_exact(x, D, taps, _f_bin(k, nb, fs), fs)
        assert rel_rms(full[k], ref) < 1e-5, (seed, nb, k, rel_rms(full[k], ref))


@pytest.mark.parametrize("seed", _seeds())
def test_random_structural_churn_at_2p4_msps(gpu_required, seed):
    """tests/test_gpu_fuzz.py::test_random_structural_churn with this family in the draw: at 2.4 Msps the filterbank is closed
    and opened again in mid-stream among 192 bins (the channel filter), 160 bins (a generic low-pass), 64 and 128 bins; its
    taps and stage-2 channels go with it, ids of the dead answer ENOCHAN and nothing else.  A direct keeper channel equals
    the oracle over the whole stream (< 2e-5), the last bank's bin the exact-phase channel with zero history from the sample
    the bank was opened at (< 3e-5)."""
    nat = gpu_required
    rng = np.random.default_rng(35000 + seed)
    fs, cr = 2.4e6, 12500
    D, taps = G.channel_params(fs, cr)                       # 96 / 349
    shapes = [(192, 96), (160, 80), (64, 64), (128, 64)]

    def proto_of(nb, Db):
        if nb == 192:
            return taps
        if nb == 160:
            p = G.low_pass_2(1.0, fs, 6250.0, 7500.0, 20.0, G.WIN_HAMMING)
            assert nb < len(p) <= 2 * nb
            return p
        return G.low_pass_2(1.0, fs, fs / nb * 0.4, fs / nb * 0.2, 60.0, G.WIN_BLACKMAN_HARRIS)

    for nb, Db in shapes[:2]:
        assert nat.pfb_shape_family(nb, Db, len(proto_of(nb, Db))) == 3
    n_blocks = int(rng.integers(8, 18))
    sizes = [int(rng.integers(1, 2 * D)) if rng.random() < 0.2 else int(rng.integers(1500, 60 * D)) for _ in range(n_blocks)]
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    x = synth.awgn(rng, int(cuts[-1]))
    f_keep = 312500.0
    x = (x + 0.5 * np.exp(2j * np.pi * (f_keep + 200.0) * np.arange(len(x)) / fs)).astype(np.complex64)
    kept = []
    bank = None
    dead = []
    with nat.Frontend(fs, block_capacity=int(max(sizes)) + 16, hist_capacity=1 << 14, out_capacity=1 << 10) as fe:
        keeper = fe.chan_open(cr, f_keep)
        on_bank = []
        for b in range(n_blocks):
            s0 = int(cuts[b])
            for _ in range(int(rng.integers(0, 4))):
                u = rng.random()
                try:
                    if u < 0.3:
                        if bank is not None:
                            fe.pfb_close()
                            bank = None
                            dead += on_bank
                            on_bank = []
                        nb, Db = shapes[int(rng.integers(0, len(shapes)))]
                        if nat.pfb_shape_supported(nb, Db, len(proto_of(nb, Db))):
                            fe.pfb_open(nb, Db, proto_of(nb, Db))
                            bank = dict(nb=nb, Db=Db, proto=proto_of(nb, Db), at=s0, bin=int(rng.integers(0, nb)), reads=[])
                    elif u < 0.4 and bank is not None:
                        fe.pfb_close()
                        bank = None
                        dead += on_bank
                        on_bank = []
                    elif u < 0.8 and bank is not None:
                        k = int(rng.integers(0, bank["nb"]))
                        on_bank.append(fe.pfb_tap_open(k, gr_phase=bool(rng.integers(0, 2))) if rng.random() < 0.5
                                       else fe.pfb_chan_open(k, cr, 0.0))
                    elif u < 0.9 and on_bank:
                        cid = on_bank[int(rng.integers(len(on_bank)))]
                        fe.chan_read_iq(cid)
                        fe.chan_read_fm(cid, 1.0)
                    elif dead:
                        with pytest.raises(nat.RcfError) as ei:
                            fe.chan_read_iq(dead[int(rng.integers(len(dead)))])
                        assert ei.value.code == nat.RCF_ENOCHAN, (seed, str(ei.value))
                except nat.RcfError as e:
                    assert e.code in (nat.RCF_ENOCHAN, nat.RCF_ECAP, nat.RCF_EINVAL, nat.RCF_ERANGE), (seed, str(e))
            fe.push(x[s0:int(cuts[b + 1])])
            kept.append(fe.chan_read_iq(keeper))
            if bank is not None:
                bank["reads"].append(fe.pfb_read_bin(bank["bin"]))
    y = np.concatenate(kept)
    yo = _oracle_life(x, fs, cr, [(0, f_keep)], 0, len(x))
    assert len(y) == len(yo) and rel_rms(y, yo) < 2e-5, (seed, rel_rms(y, yo))
    if bank is not None and bank["reads"]:
        got = np.concatenate(bank["reads"])
        xz = x.copy()
        xz[:bank["at"]] = 0
        k, nb, Db = bank["bin"], bank["nb"], bank["Db"]
        ref = G.xlating_fir_exact(xz, Db, bank["proto"], _f_bin(k, nb, fs), fs).astype(np.complex64)[-(-bank["at"] // Db):]
        assert len(got) == len(ref), (seed, nb, Db, len(got), len(ref))
        if len(ref) > 4:
            assert rel_rms(got, ref) < 3e-5, (seed, nb, Db, k, rel_rms(got, ref))


# ------------------------------------------------------------------ 5. buffer and prototype limits (192 bins)

def _ragged_bins(nat, x, proto, cuts, **caps):
    fs, nb = 2.4e6, 192
    with nat.Frontend(fs, **caps) as fe:
        fe.pfb_open(nb, nb // 2, proto)
        for a, b in zip(cuts[:-1], cuts[1:]):
            fe.push(x[a:b])
        return fe.pfb_produced(), np.stack([fe.pfb_read_bin(k) for k in range(nb)])


def test_minimum_history_with_a_one_tap_per_branch_prototype(gpu_required):
    """rcf_pfb_open accepts hist_capacity >= P NB + D with the prototype's own P; the kernel always reads the
    two-taps-per-branch window, 2 NB - 1 samples back.  With one tap per branch and hist_capacity = NB + D exactly (288: the
    constructor takes any value; 287 is refused) the window's oldest samples lie before the wideband buffer: the
    descriptor returns zeros for them and they meet the zero tap row.  Every bin bit for bit what hist_capacity = 2^14
    gives, over ragged pushes, and the exact-phase channel of that prototype."""
    nat = gpu_required
    fs, nb = 2.4e6, 192
    D = nb // 2
    proto = G.low_pass_2(1.0, fs, 6250.0, 12500.0, 20.0, G.WIN_HAMMING)
    assert nb // 2 < len(proto) <= nb
    rng = np.random.default_rng(8800)
    x = synth.awgn(rng, D * 200 + 29)
    cuts = [0, 1, D, D + 7, 3 * D - 1, 16 * D + 5, 16 * D + 6, 50 * D + 40, 130 * D, len(x)]
    blk = max(b - a for a, b in zip(cuts[:-1], cuts[1:]))
    with nat.Frontend(fs, block_capacity=blk, hist_capacity=nb + D - 1, out_capacity=1 << 10) as fe:
        with pytest.raises(nat.RcfError) as ei:
            fe.pfb_open(nb, D, proto)
        assert ei.value.code == nat.RCF_ECAP
    n_min, b_min = _ragged_bins(nat, x, proto, cuts, block_capacity=blk, hist_capacity=nb + D, out_capacity=1 << 10)
    n_big, b_big = _ragged_bins(nat, x, proto, cuts, block_capacity=blk, hist_capacity=1 << 14, out_capacity=1 << 10)
    assert n_min == n_big == 201
    np.testing.assert_array_equal(b_min, b_big)
    for k in (0, 5, 97, 191):
        ref = G.xlating_fir_exact(x, D, proto, _f_bin(k, nb, fs), fs)
        assert rel_rms(b_min[k], ref) < 1e-5, (k, rel_rms(b_min[k], ref))


def test_pushes_of_exactly_block_capacity(gpu_required):
    """two pushes of exactly block_capacity samples, the block no multiple of a chunk (16 frames of 96 samples) nor of D: the
    window of the last, partial chunk ends where the wideband buffer's descriptor ends.  Every bin bit for bit what a
    front-end with four times the block capacity gives on the same pushes, and the exact-phase channel."""
    nat = gpu_required
    fs, nb = 2.4e6, 192
    D, taps = G.channel_params(fs, 12500)
    blk = CHUNK[nb] * D * 5 + D * 3 + 41
    assert blk % (CHUNK[nb] * D) and blk % D
    rng = np.random.default_rng(8900)
    x = synth.awgn(rng, 2 * blk)
    cuts = [0, blk, 2 * blk]
    n_a, a = _ragged_bins(nat, x, taps, cuts, block_capacity=blk, hist_capacity=1 << 12, out_capacity=1 << 10)
    n_b, b = _ragged_bins(nat, x, taps, cuts, block_capacity=4 * blk, hist_capacity=1 << 12, out_capacity=1 << 10)
    assert n_a == n_b == (2 * blk - 1) // D + 1
    np.testing.assert_array_equal(a, b)
    with nat.Frontend(fs, block_capacity=blk, hist_capacity=1 << 12, out_capacity=1 << 10) as fe:
        fe.pfb_open(nb, D, taps)
        with pytest.raises(nat.RcfError):                     # one sample more is refused, and nothing is lost by it
            fe.push(x[:blk + 1])
        fe.push(x[:blk])
        assert fe.pfb_produced() == (blk - 1) // D + 1
    for k in (0, 7, 96, 190):
        ref = G.xlating_fir_exact(x, D, taps, _f_bin(k, nb, fs), fs)
        assert rel_rms(a[k], ref) < 1e-5, (k, rel_rms(a[k], ref))


def test_stage2_lag_changes_nothing_on_a_192_bin_bank(gpu_required):
    """rcf_set_stage2_lag applies to the 256-bin kernel only: a 192-bin bank with stage-2 channels gives the same bits with
    the lag on and off (tests/test_gpu_lag.py holds the 256-bin side)"""
    nat = gpu_required
    fs, nb = 2.4e6, 192
    D, taps = G.channel_params(fs, 12500)
    rng = np.random.default_rng(8950)
    blk = D * 120
    x = synth.awgn(rng, 5 * blk)
    cuts = [blk, blk // 2 + 48, blk, 300, blk - 96]

    def run(lag):
        out = []
        with nat.Frontend(fs, 0.0, device=0, block_capacity=blk, hist_capacity=1 << 14, out_capacity=1 << 10) as fe:
            fe.set_stage2_lag(lag)
            fe.pfb_open(nb, D, taps)
            ids = [fe.pfb_chan_open((5 + 17 * i) % nb, 12500, 3125.0 * ((i % 5) - 2)) for i in range(7)]
            at = 0
            for step, n in enumerate(cuts):
                if step == 2:
                    out.append(fe.chan_read_fm(ids[0], 5.0))
                if step == 3:
                    fe.chan_set_offset(ids[3], 6250.0)
                fe.push(x[at:at + n])
                at += n
            for c in ids:
                out += [fe.chan_read_iq(c), fe.chan_read_fm(c, 5.0)]
            out.append(fe.pfb_read_bin(5))
        return out

    on, off = run(True), run(False)
    assert len(on) == len(off) == 16
    for a, b in zip(on, off):
        assert len(a) > 0
        np.testing.assert_array_equal(a, b)
