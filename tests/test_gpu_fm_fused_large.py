"""The fused discriminator (rcf_pfb_fm_enable) at launch sizes the production shapes use: thousands of chunks per launch, more
than the chip holds at once, and more than the hand-over ring of the look-back form (pfb5_fmlb_kernel) once had rows for
(4096).  Chunk c of a launch takes the frame before its first one from the row chunk c - 1's workgroup published; a row
shared by two chunks of one launch hands a wrong predecessor to frame 0 of a chunk -- one sample in every F = 16 / (NB / 400)
of every bin.  So every test compares whole streams of bins that cover every wave of the workgroup (the hand-over is wave
to wave) against references without a hand-over: the span form (RCF_PFB5_FM_LOOKBACK=0, a child process) and
discriminator-only taps (tap_finalize)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from oracle import cbind as OC, grspec as G

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _shape(fs, os_):
    D, taps = G.channel_params(fs, 12500)
    nb = os_ * D
    if os_ == 4:
        taps = taps[:nb]                                           # one tap per branch (the kernel instantiated for OS = 4)
    return D, nb, np.asarray(taps, dtype=np.float32), 16 // (nb // 400)


def _signal(seed, fs, n, nb, carriers):
    """unit noise + strong FM carriers on bin centres (float32 phases are enough here: this is a stimulus, not a reference)"""
    rng = np.random.default_rng(seed)
    x = np.empty(n, dtype=np.complex64)
    x.real = rng.standard_normal(n, dtype=np.float32) * np.float32(np.sqrt(0.5))
    x.imag = rng.standard_normal(n, dtype=np.float32) * np.float32(np.sqrt(0.5))
    t = np.arange(n, dtype=np.float64) / fs
    for i, k in enumerate(carriers):
        f0 = (k if k < nb // 2 else k - nb) * fs / nb
        ph = 2 * np.pi * (f0 * t + (0.2 + 0.05 * i) * np.sin(2 * np.pi * (500 + 130 * i) * t))
        x += (6.0 * np.exp(1j * ph)).astype(np.complex64)
    return x


def _wave_bins(nb):
    """one bin in every (wave, pass) position of the 320-thread workgroup -- thread t handles bins t + 320 bb, wave t // 64 --
    plus the edges of the bin range"""
    out = {0, 1, nb // 2, nb - 1}
    for bb in range((nb + 319) // 320):
        for w in range(5):
            lo = 320 * bb + 64 * w
            if lo < nb:
                out.add(min(nb - 1, lo + (13 * w + 29 * bb) % 64))
    return sorted(out)


def _cuts(D, F, n_chunks, partial):
    """a small launch (the stream's start), ONE launch of n_chunks chunks (its last one a single frame if `partial`), a
    small launch after it"""
    big = (n_chunks * F - ((F - 1) if partial else 0)) * D
    return [D * F * 5 + 3, big, D * F * 3 + 11], big // D


def _caps(D, cuts, frames):
    out_cap = 1 << int(np.ceil(np.log2(frames + 64)))
    return dict(block_capacity=max(cuts), hist_capacity=1 << 15, out_capacity=out_cap)


def _fused(nat, fs, nb, D, taps, x, cuts, bins, caps, mode=2):
    with nat.Frontend(fs, 0.0, device=0, **caps) as fe:
        fe.pfb_open(nb, D, taps)
        fe.pfb_fm_enable(mode, gr_phase=True)
        got = [[] for _ in bins]
        at = 0
        for n in cuts:
            fe.push(x[at:at + n])
            at += n
            for i, b in enumerate(bins):
                got[i].append(fe.pfb_read_fm(b, 1.0))
        lost = fe.pfb_fm_lost()
    return [np.concatenate(g) for g in got], lost


def _fm_only_taps(nat, fs, nb, D, taps, x, cuts, bins, caps):
    with nat.Frontend(fs, 0.0, device=0, **caps) as fe:
        fe.pfb_open(nb, D, taps)
        ids = [fe.pfb_tap_open(b, gr_phase=True) for b in bins]
        for c in ids:
            fe.chan_set_fm_only(c, True)
        got = [[] for _ in ids]
        at = 0
        for n in cuts:
            fe.push(x[at:at + n])
            at += n
            for i, c in enumerate(ids):
                got[i].append(fe.chan_read_fm(c, 1.0))
    return [np.concatenate(g) for g in got]


_SPAN_CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    sys.path[:0] = [%r, %r]
    from rcf import native as nat
    a = json.loads(sys.argv[1])
    x = np.load(a["x"], mmap_mode="r")
    taps = np.asarray(a["taps"], dtype=np.float32)
    with nat.Frontend(a["fs"], 0.0, device=0, **a["caps"]) as fe:
        fe.pfb_open(a["nb"], a["D"], taps)
        fe.pfb_fm_enable(2, gr_phase=True)
        got = {b: [] for b in a["bins"]}
        at = 0
        for n in a["cuts"]:
            fe.push(np.ascontiguousarray(x[at:at + n]))
            at += n
            for b in a["bins"]:
                got[b].append(fe.pfb_read_fm(b, 1.0))
    np.savez(a["out"], **{"b%%d" %% b: np.concatenate(v) for b, v in got.items()})
""") % (ROOT, os.path.join(ROOT, "radiocapture-rf_amd"))


def _span_form(tmp_path, fs, nb, D, taps, x, cuts, bins, caps):
    """the same stream through the span form of the kernel (no hand-over between workgroups), in a child process: the
    form is chosen once per process (RCF_PFB5_FM_LOOKBACK)"""
    import json
    xf, of = str(tmp_path / "x.npy"), str(tmp_path / "span.npz")
    np.save(xf, x)
    env = dict(os.environ)
    env.pop("RCF_PFB5_FM_SPAN", None)
    env["RCF_PFB5_FM_LOOKBACK"] = "0"
    arg = json.dumps(dict(x=xf, out=of, fs=fs, nb=nb, D=D, taps=[float(t) for t in taps], cuts=[int(c) for c in cuts],
                          bins=[int(b) for b in bins], caps=caps))
    r = subprocess.run([sys.executable, "-c", _SPAN_CHILD, arg], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(of)
    return [z["b%d" % b] for b in bins]


def _first_bad(a, b, frame0):
    """where two streams of one bin differ: (first index, on frame 0 of a chunk?, differences on frames 0, differences)"""
    bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
    return (int(bad[0]), bool(frame0[bad[0]]), int(np.count_nonzero(frame0[bad])), len(bad)) if len(bad) else None


def _frame0_mask(cuts, D, F, n_total):
    """True at the frames that are frame 0 of a chunk of their launch (the frames whose predecessor was handed over)"""
    mask = np.zeros(n_total, dtype=bool)
    s0 = 0
    s = 0
    for n in cuts:
        s += n
        s1 = min(n_total, (s - 1) // D + 1)                        # frames produced once the stream holds s samples
        mask[s0:s1:F] = True
        s0 = s1
    return mask


# every count on some shape, every shape with a count above the old ring of 4096 rows: its edges (4095 / 4096 / 4097), the
# closest aliasing the old ring allowed (4681: one block apart, 8192: four), and a 2^25-sample block (10486 / 20972 chunks)
LARGE = [
    # fs, OS, chunks per launch
    (5e6, 2, 4095),
    (5e6, 2, 4681),
    (10e6, 2, 4096),
    (10e6, 2, 10486),
    (20e6, 2, 4097),
    (20e6, 2, 8192),
    (20e6, 4, 4681),
    (20e6, 4, 20972),
]


@pytest.mark.parametrize("fs,os_,n_chunks", LARGE, ids=["%dbins-%dchunks" % (os_ * fs / 25000, n) for fs, os_, n in LARGE])
def test_large_launch_has_the_bits_of_the_span_form_and_of_taps(gpu_required, tmp_path, fs, os_, n_chunks):
    nat = gpu_required
    D, nb, taps, F = _shape(fs, os_)
    cuts, frames = _cuts(D, F, n_chunks, partial=n_chunks % 2 == 1)
    caps = _caps(D, cuts, frames)
    bins = _wave_bins(nb)
    x = _signal(n_chunks * 10 + os_, fs, sum(cuts), nb, [bins[3], bins[-3]])
    got, lost = _fused(nat, fs, nb, D, taps, x, cuts, bins, caps)
    assert lost == 0                                               # every hand-over arrived
    n_total = len(got[0])
    assert n_total >= frames + F * 8 and all(len(g) == n_total for g in got)
    frame0 = _frame0_mask(cuts, D, F, n_total)
    assert int(np.count_nonzero(frame0[F * 5 + 1:F * 5 + 1 + frames])) == n_chunks
    span = _span_form(tmp_path, fs, nb, D, taps, x, cuts, bins, caps)
    tap = _fm_only_taps(nat, fs, nb, D, taps, x, cuts, bins, caps)
    for b, g, s, t in zip(bins, got, span, tap):
        assert _same_bits(g, s), ("span form", b, _first_bad(g, s, frame0))
        assert _same_bits(g, t), ("discriminator-only tap", b, _first_bad(g, t, frame0))


def test_large_launch_within_per_sample_budget_of_the_gr_faithful_oracle(gpu_required):
    """1600 bins, one launch of 8192 chunks: carrier bins against the GNU-Radio-faithful oracle sample by sample -- a wrong
    predecessor is an error of order 1 rad in one sample of every 4, which an RMS over the stream would hide.  Frame 0 of
    every chunk (the handed-over predecessor) and the other frames are bounded separately."""
    nat = gpu_required
    fs = 20e6
    D, nb, taps, F = _shape(fs, 2)
    cuts, frames = _cuts(D, F, 8192, partial=False)
    caps = _caps(D, cuts, frames)
    carriers = [7, 333, 801, nb - 12]
    x = _signal(8192, fs, sum(cuts), nb, carriers)
    got, lost = _fused(nat, fs, nb, D, taps, x, cuts, carriers, caps)
    assert lost == 0
    frame0 = _frame0_mask(cuts, D, F, len(got[0]))
    worst = []
    for k, g in zip(carriers, got):
        f0 = (k if k < nb // 2 else k - nb) * fs / nb
        ct, incr = OC.xlating_composite(taps, D, f0, fs)
        _, fo = OC.channel_bank(x, D, ct[None, :], np.array([incr]), gains=[1.0])
        n = min(len(g), len(fo[0]))
        assert n >= frames
        d = np.abs(np.angle(np.exp(1j * (g[:n].astype(np.float64) - fo[0][:n]))))
        d[:2] = 0.0                                                # (the stream's first two samples: zero history)
        e0, e1 = float(np.max(d[frame0[:n]])), float(np.max(d[~frame0[:n]]))
        worst.append((k, e0, e1))
    print("per-sample error vs the oracle (bin, frame 0 of a chunk, other frames): %s" % worst)
    # Measured on an MI355X (worst |error| in rad, frame 0 of a chunk / the other frames): bin 7 2.4e-7 / 2.6e-7, bin 333
    # 1.9e-6 / 3.1e-5, bin 801 2.9e-6 / 4.5e-5, bin 1588 2.7e-7 / 3.0e-7.  The bound is ten times the worst of them; a
    # wrong predecessor frame is an error of order 1 rad.
    for k, e0, e1 in worst:
        assert e0 < 5e-4, ("frame 0 of a chunk", k, e0)
        assert e1 < 5e-4, ("frames 1 .. F - 1", k, e1)


def test_large_grouped_launch_has_the_bits_of_one_by_one(gpu_required):
    """three 3200-bin OS 4 banks in one grouped launch (pfb5_fmlb_group_kernel) of 8192 chunks per member, then a ragged
    round: the bits of the members pushed one by one, no hand-over lost in any member"""
    nat = gpu_required
    fs = 20e6
    D, nb, taps, F = _shape(fs, 4)
    G_ = 3
    rounds = [[D * 200 + 3, D * 300 + 1, D * 250], [8192 * F * D] * G_, [(4097 * F - 1) * D, D * 50 + 7, 8192 * F * D]]
    n_m = [sum(r[m] for r in rounds) for m in range(G_)]
    bins = _wave_bins(nb)
    xs = [_signal(77 + m, fs, n_m[m], nb, [bins[5 + m], bins[-4 - m]]) for m in range(G_)]
    caps = dict(block_capacity=8192 * F * D, hist_capacity=1 << 15, out_capacity=1 << 15)
    out = {}
    for which in ("grouped", "one by one"):
        fes = []
        for m in range(G_):
            fe = nat.Frontend(fs, 0.0, device=0, **caps)
            fe.pfb_open(nb, D, taps)
            fe.pfb_fm_enable(2, gr_phase=True)
            fes.append(fe)
        grp = nat.Group(fes) if which == "grouped" else None
        at = [0] * G_
        got = [[[] for _ in bins] for _ in range(G_)]
        for r in rounds:
            blocks = [xs[m][at[m]:at[m] + r[m]] for m in range(G_)]
            for m in range(G_):
                at[m] += r[m]
            if grp is not None:
                grp.push(blocks, nat.FMT_CF32)
            else:
                for m in range(G_):
                    fes[m].push(blocks[m])
            for m in range(G_):
                for i, b in enumerate(bins):
                    got[m][i].append(fes[m].pfb_read_fm(b, 1.0))
        lost = [fe.pfb_fm_lost() for fe in fes]
        if grp is not None:
            grp.close()
        for fe in fes:
            fe.close()
        assert lost == [0] * G_, (which, lost)
        out[which] = [[np.concatenate(g_) for g_ in gm] for gm in got]
    for m in range(G_):
        for i, b in enumerate(bins):
            a_, o_ = out["grouped"][m][i], out["one by one"][m][i]
            assert len(a_) == len(o_) >= 8192 * F, (m, b, len(a_), len(o_))
            assert _same_bits(a_, o_), (m, b, int(np.argmax(a_.view(np.uint32) != o_.view(np.uint32))))


@pytest.mark.parametrize("fs,os_", [(5e6, 2), (10e6, 2), (20e6, 2), (20e6, 4)])
def test_largest_launch_a_handle_accepts_is_one_row_per_chunk(gpu_required, fs, os_):
    """a launch of out_capacity frames -- the most a handle accepts without stage-2 channels -- has out_capacity / F chunks,
    8192 here: the hand-over ring holds a row for every one of them (no RcfError), and the bits are the taps'; one frame
    more is refused by the ring's own capacity check"""
    nat = gpu_required
    D, nb, taps, F = _shape(fs, os_)
    out_cap = 8192 * F
    cuts = [D * F * 4 + 5, out_cap * D, D * 7]
    caps = dict(block_capacity=(out_cap + 1) * D, hist_capacity=1 << 15, out_capacity=out_cap)
    bins = _wave_bins(nb)[::3]
    x = _signal(os_ * 100 + int(fs / 1e6), fs, sum(cuts), nb, [bins[1]])
    got, lost = _fused(nat, fs, nb, D, taps, x, cuts, bins, caps)
    assert lost == 0
    tap = _fm_only_taps(nat, fs, nb, D, taps, x, cuts, bins, dict(caps, out_capacity=2 * out_cap))
    for b, g, t in zip(bins, got, tap):
        assert len(g) >= out_cap and _same_bits(g, t), (b, len(g), len(t))
    with nat.Frontend(fs, 0.0, device=0, **caps) as fe:
        fe.pfb_open(nb, D, taps)
        fe.pfb_fm_enable(2, gr_phase=True)
        fe.push(x[:cuts[0]])
        with pytest.raises(nat.RcfError) as ei:
            fe.push(x[cuts[0]:cuts[0] + (out_cap + 1) * D])
        assert ei.value.code == nat.RCF_ECAP
