"""The zero-history boundary of every filterbank kernel form.  A launch whose first frame still reaches samples before the
bank's opening sample runs the masking instantiation; the planner decides that with ONE predicate
(radiocapture-rf_amd/csrc/pfb_shape.h: pfb_zero_history) and the launchers take its word:

    (n_lo - halo - OS (Ppad - 1)) D - (NB - 1) < start_sample        halo = 0, or one chunk for the fused discriminator

Every bank here is opened in mid-stream at a sample that is no multiple of D, and the pushes are cut so that consecutive
launches begin one frame before, exactly at and one frame after the first frame for which the predicate is false (for the
fused discriminator at both boundaries, halo = 0 and halo = one chunk).  A decision that is off by one frame either way
gives wrong samples at the stream's start (steady-state kernel too early: it reads what was pushed before the bank was
opened) or is caught by the cut-invariance below where the two instantiations differ.

Asserted per form: every bin (and discriminator sample) is bit for bit what the same stream gives in ONE push -- every
form is cut-invariant to the bit (tests/test_gpu_fuzz.py::test_random_filterbank_shapes_and_cuts, tests/test_gpu_pfbm.py and
tests/test_gpu_fm_fused.py hold that under other cuts) -- and equals the oracle at the project's bars: IQ <= 1e-5 relative rms per bin against the exact-phase channel on the stream zeroed before the opening sample, the
discriminator <= 1e-4 rms against the GNU-Radio-faithful oracle channel on FM carriers.  rcf_pfb_fm_lost is 0."""
import numpy as np
import pytest

from oracle import cbind as OC
from oracle import grspec as G
from rcf import synth

from test_gpu_fm_fused import _signal
from test_gpu_pfbm import _exact_all_bins, rel_rms

pytestmark = pytest.mark.gpu

FRAMES = 64


def _sinc_proto(nb, P):
    """a Hamming-windowed sinc of P taps per branch less three (the last polyphase row is part zeros): the kernel
    instantiated for P rows runs it as it is"""
    n = P * nb - 3
    i = np.arange(n) - (n - 1) / 2.0
    return (np.sinc(i / nb) * np.hamming(n) / nb).astype(np.float32)


def _ref_proto(fs):
    D, proto = G.channel_params(fs, 12500)
    return D, np.asarray(proto, dtype=np.float32)


# name -> (fs, bins, D, prototype, rows the kernel reads (Ppad), frames per chunk)
def _shape(name):
    if name == "plain-256":
        return 256 * 12500.0, 256, 256, _sinc_proto(256, 14), 14, 16
    if name == "two-branch-512":
        return 512 * 12500.0, 512, 512, _sinc_proto(512, 4), 4, 16
    if name == "persistent-512":
        return 256 * 12500.0, 512, 256, _sinc_proto(512, 4), 4, 16
    if name == "pfb5-1600":
        D, proto = _ref_proto(20e6)
        return 20e6, 1600, D, proto, 2, 4
    if name == "pfbm-192":
        D, proto = _ref_proto(2.4e6)
        return 2.4e6, 192, D, proto, 2, 16
    raise KeyError(name)


def _first_steady_frame(nb, D, ppad, start, halo):
    """the first absolute frame index n_lo for which the predicate above is false"""
    os_ = nb // D
    n = -(-(start + nb - 1) // D) + halo + os_ * (ppad - 1)
    assert (n - halo - os_ * (ppad - 1)) * D - (nb - 1) >= start > (n - 1 - halo - os_ * (ppad - 1)) * D - (nb - 1)
    return n


_streams = {}


def _stream(name, seed=0):
    """noise + three tones 12 dB over a bin's noise (a float32 transform's rounding is relative to the strongest bin that
    shares a butterfly, and the bar below is relative per bin: tests/test_gpu_pfbm.py), a lead-in (no multiple of D) before
    the bank is opened, 64 frames plus the prototype's reach after it; the exact-phase bins of the zeroed stream"""
    key = (name, seed)
    if key in _streams:
        return _streams[key]
    fs, nb, D, proto, ppad, F = _shape(name)
    rng = np.random.default_rng(8100 + nb + D + seed)
    lead = D + int(rng.integers(1, D))
    assert lead % D
    n = lead + (FRAMES + -(-len(proto) // D)) * D
    x = synth.awgn(rng, n).astype(np.complex128)
    t = np.arange(n) / fs
    floor = float(np.sqrt(np.sum(proto.astype(np.float64) ** 2)))
    for f in (7 * fs / nb, -20.37 * fs / nb, -(nb // 2 - 1) * fs / nb):
        x += 4.0 * floor * np.exp(2j * np.pi * f * t)
    x = x.astype(np.complex64)
    xz = x.copy()
    xz[:lead] = 0
    k0 = -(-lead // D)
    ref = _exact_all_bins(xz, D, proto, nb, fs)[:, k0:]
    _streams[key] = (x, lead, ref)
    return _streams[key]


def _cuts(name, lead, n, halos):
    """a launch begins at frame m when its push begins at a sample in ((m - 1) D, m D]: pushes that begin at
    m D - D // 3 for m = one before, at and one after each boundary"""
    fs, nb, D, proto, ppad, F = _shape(name)
    frames = sorted({_first_steady_frame(nb, D, ppad, lead, h) + d for h in halos for d in (-1, 0, 1)})
    cuts = [lead] + [m * D - D // 3 for m in frames] + [n]
    assert all(a < b for a, b in zip(cuts[:-1], cuts[1:])), cuts
    return cuts


def _run(nat, name, cuts, fm_mode=0, fm_bins=(), x=None):
    """x: another stream of the same length and lead-in (the discriminator's carriers); its bins are not read"""
    fs, nb, D, proto, ppad, F = _shape(name)
    other = x is not None
    xa, lead, _ = _stream(name)
    x = x if other else xa
    assert len(x) == len(xa)
    with nat.Frontend(fs, 0.0, device=0, block_capacity=len(x), hist_capacity=1 << 15, out_capacity=1 << 10) as fe:
        fe.push(x[:lead])
        fe.pfb_open(nb, D, proto)
        if fm_mode:
            fe.pfb_fm_enable(fm_mode, gr_phase=True)
        for a, b in zip(cuts[:-1], cuts[1:]):
            fe.push(x[a:b])
        produced = fe.pfb_produced()
        bins = None if fm_mode == 2 or other else np.stack([fe.pfb_read_bin(k) for k in range(nb)])
        fm = np.stack([fe.pfb_read_fm(k, 1.0) for k in fm_bins]) if fm_mode else None
        if fm_mode:
            assert fe.pfb_fm_lost() == 0
    return produced, bins, fm


def _check_bins(name, one, cut, ref):
    diff = float(np.max(np.abs(one - cut)))
    errs = np.array([rel_rms(cut[k], ref[k]) for k in range(len(ref))])
    print("%s: cut vs one push max |diff| %.3e; oracle rel rms max %.3e (bin %d)" % (name, diff, errs.max(), int(errs.argmax())))
    assert one.shape == cut.shape == ref.shape
    np.testing.assert_array_equal(one, cut)
    assert errs.max() <= 1e-5, (name, int(errs.argmax()), float(errs.max()))


@pytest.mark.parametrize("name", ["plain-256", "two-branch-512", "persistent-512", "pfb5-1600", "pfbm-192"])
def test_launches_around_the_first_steady_frame(gpu_required, name):
    nat = gpu_required
    x, lead, ref = _stream(name)
    n_one, one, _ = _run(nat, name, [lead, len(x)])
    n_cut, cut, _ = _run(nat, name, _cuts(name, lead, len(x), (0,)))
    assert n_one == n_cut == ref.shape[1] >= FRAMES
    _check_bins(name, one, cut, ref)


@pytest.mark.parametrize("mode", [1, 2])
def test_fused_discriminator_around_both_boundaries(gpu_required, mode):
    """launches that begin around the first frame the plain predicate lets go AND around the first frame whose halo chunk --
    the chunk before it, which the first workgroups recompute -- no longer reaches before the opening sample"""
    nat = gpu_required
    name = "pfb5-1600"
    fs, nb, D, proto, ppad, F = _shape(name)
    x, lead, ref = _stream(name)
    fm_bins = sorted(set(range(0, nb, 7)) | {1, nb // 2 - 1, nb // 2, nb // 2 + 1, nb - 1})
    n_one, one, fm_one = _run(nat, name, [lead, len(x)], mode, fm_bins)
    n_cut, cut, fm_cut = _run(nat, name, _cuts(name, lead, len(x), (0, F)), mode, fm_bins)
    assert n_one == n_cut == ref.shape[1]
    if mode == 1:
        _check_bins(name + " fused", one, cut, ref)
    print("fused mode %d: discriminator cut vs one push max |diff| %.3e" % (mode, float(np.max(np.abs(fm_one - fm_cut)))))
    assert fm_one.shape == fm_cut.shape == (len(fm_bins), n_one)
    np.testing.assert_array_equal(fm_one, fm_cut)
    # The discriminator against the GNU-Radio-faithful channel, as tests/test_gpu_fm_fused.py holds it: on FM carriers.  That
    # channel's taps carry float32 phases (i w0 up to 8000 rad: ~3e-4 relative on its output), which the bar allows for a
    # carrier and not for a bin of bare noise -- 2e-3 rms there between the oracle and the exact-phase discriminator in
    # float64, whatever the bank does.  Carriers this strong beside bins of noise would in turn cost the IQ bar above (a
    # transform's rounding is relative to the strongest bin of a butterfly): a second stream of the same length, opened at
    # the same sample and cut at the same places.  The oracle's frame k0 - 1 is all zeros, the bank's is not defined: the
    # comparison starts two frames in, before every boundary.
    carriers = [7, 805, 1589]
    xc = _signal(np.random.default_rng(8200 + mode), fs, len(x), nb, carriers)
    _, _, fmc_one = _run(nat, name, [lead, len(x)], mode, carriers, x=xc)
    _, _, fmc_cut = _run(nat, name, _cuts(name, lead, len(x), (0, F)), mode, carriers, x=xc)
    np.testing.assert_array_equal(fmc_one, fmc_cut)
    xz = xc.copy()
    xz[:lead] = 0
    k0 = -(-lead // D)
    worst = 0.0
    for i, k in enumerate(carriers):
        ct, incr = OC.xlating_composite(proto, D, (k if k < nb // 2 else k - nb) * fs / nb, fs)
        _, fo = OC.channel_bank(xz, D, ct[None, :], np.array([incr]), gains=[1.0])
        want = fo[0][k0:]
        assert len(want) == n_one == fmc_cut.shape[1]
        d = np.angle(np.exp(1j * (fmc_cut[i].astype(np.float64) - want)))
        worst = max(worst, float(np.sqrt(np.mean(d[2:] ** 2))))
    print("fused mode %d: discriminator rms vs oracle %.3e" % (mode, worst))
    assert worst <= 1e-4, worst


def test_group_takes_a_member_in_at_its_first_steady_frame(gpu_required):
    """two 192-bin and two 1600-bin members pushed as group blocks; one of each pair is opened in mid-stream, and the rounds are
    cut around ITS first steady frame: before it the member goes out alone (masking kernel), from it on in its shape's
    grouped launch, which has no masking form"""
    nat = gpu_required
    names = ["pfbm-192", "pfbm-192", "pfb5-1600", "pfb5-1600"]
    late = [False, True, False, True]
    fes, xs, refs, leads, cuts = [], [], [], [], []
    for m, name in enumerate(names):
        fs, nb, D, proto, ppad, F = _shape(name)
        x, lead, ref = _stream(name)                           # both members of a pair carry the same stream
        if not late[m]:                                        # opened at sample 0: its own reference
            ref = _exact_all_bins(x, D, proto, nb, fs)
        fe = nat.Frontend(fs, 0.0, device=0, block_capacity=len(x), hist_capacity=1 << 15, out_capacity=1 << 10)
        if not late[m]:
            fe.pfb_open(nb, D, proto)
        fes.append(fe)
        xs.append(x)
        refs.append(ref)
        leads.append(lead)
        cuts.append([0] + _cuts(name, lead, len(x), (0,)))     # every member of a pair is cut where the late one needs it
    assert len({len(c) for c in cuts}) == 1
    grp = nat.Group(fes)
    try:
        for r in range(len(cuts[0]) - 1):
            if r == 1:
                for m, name in enumerate(names):
                    if late[m]:
                        fs, nb, D, proto, ppad, F = _shape(name)
                        fes[m].pfb_open(nb, D, proto)
            grp.push([xs[m][cuts[m][r]:cuts[m][r + 1]] for m in range(4)], nat.FMT_CF32)
        got = [np.stack([fe.pfb_read_bin(k) for k in range(_shape(name)[1])]) for fe, name in zip(fes, names)]
    finally:
        grp.close()
        for fe in fes:
            fe.close()
    for m, name in enumerate(names):
        fs, nb, D, proto, ppad, F = _shape(name)
        with nat.Frontend(fs, 0.0, device=0, block_capacity=len(xs[m]), hist_capacity=1 << 15, out_capacity=1 << 10) as fe:
            if late[m]:
                fe.push(xs[m][:leads[m]])
            fe.pfb_open(nb, D, proto)
            fe.push(xs[m][leads[m] if late[m] else 0:])
            one = np.stack([fe.pfb_read_bin(k) for k in range(nb)])
        _check_bins("group member %d (%s%s)" % (m, name, ", opened in mid-stream" if late[m] else ""), one, got[m], refs[m])
