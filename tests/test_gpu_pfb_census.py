"""-m gpu: exact census of the polyphase filterbanks (radiocapture-rf_amd/csrc/pfb.hip, pfb5.hip, pfbm.hip), through the C ABI.

Bin 0 of every bank is a plain FIR whose float32 sums are exact on small integers in any order, so it must equal the
integer reference of tests/pfb_census_ref.py BIT FOR BIT: one row per kernel instantiation of pfb_shape.h, pushed in cuts
chosen against the row's chunk and its zero-history boundary into a ring that wraps; the grouped kernels, the persistent
kernel walking more chunks than it has workgroups, the 256-bin bank carrying the stage-2 rider, the fused discriminator
in both modes and one launch of 2048 chunks.  One missing, doubled or misplaced tap or input row shows in a named frame.
The coded impulses then name the tap and the branch-to-bin twiddle EVERY output of every bin read: its magnitude is the
tap's code (an integer: bar 0.5), its phase that of one unit phasor (bar: a quarter of the 2 pi / NB step between two
(branch, bin) pairs); the banks' float32 rounding, relative 2e-7 (tests/test_gpu_pfbm.py), leaves both bars a factor of
more than 100 at T <= 16384.  tests/test_pfb_census_cpu.py holds the table's coverage and the references."""
import numpy as np
import pytest

import pfb_census_ref as P
from fir_census_ref import fir_reference, int_stream, int_taps, n_outputs

pytestmark = pytest.mark.gpu

FS = 20e6


def _assert_exact(got, want, what, chunk, first_frame=0):
    """np.array_equal with a message that names the frame: `first_frame` is the position of got[0] in its LAUNCH, whose
    chunks (one workgroup each) are counted from the launch's first frame"""
    assert len(got) == len(want), "%s: %d frames, want %d" % (what, len(got), len(want))
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    j = int(bad[0])
    raise AssertionError("%s: frame %d of this push is %r, want %r -- chunk %d of the launch, position %d of %d in it; %d of %d "
                         "frames differ" % (what, j, got[j], want[j], (first_frame + j) // chunk, (first_frame + j) % chunk, chunk,
                                            len(bad), len(want)))


def _hist(NB, Ppad):
    return max(1 << 14, 2 * NB * Ppad)


# ---------------------------------------------------------------------------------------------- 1. every instantiation
@pytest.mark.parametrize("row", range(len(P.PFB_ROWS)), ids=lambda i: P.row_id(P.PFB_ROWS[i]))
def test_bin0_of_every_bank_equals_the_integer_fir(gpu_required, row):
    nat = gpu_required
    r = P.PFB_ROWS[row]
    x, h, y = P.bank_census(r, np.random.default_rng(7000 + row))
    zh = P.launches_zero_history(r)
    with nat.Frontend(FS, block_capacity=max(r.cuts + [r.lead]), hist_capacity=_hist(r.NB, r.Ppad), out_capacity=P.RING) as fe:
        fe.push(x[:r.lead])                                  # a lead-in that is no multiple of D
        fe.pfb_open(r.NB, r.D, h)
        fe.timing_enable(True, classes=[nat.T_PFB])
        at, m = r.lead, 0
        for j, (n, c) in enumerate(zip(r.cuts, r.n_frames)):
            what = "%s (T %d, chunk %d) push %d of %d frames from frame %d%s" % (
                P.row_id(r), r.T, r.chunk, j, c, m, " [zero-history launch]" if zh[j] else "")
            fe.push(x[at:at + n])
            at += n
            launches = fe.timing_read(nat.T_PFB)[1]
            assert launches == (1 if c else 0), "%s: %d filterbank launches" % (what, launches)
            _assert_exact(fe.pfb_read_bin(0), y[m:m + c], what, r.chunk)
            m += c
        assert fe.pfb_produced() == m == len(y)


# ---------------------------------------------------------------------------------------------- 2. other launch forms
GROUP_SHAPES = [(256, 1, 14), (512, 1, 4), (400, 2, 2), (192, 2, 2)]     # pfb_group_kernel_os, _2b, pfb5_group_kernel, pfbm_group_kernel
# frames per member and round: all three mask (their first launch); a ragged round; member 1 skipped; ragged; member 1 alone
GROUP_ROUNDS = [[40, 40, 40], [33, 16, 50], [17, 0, 31], [1, 47, 16], [0, 5, 0]]


@pytest.mark.parametrize("shape", GROUP_SHAPES, ids=lambda s: "%dbins_os%d_p%d" % s)
def test_grouped_launch_bin0_equals_the_integer_fir(gpu_required, shape):
    nat = gpu_required
    NB, OS, Pp = shape
    D, T, F = NB // OS, NB * Pp - NB // 3, 16
    M = 3
    members = []
    for m in range(M):
        n_frames = [rd[m] for rd in GROUP_ROUNDS if rd[m]]
        x, h, _, cuts, y = P.simple_census(np.random.default_rng(8000 + NB + m), NB, D, T, n_frames)
        members.append((x, h, iter(cuts), y))
    fes = [nat.Frontend(FS, 0.0, device=0, block_capacity=1 << 15, hist_capacity=_hist(NB, Pp), out_capacity=P.RING) for _ in range(M)]
    try:
        for fe, (x, h, _, _) in zip(fes, members):
            fe.pfb_open(NB, D, h)
            fe.timing_enable(True, classes=[nat.T_PFB])
        with nat.Group(fes) as grp:
            at, done = [0] * M, [0] * M
            for rnd, frames in enumerate(GROUP_ROUNDS):
                blocks, masks = [], 0
                for m, c in enumerate(frames):
                    if not c:
                        blocks.append(None)
                        continue
                    n = next(members[m][2])
                    blocks.append(members[m][0][at[m]:at[m] + n])
                    at[m] += n
                    masks += P.zero_history(NB, D, Pp, done[m], 0)
                grp.push(blocks)
                grp.sync()
                steady = sum(1 for c in frames if c) - masks
                launches = sum(fe.timing_read(nat.T_PFB)[1] for fe in fes)
                # a member whose launch still masks goes alone; two or more in steady state share ONE launch
                assert launches == masks + min(steady, 1), "round %d: %d filterbank launches" % (rnd, launches)
                for m, c in enumerate(frames):
                    what = "%d bins OS %d, round %d, member %d, %d frames from frame %d" % (NB, OS, rnd, m, c, done[m])
                    _assert_exact(fes[m].pfb_read_bin(0), members[m][3][done[m]:done[m] + c], what, F)
                    done[m] += c
            assert [d for d in done] == [len(mb[3]) for mb in members]
    finally:
        for fe in fes:
            fe.close()


def test_persistent_kernel_walking_several_chunks_per_workgroup(gpu_required):
    """512 bins at OS 2 (pfb_kernel_pp): one resident round of workgroups, two per CU; a launch of 552 chunks and three frames
    makes some of them walk two chunks and others one"""
    nat = gpu_required
    NB, D, Pp, F = 512, 256, 4, 16
    n_frames = [70, 552 * F + 3]
    x, h, _, cuts, y = P.simple_census(np.random.default_rng(81), NB, D, NB * Pp - NB // 3, n_frames)
    assert not P.zero_history(NB, D, Pp, n_frames[0], 0)
    with nat.Frontend(FS, block_capacity=max(cuts), hist_capacity=_hist(NB, Pp), out_capacity=1 << 14) as fe:
        fe.pfb_open(NB, D, h)
        fe.timing_enable(True, classes=[nat.T_PFB])
        at = m = 0
        for j, (n, c) in enumerate(zip(cuts, n_frames)):
            fe.push(x[at:at + n])
            at += n
            assert fe.timing_read(nat.T_PFB)[1] == 1
            _assert_exact(fe.pfb_read_bin(0), y[m:m + c], "512 bins OS 2, push %d" % j, F)
            m += c


def test_bank_carrying_the_stage2_rider_both_exact(gpu_required):
    """The 256-bin bank with a channel of 11 integer taps at decimation 3 on bin 0.  Nothing is read between the pushes (a read
    queues the pending stage-2 launch at once), so block n's stage-2 launch rides in block n + 1's filterbank launch: the
    first block's trails its masking launch, the last one's is queued by the first read -- two stage-2 launches of their
    own for six blocks.  The bank's bin 0 and the channel's IQ are both exact."""
    nat = gpu_required
    c = P.rider_case(np.random.default_rng(31))
    with nat.Frontend(FS, block_capacity=max(c["cuts"]), hist_capacity=1 << 14, out_capacity=1 << 12) as fe:
        fe.pfb_open(c["NB"], c["D"], c["h"])
        cid = fe.chan_open_taps(nat.SRC_PFB_BIN0 + 0, c["D2"], c["t2"], 0.0)
        fe.timing_enable(True, classes=[nat.T_PFB, nat.T_FIR_DERIVED])
        at = 0
        for n in c["cuts"]:
            fe.push(c["x"][at:at + n])
            at += n
        n_pfb, n_s2 = fe.timing_read(nat.T_PFB)[1], fe.timing_read(nat.T_FIR_DERIVED)[1]
        assert (n_pfb, n_s2) == (len(c["cuts"]), 2), "%d filterbank and %d stage-2 launches" % (n_pfb, n_s2)
        _assert_exact(fe.pfb_read_bin(0), c["y0"], "256 bins with the rider, bin 0", 16)
        got = fe.chan_read_iq(cid)
        assert len(got) == len(c["y2"]) == n_outputs(len(c["y0"]), c["D2"])
        bad = np.flatnonzero(got != c["y2"])
        assert not len(bad), ("stage-2 channel on bin 0: output %d is %r, want %r; %d of %d outputs differ (bank frames per push %s)"
                              % (bad[0], got[bad[0]], c["y2"][bad[0]], len(bad), len(got), c["n_frames"]))


@pytest.mark.parametrize("mode", [1, 2], ids=["beside_the_bins", "instead_of_the_bins"])
def test_fused_discriminator_bin0_exact(gpu_required, mode):
    """400 bins at OS 2 with rcf_pfb_fm_enable (gr_phase on: at bin 0 GNU Radio's rotator advance is float32(-0 * D) = the
    exact phase, the increment is (1, 0) and the turn by it is exact).  Mode 1: bin 0 of the bins ring; mode 2: an idle
    tap on bin 0; both modes: the discriminator ring against quadrature_demod_cf of the integer reference, bit for bit,
    over ALL outputs (pfb_census_ref.fm_case: every product and sum is an integer below 2^24; tests/test_device_atan_cpu.py
    pins the device's arctangent to the oracle's)"""
    nat = gpu_required
    c = P.fm_case(np.random.default_rng(41))
    assert c["exact"].all()
    with nat.Frontend(FS, block_capacity=max(c["cuts"]), hist_capacity=1 << 15, out_capacity=1 << 10) as fe:
        fe.pfb_open(c["NB"], c["D"], c["h"])
        tap = fe.pfb_tap_open(0, gr_phase=False) if mode == 2 else None
        fe.pfb_fm_enable(mode, gr_phase=True)
        fe.timing_enable(True, classes=[nat.T_PFB])
        at = m = 0
        for j, (n, k) in enumerate(zip(c["cuts"], c["n_frames"])):
            what = "400 bins OS 2 fused mode %d, push %d of %d frames from frame %d" % (mode, j, k, m)
            fe.push(c["x"][at:at + n])
            at += n
            assert fe.timing_read(nat.T_PFB)[1] == 1, what
            iq = fe.pfb_read_bin(0) if mode == 1 else fe.chan_read_iq(tap)
            _assert_exact(iq, c["y0"][m:m + k], what + (", bins ring" if mode == 1 else ", idle tap"), 16)
            fm = fe.pfb_read_fm(0, 1.0)
            _assert_exact(fm.view(np.uint32), c["fm"][m:m + k].view(np.uint32), what + ", discriminator bits", 16)
            m += k
        assert fe.pfb_fm_lost() == 0


def test_one_launch_of_2048_chunks_of_the_headline_shape(gpu_required):
    """256 bins, OS 1, 14 rows: a small push (the masking launch), then ONE push of 2^23 samples = 32768 frames"""
    nat = gpu_required
    NB, D, F = 256, 256, 16
    T = NB * 14 - 85
    n0, n1 = 64 * D + 5, 1 << 23
    rng = np.random.default_rng(91)
    x = int_stream(rng, n0 + n1, P.X_MAX)
    h = int_taps(rng, 1, T, P.H_MAX)[0]
    assert T * 2 * P.X_MAX * P.H_MAX < 2 ** 24
    y = fir_reference(x, h, D)[0].astype(np.complex64)       # (the gather runs in blocks of 2048 frames)
    k0 = n_outputs(n0, D)
    assert len(y) - k0 == 2048 * F and not P.zero_history(NB, D, 14, k0, 0)
    with nat.Frontend(FS, block_capacity=n1, out_capacity=1 << 15) as fe:
        fe.pfb_open(NB, D, h)
        fe.timing_enable(True, classes=[nat.T_PFB])
        fe.push(x[:n0])
        _assert_exact(fe.pfb_read_bin(0), y[:k0], "256 bins, first push", F)
        fe.push(x[n0:])
        assert fe.timing_read(nat.T_PFB)[1] == 2
        _assert_exact(fe.pfb_read_bin(0), y[k0:], "256 bins, the launch of 2048 chunks", F)


# ---------------------------------------------------------------------------------------------- 3. coded impulses
CODED_PIECE, CODED_RING = 203, 256       # frames per push (no multiple of any chunk) and frames of the bins ring


@pytest.mark.parametrize("shape", P.CODED_SHAPES, ids=lambda s: "%d_os%d_p%d" % s[:3])
def test_coded_impulses_name_tap_and_twiddle_of_every_output(gpu_required, shape):
    nat = gpu_required
    NB, OS, Ppad, all_bins = shape
    D = NB // OS
    bins = list(range(NB)) if all_bins else P.spread_bins(NB)
    x, h, tap, want = P.coded_bank(NB, D, Ppad, bins=bins)
    piece = CODED_PIECE * D - 5                              # samples per push: the cuts drift off the frame grid
    phase_bar = np.pi / (2 * NB)
    worst_mag = worst_ph = 0.0
    with nat.Frontend(FS, block_capacity=piece, hist_capacity=_hist(NB, Ppad), out_capacity=CODED_RING) as fe:
        fe.pfb_open(NB, D, h)
        m = 0
        for at in range(0, len(x), piece):
            fe.push(x[at:at + piece])
            got = np.stack([fe.pfb_read_bin(k, CODED_RING) for k in bins], axis=1).astype(np.complex128)      # [frames, bins]
            n = got.shape[0]
            assert n <= CODED_PIECE and m + n <= len(tap)
            t, w = tap[m:m + n], want[m:m + n]
            none = t < 0
            bad = np.argwhere(got[none] != 0)
            assert not len(bad), ("%d bins OS %d: frame %d of bin %d reads no tap and is %r, want exactly 0; %d such outputs"
                                  % (NB, OS, m + np.flatnonzero(none)[bad[0][0]], bins[bad[0][1]], got[none][tuple(bad[0])], len(bad)))
            g, w, t = got[~none], w[~none], t[~none]
            frames = m + np.flatnonzero(~none)
            read, _ = P.decode_bank(g)
            dph = np.abs(np.angle(g * np.conj(w)))
            bad = np.argwhere((read != t[:, None]) | ~(dph < phase_bar))
            if len(bad):
                f, b = bad[0]
                raise AssertionError("%d bins OS %d: bin %d frame %d reads tap %d (branch %d), want tap %d (branch %d); phase off by "
                                     "%.3e rad (bar %.3e); %d outputs of this push differ"
                                     % (NB, OS, bins[b], frames[f], read[f, b], read[f, b] % NB, t[f], t[f] % NB, dph[f, b],
                                        phase_bar, len(bad)))
            if len(g):
                worst_mag = max(worst_mag, float(np.abs(np.abs(g) - (1 + t[:, None])).max()))
                worst_ph = max(worst_ph, float(dph.max()))
            m += n
        assert m == len(tap) == fe.pfb_produced()
    print("coded %d bins OS %d P %d (%d bins read, %d frames): largest magnitude error %.3e (bar 0.5), largest phase error %.3e rad "
          "(bar %.3e)" % (NB, OS, Ppad, len(bins), len(tap), worst_mag, worst_ph, phase_bar))
