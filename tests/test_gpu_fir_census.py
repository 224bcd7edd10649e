"""-m gpu: exact census of the stage-2 FIR kernels (radiocapture-rf_amd/csrc/fir.hip) under every launch plan.

Channels opened at offset 0 on integer taps and integer samples must equal the integer reference of tests/fir_census_ref.py
BIT FOR BIT, whatever the order of the float32 sums: matrix cores at every (NT, parts) the planner can answer (the table
is fir_census_ref.MFMA_ROWS; tests/test_fir_census_cpu.py holds its coverage), split-K and finish, the operand packer at
both tap parities and both sides of a chunk boundary, the zero-history fix-up launch, the vector kernel on a shared source
and on its own, and the small-T kernel with its fused discriminator.  Complex taps -- the [cr -ci; ci cr] signs and the
Re/Im placement the offset-0 census cannot see -- are held per output to the derived summation bound plus the recorded
rotator allowance."""
import numpy as np
import pytest

import fir_census_ref as R
from oracle import cbind as OC
from oracle import grspec as G

pytestmark = pytest.mark.gpu


def _first_mismatch(got, want):
    """index of the first element that differs (arrays of equal length), or None"""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return int(bad[0]) if len(bad) else None


def _assert_exact(got, want, what, plan=None):
    """np.array_equal with a message that names the output"""
    assert len(got) == len(want), "%s: %d outputs, want %d" % (what, len(got), len(want))
    if np.array_equal(got, want):
        return
    j = _first_mismatch(got, want)
    n_bad = int(np.count_nonzero(np.asarray(got) != np.asarray(want)))
    raise AssertionError("%s: output %d of this push is %r, want %r (%d of %d outputs differ)%s"
                         % (what, j, got[j], want[j], n_bad, len(want),
                            "" if plan is None else "; predicted plan NT %d, parts %d" % plan))


def _expect_fixup(k_lo, D, T, start=0):
    """split_class queues the vector fix-up launch behind the matrix cores while outputs still reach before the start"""
    return k_lo * D - start < T - 1


def _push_and_count(nat, fe, block, mfma, fixup, what):
    fe.push(block)
    n_mfma, n_vec = fe.timing_read(nat.T_FIR_MFMA)[1], fe.timing_read(nat.T_FIR)[1]
    assert (n_mfma, n_vec) == (mfma, fixup), "%s: %d matrix-core and %d vector launches, want %d and %d" % (what, n_mfma, n_vec, mfma, fixup)


@pytest.mark.parametrize("row", range(len(R.MFMA_ROWS)), ids=lambda i: "T%d_D%d_%dch" % R.MFMA_ROWS[i][:3])
def test_matrix_core_bank_equals_the_integer_census(gpu_required, row):
    nat = gpu_required
    T, D, n_chans, n_ks, out_cap = R.MFMA_ROWS[row]
    cuts = R.cuts_for(n_ks, D)
    x, taps, y = R.census(np.random.default_rng(1000 + row), T, D, n_chans, sum(cuts), 7, 7)
    with nat.Frontend(1e6, out_capacity=out_cap) as fe:
        ids = [fe.chan_open_taps(-1, D, taps[c], 0.0) for c in range(n_chans)]
        fe.timing_enable(True)
        at = k = 0
        for j, (n, nk) in enumerate(zip(cuts, n_ks)):
            plan = R.mfma_plan(n_chans, nk, T)
            what = "row %d (T %d, D %d, %d channels) push %d of %d outputs" % (row, T, D, n_chans, j, nk)
            # one matrix-core launch per push; while outputs still reach before sample 0, the vector fix-up launch behind it
            _push_and_count(nat, fe, x[at:at + n], 1, int(_expect_fixup(k, D, T)), what)
            for c, cid in enumerate(ids):
                _assert_exact(fe.chan_read_iq(cid), y[c, k:k + nk], "%s, channel %d, first output %d" % (what, c, k), plan)
            at += n
            k += nk
        assert k == y.shape[1]


@pytest.mark.parametrize("n_ks", [[1400, 1400], [3000, 3000]], ids=["NT1", "NT2"])
def test_coded_impulses_name_the_channel_and_tap_every_output_read(gpu_required, n_ks):
    """taps[c, t] = 1 + t + 1024 c against unit impulses T samples apart: every output of every channel is the code of
    exactly one tap, under a (1, 7) and under a (2, 7) plan (8 chunks in 7 parts)"""
    nat = gpu_required
    T, D, n_chans = 449, 2, 65
    plans = [R.mfma_plan(n_chans, nk, T) for nk in n_ks]
    assert plans == [({1400: 1, 3000: 2}[n_ks[0]], 7)] * 2
    cuts = R.cuts_for(n_ks, D)
    n = sum(cuts)
    x, taps, want = R.coded(T, D, n_chans, n, range(0, n, T))
    assert (want >= 0).all()
    with nat.Frontend(1e6) as fe:
        ids = [fe.chan_open_taps(-1, D, taps[c], 0.0) for c in range(n_chans)]
        fe.timing_enable(True)
        at = k = 0
        for j, (m, nk) in enumerate(zip(cuts, n_ks)):
            _push_and_count(nat, fe, x[at:at + m], 1, int(_expect_fixup(k, D, T)), "push %d" % j)
            for c, cid in enumerate(ids):
                gc, gt = R.decode(fe.chan_read_iq(cid))
                assert len(gt) == nk
                bad = np.flatnonzero((gc != c) | (gt != want[k:k + nk]))
                assert not len(bad), ("channel %d output %d read (channel, tap) = (%d, %d), want (%d, %d); %d outputs of this "
                                      "push differ; plan NT %d, parts %d"
                                      % (c, k + bad[0], gc[bad[0]], gt[bad[0]], c, want[k + bad[0]], len(bad), *plans[j]))
            at += m
            k += nk


def test_lifecycle_close_open_and_shrink_stay_exact(gpu_required):
    """40 channels; one closes (ids shift, the groups of 32 repack); a new one opens mid-stream off the decimation grid
    (zero history before its start: masked fix-up outputs); the class shrinks to 32 and loses its second group"""
    nat = gpu_required
    T, D = 191, 3
    rng = np.random.default_rng(77)
    n_ks = [70, 130, 129, 200]
    cuts = R.cuts_for(n_ks, D)
    x = R.int_stream(rng, sum(cuts), 7)
    taps = R.int_taps(rng, 41, T, 7)
    ends = np.cumsum(cuts)
    starts = {}
    with nat.Frontend(1e6) as fe:
        ids = {c: fe.chan_open_taps(-1, D, taps[c], 0.0) for c in range(40)}
        starts.update({c: 0 for c in ids})
        fe.timing_enable(True)
        ref = {c: R.fir_reference(x, taps[c], D)[0].astype(np.complex64) for c in range(40)}
        read = {c: 0 for c in range(41)}

        def step(j, fixup):
            lo = int(ends[j] - cuts[j])
            _push_and_count(nat, fe, x[lo:ends[j]], 1, fixup, "step %d" % j)
            k_end = R.n_outputs(int(ends[j]), D)
            for c, cid in ids.items():
                k0 = -(-starts[c] // D)
                want = ref[c][read[c]:k_end - k0]
                _assert_exact(fe.chan_read_iq(cid), want, "step %d, channel %d (%d open), from its output %d"
                              % (j, c, len(ids), read[c]), R.mfma_plan(len(ids), n_ks[j], T))
                read[c] = k_end - k0

        step(0, 1)
        fe.chan_close(ids.pop(3))
        step(1, 0)
        starts[40] = int(ends[1])
        assert starts[40] % D != 0
        ids[40] = fe.chan_open_taps(-1, D, taps[40], 0.0)
        assert fe.chan_start(ids[40]) == starts[40]
        ref[40] = R.fir_reference(x, taps[40], D, start=starts[40])[0].astype(np.complex64)
        step(2, 1)                                          # the new channel's first (T - 1) / D outputs are redone masked
        for c in (0, 7, 31, 32, 35, 36, 38, 39):
            fe.chan_close(ids.pop(c))
        assert len(ids) == 32
        step(3, 0)


@pytest.mark.parametrize("row", range(len(R.COMPLEX_ROWS)), ids=lambda i: "T%d_D%d_%dch" % R.COMPLEX_ROWS[i][:3])
def test_complex_taps_within_the_summation_bound(gpu_required, row):
    """Gaussian samples, random float taps, non-zero offsets: per output against phase_oracle[k] * sum ct32[t] x[k D - t] in
    float64, tolerance = summation_bound + rotator allowance * |v_ref[k]| (fir_census_ref: both derived or measured on the CPU)"""
    nat = gpu_required
    T, D, n_chans, n_ks = R.COMPLEX_ROWS[row]
    fs = R.COMPLEX_FS
    rng = np.random.default_rng(2000 + row)
    cuts = R.cuts_for(n_ks, D)
    n = sum(cuts)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    taps = rng.standard_normal((n_chans, T)).astype(np.float32)
    offs = R.complex_offsets(n_chans)
    n_out = R.n_outputs(n, D)
    parts = np.concatenate([np.full(nk, R.mfma_plan(n_chans, nk, T)[1]) for nk in n_ks])
    comp = [OC.xlating_composite(taps[c], D, offs[c], fs) for c in range(n_chans)]
    ct = np.stack([c[0] for c in comp])
    phases = {}
    for (_, incr), f in zip(comp, offs):
        if f not in phases:
            phases[f] = G.rotator_phases(incr, n_out)[0].astype(np.complex128)
    v = R.fir_reference(x, ct, D)
    tol = R.summation_bound(ct, x, D, T, parts[None, :]) + R.ROTATOR_ALLOWANCE * np.abs(v)
    with nat.Frontend(fs) as fe:
        ids = [fe.chan_open_taps(-1, D, taps[c], offs[c]) for c in range(n_chans)]
        fe.timing_enable(True)
        at = k = 0
        got = [[] for _ in ids]
        for j, (m, nk) in enumerate(zip(cuts, n_ks)):
            _push_and_count(nat, fe, x[at:at + m], 1, int(_expect_fixup(k, D, T)), "push %d" % j)
            for c, cid in enumerate(ids):
                got[c].append(fe.chan_read_iq(cid))
            at += m
            k += nk
    worst = 0.0
    for c in range(n_chans):
        y = np.concatenate(got[c]).astype(np.complex128)
        want = v[c] * phases[offs[c]]
        assert len(y) == n_out
        err = np.abs(y - want)
        worst = max(worst, float((err / tol[c]).max()))
        bad = np.flatnonzero(err > tol[c])
        assert not len(bad), ("channel %d (offset %.0f Hz) output %d: %r, want %r, |error| %.3e > tolerance %.3e; %d outputs out"
                              % (c, offs[c], bad[0], y[bad[0]], want[bad[0]], err[bad[0]], tol[c][bad[0]], len(bad)))
    print("largest |error| / tolerance: %.3e" % worst)


# ---------------------------------------------------------------------------------------------- vector kernels
@pytest.mark.parametrize("D", R.VECTOR_D)
@pytest.mark.parametrize("T", R.VECTOR_T)
@pytest.mark.parametrize("n_chans", R.VECTOR_CHANS)
def test_vector_bank_on_a_shared_source_equals_the_integer_census(gpu_required, n_chans, T, D):
    """fir_bank_kernel, direct channels below 64 taps: a dead channel of a CT = 2 pair (1, 3, 17), a second workgroup row
    holding one channel (17), pushes of 1, 7, 8 and 9 outputs around KR = 8 and past the 256-output tile; the first pushes
    are zero history (fir_item<true>) wherever T > 1"""
    nat = gpu_required
    cuts = R.cuts_for(R.VECTOR_N_KS, D)
    x, taps, y = R.census(np.random.default_rng(100 * n_chans + 10 * T + D), T, D, n_chans, sum(cuts), 7, 63)
    with nat.Frontend(1e6, block_capacity=1 << 15) as fe:
        ids = [fe.chan_open_taps(-1, D, taps[c], 0.0) for c in range(n_chans)]
        fe.timing_enable(True)
        at = k = 0
        for j, (n, nk) in enumerate(zip(cuts, R.VECTOR_N_KS)):
            what = "T %d, D %d, %d channels, push %d of %d outputs" % (T, D, n_chans, j, nk)
            _push_and_count(nat, fe, x[at:at + n], 0, 1, what)
            for c, cid in enumerate(ids):
                _assert_exact(fe.chan_read_iq(cid), y[c, k:k + nk], "%s, channel %d, first output %d" % (what, c, k))
            at += n
            k += nk


def test_chained_channels_small_and_vector_kernels_equal_the_integer_census(gpu_required):
    """fir_small_kernel (T 1, 5, 95, 96) and the own-source fir_bank_kernel (T 97, 200), D 1 and 3, as children of two
    offset-0 integer channels: IQ bit for bit; and the discriminator behind them -- fused into the small kernel, disc_kernel
    behind the vector kernel -- bit for bit against quadrature_demod_cf of the reference IQ: its products y[k] conj(y[k-1])
    are exact integers below 2^24, so fusing cannot show (tests/test_fir_census_cpu.py
    ::test_chain_case_is_exact_and_the_discriminator_oracle_does_not_depend_on_fusing), and the device's fast_atan2f is the
    oracle's bit for bit (tests/test_device_atan_cpu.py)."""
    nat = gpu_required
    x, cuts, parents, children = R.chain_case(np.random.default_rng(11))
    Tp, Dp = R.CHAIN_PARENT
    with nat.Frontend(1e6, block_capacity=1 << 15) as fe:
        pids = [fe.chan_open_taps(-1, Dp, tp, 0.0) for tp, _ in parents]
        cids = [fe.chan_open_taps(pids[pi], D, tc, 0.0) for pi, T, D, tc, _, _ in children]
        at = 0
        kp = 0
        read = [0] * len(children)
        for j, (n, nk) in enumerate(zip(cuts, R.CHAIN_PARENT_N_KS)):
            fe.push(x[at:at + n])
            at += n
            kp += nk
            for pid, (_, yp) in zip(pids, parents):
                _assert_exact(fe.chan_read_iq(pid), yp[kp - nk:kp], "push %d, parent %d" % (j, pid))
            for i, (cid, (pi, T, D, tc, yc, fm)) in enumerate(zip(cids, children)):
                k_end = R.n_outputs(kp, D)
                what = "push %d, child T %d D %d of parent %d, from its output %d" % (j, T, D, pi, read[i])
                _assert_exact(fe.chan_read_iq(cid), yc[read[i]:k_end], what + ", IQ")
                _assert_exact(fe.chan_read_fm(cid, 1.0).view(np.uint32), fm[read[i]:k_end].view(np.uint32), what + ", discriminator bits")
                read[i] = k_end
        assert all(r == len(c[4]) for r, c in zip(read, children))
