"""The symbol clock stage without a GPU (rcf_chan_clock_mm, rcf_design_mmse_interpolator, rcf/control.py): the
interpolator bank against an independent solve, the float32 restatement (tests/mm_ref.py) as a clock recovery on a
known signal, the slicer / packer, and the binding."""
import numpy as np

import mm_ref as M
from rcf import control, native


def test_interpolator_bank_unit_rows_and_independent_solve():
    T = native.design_mmse_interpolator()
    assert T.shape == (129, 8) and T.dtype == np.float32
    # rows 0 and 128 are the unit rows, exactly: with T[imu][7 - j] the interpolated point is p + 3 + mu
    assert T[0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert T[128].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    # Float rounding of values <= 1 is 6e-8; the rest of 1e-6 is for two solvers of an 8 x 8 system of condition number
    # 6.2e4 (double: ~1e-11).  Measured here: 3.0e-8, i.e. the rounding alone.
    want = M.mmse_bank()
    d = float(np.abs(T.astype(np.float64) - want).max())
    print("interpolator bank: max |product - numpy.linalg.solve| = %.3g" % d)
    assert d <= 1e-6
    # the sizing convention of the other design entry points, and the general form
    assert native.lib().rcf_design_mmse_interpolator(8, 128, 0.25, None, 0) == -129 * 8
    assert native.lib().rcf_design_mmse_interpolator(7, 128, 0.25, None, 0) == native.RCF_EINVAL
    assert native.lib().rcf_design_mmse_interpolator(8, 128, 0.75, None, 0) == native.RCF_EINVAL
    T4 = native.design_mmse_interpolator(4, 16, 0.2)
    assert float(np.abs(T4 - M.mmse_bank(4, 16, 0.2)).max()) <= 1e-6
    assert T4[0].tolist() == [0, 0, 1, 0] and T4[16].tolist() == [0, 1, 0, 0]


def test_restatement_recovers_a_clean_two_level_signal():
    """+-1 rectangular pulses at 25000 / 3600 samples per symbol: after the first 100 symbols the restatement's bits are
    the sent bits at one contiguous alignment offset, without an error -- a clock recovery, not merely self-consistent"""
    T = native.design_mmse_interpolator()
    sps = 25000 / 3600.0
    for seed in (1, 2, 3):
        bits = np.random.default_rng(seed).integers(0, 2, 700)
        x = M.fsk2_baseband(bits, sps)
        y, slips = M.clock_recovery_mm(x, sps, gain=1.0, taps=T)
        assert slips == 0 and abs(len(y) - len(bits)) <= 2, (seed, len(y), slips)
        off, errs = M.align_bits(y >= 0, bits, skip=100)
        print("seed %d: %d symbols, offset %d, %d errors" % (seed, len(y), off, errs))
        assert errs == 0 and len(y) - 100 >= 500, (seed, off, errs)
    # the caller's bank is honoured by the restatement too: linear interpolation recovers the same bits
    y, _ = M.clock_recovery_mm(x, sps, gain=1.0, taps=M.linear_bank())
    assert M.align_bits(y >= 0, bits, skip=100)[1] == 0
    # gain in front is one float32 product
    y5, _ = M.clock_recovery_mm(x, sps, gain=5.0, taps=T)
    y5u, _ = M.clock_recovery_mm((np.float32(5.0) * x).astype(np.float32), sps, taps=T, unit_gain_input=False)
    assert y5.tobytes() == y5u.tobytes()


def test_restatement_guards():
    """a step < 1 advances by one input, a non-finite state starts over ceil(omega) inputs on: both counted, and at most
    one symbol per input whatever the input"""
    T = native.design_mmse_interpolator()
    rng = np.random.default_rng(5)
    x = rng.uniform(-np.pi, np.pi, 2000).astype(np.float32)
    y, slips = M.clock_recovery_mm(x, 2.6, gain_mu=1.0, taps=T)
    assert slips > 0 and len(y) <= len(x)
    y, slips = M.clock_recovery_mm(x, 2.6, gain_omega=3e38, taps=T)
    assert slips > 0 and len(y) <= len(x) and np.isfinite(y).all()
    y, _ = M.clock_recovery_mm(x, 2.6, gain_mu=3e38, taps=T)      # a step that saturates ends the stream's symbols
    assert len(y) < 20
    x[100] = np.nan
    y, slips = M.clock_recovery_mm(x, 6.9, taps=T)
    assert slips > 0 and np.isnan(y).sum() <= 8 + 8       # the windows that hold the sample, and the one after each reset


def test_pack_bits_is_packbits_with_carries():
    rng = np.random.default_rng(11)
    soft = rng.standard_normal(1003).astype(np.float32)
    soft[::17] = 0.0                                       # binary_slicer_fb: x >= 0 is a one
    want_bits = (soft >= 0).astype(np.uint8)
    got, carry, at = [], None, 0
    for n in (0, 1, 7, 8, 9, 64, 5, 300, 3, 606):
        b, carry = control.pack_bits(soft[at:at + n], carry)
        assert b.dtype == np.uint8 and len(carry) < 8
        got.append(b)
        at += n
    assert at == len(soft)
    got = np.concatenate(got)
    np.testing.assert_array_equal(got, np.packbits(want_bits[:len(want_bits) // 8 * 8]))
    np.testing.assert_array_equal(carry, want_bits[len(want_bits) // 8 * 8:])
    assert control.pack_bits(np.array([1, -1, 1, 1, 0, -0.5, -2, 3], dtype=np.float32))[0].tolist() == [0b10111001]


def test_native_exposes_the_clock_entry_points():
    for s in ("rcf_chan_clock_mm", "rcf_chan_clock_produced", "rcf_chan_read_clock", "rcf_chan_clock_ring",
              "rcf_design_mmse_interpolator"):
        assert s in native.SYMBOLS and hasattr(native.lib(), s), s
    for m in ("chan_clock_mm", "chan_read_clock", "chan_clock_produced", "chan_clock_ring"):
        assert callable(getattr(native.Frontend, m)), m
    assert native.T_CLOCK == 10
    assert callable(control.smartnet_clock) and callable(control.edacs_clock)
