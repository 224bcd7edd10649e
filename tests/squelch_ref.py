"""The carrier detector (rcf_chan_squelch, rcf_pfb_squelch; definition: include/rcf.h) restated in numpy / float64, and the
signals the CPU and GPU suites share.

GNU Radio 3.8's simple_squelch_cc_impl::work, sample by sample:
    thr   = pow(10.0, threshold_db / 10)
    p     = float32(re * re + im * im)         float32 products, float32 sum
    level = alpha * p + (1 - alpha) * level    single_pole_iir<double,double,double>, level 0 at the start
    open  = level >= thr
The loop below is sequential in time and elementwise over any trailing axes (the bins of a bank): numpy's elementwise
multiply and add round each result once, like the C++ compiled without contraction."""
import math

import numpy as np


def threshold(db):
    """simple_squelch_cc::set_threshold: C's pow"""
    return math.pow(10.0, float(db) / 10)


def power(x):
    """|x|^2 as the block computes it: float32 products and a float32 sum"""
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    return re * re + im * im


def run(x, thr, alpha, level0=0.0, first_index=0):
    """The sequential evaluation over axis 0 of x (complex64; further axes: independent streams, thr broadcast over them).
    -> dict(levels [like x] float64, level (the last), open [like x] bool, n_seen, n_open, first_open, last_open (indices from
    first_index on, -1: none), unmuted)"""
    p = power(x).astype(np.float64)
    n = p.shape[0]
    shape = p.shape[1:]
    thr = np.broadcast_to(np.asarray(thr, np.float64), shape)
    alpha = np.asarray(alpha, np.float64)         # (one per stream, or one for all)
    oma = np.float64(1.0) - alpha
    level = np.broadcast_to(np.asarray(level0, np.float64), shape).copy()
    levels = np.empty(p.shape, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            level = alpha * p[i] + oma * level
            levels[i] = level
        is_open = levels >= thr                       # a NaN: False
    idx = np.arange(first_index, first_index + n, dtype=np.int64).reshape((n,) + (1,) * len(shape))
    any_open = is_open.any(axis=0) if n else np.zeros(shape, bool)
    big = np.iinfo(np.int64).max
    first = np.where(any_open, np.where(is_open, idx, big).min(axis=0, initial=big), -1)
    last = np.where(any_open, np.where(is_open, idx, -1).max(axis=0, initial=-1), -1)
    return dict(levels=levels, level=levels[-1] if n else level, open=is_open, n_seen=n, n_open=is_open.sum(axis=0).astype(np.int64),
                first_open=first.astype(np.int64), last_open=last.astype(np.int64),
                unmuted=is_open[-1] if n else np.zeros(shape, bool))


def margin(levels, thr):
    """min over samples of |level / thr - 1|: how far the closest level stays from its threshold (a NaN level counts as far:
    it is muted whatever the rounding)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.asarray(levels, np.float64) / thr - 1.0)
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.min()) if d.size else float("inf")


def bound(alpha):
    """the derived bound of the segmented evaluation against the sequential one, relative (rcf.h at rcf_pfb_squelch)"""
    return 64.0 * 2.0 ** -53 / alpha


def ragged_cuts(n, sizes):
    """cut points 0 = c0 <= c1 <= ... = n: the given piece sizes in turn (zeros allowed), then the rest"""
    cuts = [0]
    for s in sizes:
        if cuts[-1] + s > n:
            break
        cuts.append(cuts[-1] + s)
    cuts.append(n)
    return cuts


# ------------------------------------------------------------------------------------------------ signals
def keyed_noise(rng, n, on_ranges, amp_on, amp_off=0.0, noise=1e-3):
    """one stream of n complex64 samples: weak noise, and a unit-modulus carrier of amplitude amp_on inside the index ranges
    (amp_off outside them)"""
    a = np.full(n, amp_off, np.float64)
    for lo, hi in on_ranges:
        a[lo:hi] = amp_on
    ph = np.exp(2j * np.pi * (0.013 * np.arange(n) + rng.random()))
    w = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (noise / math.sqrt(2))
    return (a * ph + w).astype(np.complex64)


def designed_keying(rng, fs, n_bins, decim, n_frames, plan, gain, noise=1e-4):
    """The bank tests' wideband input: carriers at bin centres keyed on and off, with amplitude steps 20 dB either side of
    their thresholds, over weak noise.
    plan: {bin: (threshold_db, [(frame_on, frame_off), ...])} -- a carrier on bin k at k fs / n_bins (bins above n_bins / 2:
    the negative frequencies) whose bin output stands 20 dB above the bin's threshold while it is keyed and 20 dB below it
    otherwise; gain: the bank's amplitude gain for a carrier at a bin centre (sum of the prototype's taps).
    -> complex64 [n_frames * decim]"""
    n = n_frames * decim
    t = np.arange(n, dtype=np.float64)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (noise / math.sqrt(2))
    for k, (thr_db, ranges) in sorted(plan.items()):
        amp = math.sqrt(threshold(thr_db + 20.0)) / gain
        env = np.full(n, math.sqrt(threshold(thr_db - 20.0)) / gain)
        for f_on, f_off in ranges:
            env[f_on * decim:f_off * decim] = amp
        kk = k if k < n_bins // 2 else k - n_bins
        x += env * np.exp(2j * np.pi * (kk / n_bins) * t + 2j * np.pi * rng.random())
    return x.astype(np.complex64)
