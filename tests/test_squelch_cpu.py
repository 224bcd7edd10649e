"""The carrier detector (rcf_chan_squelch, rcf_pfb_squelch) without a GPU: the kernels' arithmetic header
(radiocapture-rf_amd/csrc/squelch_core.hpp) compiled for the host -- plain, and once more under AddressSanitizer and UBSan, as
a stand-alone program -- and walked over the streams the numpy restatement (tests/squelch_ref.py) sees.  Its sequential form
equals the restatement bit for bit under ragged cuts; its segmented form (zero-state response, carry by a^S, second walk)
stays within the derived bound 64 x 2^-53 / alpha of it, with equal counters; a NaN mutes for good, an Inf stays open; the
threshold conversion; and the binding's names and sizes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import squelch_ref as R
from rcf import native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def check_programs():
    """squelch_core.hpp compiled for the host, plain and with the sanitizers: stand-alone programs"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(HERE, "native", "squelch_core_check.cpp")
    exes = []
    for name, extra in (("squelch_core_check", ["-O2"]),
                        ("squelch_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(out, name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-ffp-contract=off"] + extra
                              + [src, "-o", exe])
        exes.append(exe)
    return exes


def walk(exes, tmp_path, mode, x, thr_db, alpha, blocks, first_index=0, segment=None):
    """the checker's per-block lines, parsed; the plain and the sanitized program must print the same"""
    path = os.path.join(str(tmp_path), "x.cf32")
    np.asarray(x, np.complex64).tofile(path)
    args = [mode, path, float(thr_db).hex(), float(alpha).hex(), str(first_index)]
    if segment is not None:
        args.append(str(segment))
    args += [str(b) for b in blocks]
    outs = [subprocess.check_output([exe] + args, text=True) for exe in exes]
    assert outs[0] == outs[1]
    rows = []
    for line in outs[0].splitlines():
        f = line.split()
        rows.append(dict(level=float.fromhex(f[0]), n_seen=int(f[1]), n_open=int(f[2]), first_open=int(f[3]), last_open=int(f[4]),
                         unmuted=int(f[5])))
    assert len(rows) == len(blocks)
    return rows


def prefix(ref, n, first_index=0):
    """the restatement's state after its first n samples"""
    o = ref["open"][:n]
    idx = np.flatnonzero(o)
    return dict(level=float(ref["levels"][n - 1]) if n else 0.0, n_seen=n, n_open=int(o.sum()),
                first_open=int(idx[0]) + first_index if len(idx) else -1, last_open=int(idx[-1]) + first_index if len(idx) else -1,
                unmuted=int(o[-1]) if n else 0)


def same_float(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def keyed(seed, n, thr_db):
    """a carrier keyed on and off, 20 dB either side of the threshold, over weak noise"""
    rng = np.random.default_rng(seed)
    thr = R.threshold(thr_db)
    on = [(n // 9, n // 3), (n // 2, n // 2 + 3), (2 * n // 3, 5 * n // 6)]
    return R.keyed_noise(rng, n, on, amp_on=np.sqrt(100 * thr), amp_off=np.sqrt(thr / 100), noise=np.sqrt(thr) * 1e-3)


# ------------------------------------------------------------------------------------------------ the sequential form
@pytest.mark.parametrize("alpha, thr_db", [(0.1, -40.0), (1.0, -40.0), (0.01, -100.0), (0.37, 0.0)])
def test_sequential_form_equals_the_restatement_bit_for_bit_under_ragged_cuts(check_programs, tmp_path, alpha, thr_db):
    n = 1500
    x = keyed(11, n, thr_db)
    ref = R.run(x, R.threshold(thr_db), alpha, first_index=70)
    assert 0 < ref["n_open"] < n and R.margin(ref["levels"], R.threshold(thr_db)) > 0
    for sizes in ([n], [0, 1, 0, 63, 64, 65, 1, 1, 200, 0, 511], [1] * 40 + [7, 0, 300]):
        cuts = R.ragged_cuts(n, sizes)
        blocks = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
        rows = walk(check_programs, tmp_path, "seq", x, thr_db, alpha, blocks, first_index=70)
        for row, end in zip(rows, cuts[1:]):
            want = prefix(ref, end, 70)
            assert same_float(row.pop("level"), want.pop("level")), (sizes, end)
            assert row == want, (sizes, end)
    assert rows[-1]["n_open"] == int(ref["n_open"]) and rows[-1]["last_open"] == int(ref["last_open"])


# ------------------------------------------------------------------------------------------------ the segmented form
@pytest.mark.parametrize("alpha", [1.0, 0.1, 0.01])
def test_segmented_form_stays_within_the_derived_bound_and_counts_what_the_restatement_counts(check_programs, tmp_path, alpha):
    """blocks of 1, 2, 3 and 40 segments, a block whose last segment holds one frame, blocks of 0 and 1 frames and a segment
    short of one frame -- each entered at the level the blocks before left"""
    S, thr_db = 16, -40.0
    blocks = [S, 0, 2 * S, 1, 3 * S, S - 1, 40 * S, 2 * S + 1, S + 1, 5 * S + 3]
    n = sum(blocks)
    x = keyed(23, n, thr_db)
    thr = R.threshold(thr_db)
    ref = R.run(x, thr, alpha)
    assert 0 < ref["n_open"] < n
    assert R.margin(ref["levels"], thr) >= 1e-6            # a condition on the input: no level within rounding of its threshold
    rows = walk(check_programs, tmp_path, "seg", x, thr_db, alpha, blocks, segment=S)
    worst, end = 0.0, 0
    for row, b in zip(rows, blocks):
        end += b
        want = prefix(ref, end)
        got = row.pop("level")
        exact = want.pop("level")
        if end:
            worst = max(worst, abs(got - exact) / exact)
        assert row == want, end
    print("alpha %g: largest relative distance %.3g (bound %.3g)" % (alpha, worst, R.bound(alpha)))
    assert worst <= R.bound(alpha)


def test_one_segment_per_block_is_the_sequential_form_itself(check_programs, tmp_path):
    x = keyed(5, 300, -40.0)
    blocks = [100, 100, 100]
    a = walk(check_programs, tmp_path, "seq", x, -40.0, 0.1, blocks)
    b = walk(check_programs, tmp_path, "seg", x, -40.0, 0.1, blocks, segment=128)
    assert a == b


# ------------------------------------------------------------------------------------------------ NaN and Inf
@pytest.mark.parametrize("mode, segment", [("seq", None), ("seg", 16), ("seg", 512)])
def test_a_nan_mutes_for_good_and_an_inf_stays_open(check_programs, tmp_path, mode, segment):
    n = 400
    thr = R.threshold(-40.0)
    x = keyed(31, n, -40.0)
    blocks = [150, 1, 0, 249]
    # a NaN inside an open stretch: muted from there on, the level stays NaN, the counters stop
    xn = x.copy()
    assert R.run(x, thr, 0.1)["open"][60]
    xn[60] = complex(np.nan, 0.0)
    ref = R.run(xn, thr, 0.1)
    rows = walk(check_programs, tmp_path, mode, xn, -40.0, 0.1, blocks, segment=segment)
    assert np.isnan(ref["level"]) and all(np.isnan(r["level"]) for r in rows)
    assert [r["unmuted"] for r in rows] == [0, 0, 0, 0]
    assert rows[-1]["n_open"] == int(ref["n_open"]) == int(ref["open"][:60].sum()) and rows[-1]["last_open"] == int(ref["last_open"]) == 59
    # an Inf inside a closed stretch: open from there on, the level stays Inf (alpha < 1)
    xi = x.copy()
    assert not R.run(x, thr, 0.9)["open"][5]
    xi[5] = complex(np.inf, 0.0)
    ref = R.run(xi, thr, 0.9)
    rows = walk(check_programs, tmp_path, mode, xi, -40.0, 0.9, blocks, segment=segment)       # (0.1^512 underflows: the carry keeps the Inf)
    assert np.isposinf(ref["level"]) and all(np.isposinf(r["level"]) for r in rows)
    assert [r["unmuted"] for r in rows] == [1, 1, 1, 1]
    assert rows[-1]["n_open"] == int(ref["n_open"]) == n - 5 and rows[-1]["first_open"] == int(ref["first_open"]) <= 5
    # ... and with alpha 1 the sample behind it makes 0 x Inf, as GNU Radio's filter does
    ref = R.run(xi, thr, 1.0)
    rows = walk(check_programs, tmp_path, mode, xi, -40.0, 1.0, blocks, segment=segment)
    assert np.isnan(ref["level"]) and np.isnan(rows[-1]["level"]) and rows[-1]["n_open"] == int(ref["n_open"])


# ------------------------------------------------------------------------------------------------ constants and the binding
def test_threshold_conversion(check_programs):
    for exe in check_programs:
        out = subprocess.check_output([exe, "thr", "-100", "-40", "0"], text=True).split()
        assert [float.fromhex(v) for v in out] == [R.threshold(-100), R.threshold(-40), R.threshold(0)]
    assert R.threshold(0) == 1.0 and abs(R.threshold(-40) / 1e-4 - 1) < 1e-15 and abs(R.threshold(-100) / 1e-10 - 1) < 1e-15


def test_binding_names_sizes_and_segment():
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    for name in ("rcf_chan_squelch", "rcf_chan_squelch_state", "rcf_pfb_squelch", "rcf_pfb_squelch_read", "rcf_pfb_squelch_segment"):
        assert name in native.SYMBOLS and hasattr(native.lib(), name) and re.search(r"\b%s\s*\(" % name, hdr)
    assert C.sizeof(native.SquelchParams) == 16 and C.sizeof(native.SquelchState) == 48
    core = open(os.path.join(ROOT, "radiocapture-rf_amd", "csrc", "squelch_core.hpp")).read()
    seg = int(re.search(r"kSquelchSegment = (\d+);", core).group(1))
    assert native.pfb_squelch_segment() == seg == 256
    assert int(re.search(r"#define RCF_T_COUNT\s+(\d+)", hdr).group(1)) == 14          # the new launches are no timing class
    for fn in (native.Frontend.chan_squelch, native.Frontend.chan_squelch_state, native.Frontend.pfb_squelch, native.Frontend.pfb_squelch_read):
        assert callable(fn)
