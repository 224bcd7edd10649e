"""CPU side of the filterbank census (tests/pfb_census_ref.py, tests/test_gpu_pfb_census.py): the row table is held to the
shapes pfb_shape.h itself names (tests/native/pfb_shape_check.cpp, compiled here with g++, the way
tests/test_pfb_shape_table.py reads the header), the references are tested against the oracle's exact-phase channel, and
the gap test shows why the census exists: faults a relative rms over a bin of noise lets through, each caught exactly."""
import json
import os
import subprocess

import numpy as np
import pytest

import pfb_census_ref as P
from fir_census_ref import fir_reference, n_outputs
from oracle import grspec as G
from rcf import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FS = 20e6


def rel_rms(a, b):
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2) / np.mean(np.abs(b) ** 2)))


@pytest.fixture(scope="module")
def header_shapes():
    """what pfb_shape.h answers over the grid of tests/golden/pfb_shapes.json: {(NB, D, P): (family, Ppad, chunk_frames)}
    for every supported shape"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "pfb_shape_check_census")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc"),
                           os.path.join(HERE, "native", "pfb_shape_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    shapes = {}
    for NB, D, ntaps, supported, family, Ppad, chunk, *_ in json.loads(p.stdout.decode())["rows"]:
        if supported:
            shapes[(NB, D, -(-ntaps // NB))] = (family, Ppad, chunk)
    assert len(shapes) == 200              # (400 supported rows: two prototype lengths per taps-per-branch count)
    return shapes


def test_rows_reach_every_instantiation_the_header_can_answer(header_shapes):
    """a new shape in pfb_shape.h without a row fails here"""
    header = {(fam, NB, NB // D, Ppad) for (NB, D, _), (fam, Ppad, _) in header_shapes.items()}
    rows = {(r.family, r.NB, r.OS, r.Ppad) for r in P.PFB_ROWS}
    assert header - rows == set(), "shapes without a census row: %s" % sorted(header - rows)
    assert rows - header == set(), "rows the header does not know: %s" % sorted(rows - header)
    assert len(P.PFB_ROWS) == 5 * 5 + 16 + 12 and len({P.row_id(r) for r in P.PFB_ROWS}) == len(P.PFB_ROWS)
    for r in P.PFB_ROWS:
        assert header_shapes[(r.NB, r.D, r.P)] == (r.family, r.Ppad, r.chunk), r
    # family 3 runs a one-row prototype beside a row of zeros
    assert sorted(r.NB for r in P.PFB_ROWS if r.family == 3 and r.P == 1) == sorted(a * b for a, b in P.PFBM_SHAPES)
    # the coded test takes the smallest row count of every bin count, and every bin count
    smallest = {}
    for (NB, D, _), (_, Ppad, _) in header_shapes.items():
        smallest[NB] = min(smallest.get(NB, 99), Ppad)
    assert {s[0] for s in P.CODED_SHAPES} == set(smallest)
    for NB, OS, Ppad, all_bins in P.CODED_SHAPES:
        assert Ppad == smallest[NB] and any(k[0] == NB and k[1] == NB // OS and v[1] == Ppad for k, v in header_shapes.items())
        assert all_bins == (NB <= 400)


def test_rows_cut_against_chunk_and_zero_history_boundary():
    for r in P.PFB_ROWS:
        F, zh = r.chunk, P.launches_zero_history(r)
        assert r.T % r.NB != 0 and -(-r.T // r.NB) == r.P and r.lead % r.D != 0
        assert 190 <= sum(r.n_frames) <= 260, (P.row_id(r), sum(r.n_frames))
        steady = [c for c, z in zip(r.n_frames, zh) if z is False]
        assert {1, F - 1, F, F + 1, 3 * F + 5} <= set(steady), P.row_id(r)        # ... and several chunks plus a remainder
        assert 0 in r.n_frames and all(n < r.D for c, n in zip(r.n_frames, r.cuts) if c == 0)
        # the last masking launch is directly followed by the first launch that no longer reaches before the start, and
        # that one begins exactly at the boundary
        real = [(c, z) for c, z in zip(r.n_frames, zh) if c]
        first = next(i for i, (_, z) in enumerate(real) if not z)
        assert first >= 1 and real[first - 1] == (1, True) and all(not z for _, z in real[first:])
        assert sum(c for c, _ in real[:first]) == r.zh_frames
        k0 = -(-r.lead // r.D)
        assert P.zero_history(r.NB, r.D, r.Ppad, k0 + r.zh_frames - 1, r.lead)
        assert not P.zero_history(r.NB, r.D, r.Ppad, k0 + r.zh_frames, r.lead)
        # the ring of the GPU test holds every push and wraps
        assert max(r.n_frames) <= P.RING < sum(r.n_frames) // 3


def test_partial_sums_stay_exact_in_float32():
    for r in P.PFB_ROWS:
        assert P.row_bound(r) == r.T * 49 * 2 < 2 ** 24, P.row_id(r)
    for NB, OS, Ppad, _ in P.CODED_SHAPES:
        assert NB * Ppad < 2 ** 24 and NB * Ppad <= 16384
    P.rider_case(np.random.default_rng(1))                # (asserts every intermediate itself)
    c = P.fm_case(np.random.default_rng(2))
    assert c["exact"].all() and len(c["fm"]) == len(c["y0"]) == sum(c["n_frames"])


@pytest.mark.parametrize("row", range(len(P.PFB_ROWS)), ids=lambda i: P.row_id(P.PFB_ROWS[i]))
def test_census_bin0_equals_the_exact_phase_channel_at_offset_zero(row):
    r = P.PFB_ROWS[row]
    x, h, y = P.bank_census(r, np.random.default_rng(5000 + row))
    xz = x.copy()
    xz[:r.lead] = 0
    k0 = -(-r.lead // r.D)
    ref = G.xlating_fir_exact(xz, r.D, h, 0.0, FS)[k0:]
    assert np.array_equal(y.astype(np.complex128), ref)
    assert len(y) == sum(r.n_frames) and np.abs(y).max() > 0


@pytest.mark.parametrize("shape", [(64, 1, 4), (192, 2, 2), (400, 2, 1), (512, 2, 4)], ids=lambda s: "%d_os%d_p%d" % s)
def test_coded_expectation_equals_the_exact_phase_channel(shape):
    NB, OS, Ppad = shape
    D = NB // OS
    bins = [0, 1, 7, NB // 2, NB - 1]
    x, h, tap, want = P.coded_bank(NB, D, Ppad, bins=bins)
    assert want.shape == (n_outputs(len(x), D), len(bins))
    for j, k in enumerate(bins):
        ref = G.xlating_fir_exact(x, D, h, (k if k <= NB // 2 else k - NB) * FS / NB, FS)
        # float64 phases of arguments up to 2 pi T and 2 pi frames: a few 1e-13 of the code
        assert np.abs(want[:, j] - ref).max() < 1e-9 * len(h), (NB, k, float(np.abs(want[:, j] - ref).max()))
    got_tap, _ = P.decode_bank(want)
    assert np.array_equal(got_tap, np.broadcast_to(tap[:, None], want.shape))
    assert np.all(want[tap < 0] == 0)


@pytest.mark.parametrize("shape", P.CODED_SHAPES, ids=lambda s: "%d_os%d_p%d" % s[:3])
def test_coded_stream_is_sound(shape):
    NB, OS, Ppad, all_bins = shape
    D = NB // OS
    bins = None if all_bins else P.spread_bins(NB)
    x, h, tap, want = P.coded_bank(NB, D, Ppad, bins=bins)
    T = len(h)
    pos = np.flatnonzero(x)
    assert len(pos) == D and np.all(x[pos] == 1)
    # no frame's window [n D - T + 1, n D] holds two impulses
    n = np.arange(len(tap), dtype=np.int64)
    seen = np.searchsorted(pos, n * D, side="right") - np.searchsorted(pos, n * D - T + 1, side="left")
    assert seen.max() == 1 and np.array_equal(seen == 1, tap >= 0)
    # every tap exactly once per bin
    assert np.array_equal(np.bincount(tap[tap >= 0], minlength=T), np.ones(T, dtype=np.int64))
    # every (branch, bin) pair of the NB x NB matrix
    assert T >= NB and set(tap[tap >= 0] % NB) == set(range(NB))
    ks = list(range(NB)) if bins is None else bins
    assert want.shape[1] == len(ks) == (NB if all_bins else 64)
    assert {1, NB // 2 - 1, NB // 2, NB // 2 + 1, NB - 1} <= set(ks)
    if not all_bins:
        assert {k // 64 for k in ks} == set(range(-(-NB // 64)))                   # every aligned run of 64 bins
        if NB in P.PFB1_NB:
            assert {k % (NB // 16) // 4 for k in ks} == set(range(NB // 64))       # every wave of pfb.hip's epilogue


def _proto(m):
    if m.proto == "lp2":
        bw = FS / m.NB
        return G.low_pass_2(1.0, FS, bw * 0.4, bw * 0.2, 60.0, G.WIN_BLACKMAN_HARRIS)
    D, taps = G.channel_params(FS, 12500)
    assert D == m.D
    return taps


@pytest.mark.parametrize("mi", range(len(P.MUTATIONS)), ids=lambda i: P.MUTATIONS[i].name.replace(" ", "_"))
def test_the_gap_a_relative_rms_bar_passes_what_the_census_catches(mi):
    """each mutation on the existing tests' stimulus (unit noise, 150 frames, the shape's own prototype) stays UNDER the
    existing bar -- today's tests would pass it -- and the census differs from it in every affected frame.  Where the
    error's expectation sits AT the bar the draw decides the inequality (pfb_census_ref.MUTATIONS says which, and how the
    draw was taken); the expectation itself is held here as well, so that nobody reads more into the draw than it holds."""
    m = P.MUTATIONS[mi]
    proto = _proto(m)
    T, NB, D = len(proto), m.NB, m.D
    Pb = -(-T // NB)
    if m.name.startswith("256 bins"):
        assert (T, Pb) == (3491, 14)
    if m.proto == "chan":
        assert T == 2909
    x = synth.awgn(np.random.default_rng(m.seed), D * P.GAP_FRAMES).astype(np.complex64)
    clean = fir_reference(x, proto.astype(np.float64), D)[0]
    bad, _ = P.mutated_bin0(x, proto.astype(np.float64), D, NB, m.kind, m.arg)
    err, expect = rel_rms(bad, clean), P.expected_rel_rms(m, proto)
    print("%s: relative rms %.2e on this draw, %.2e in expectation, bar %.0e" % (m.name, err, expect, m.bar))
    assert 0 < err < m.bar
    if m.at_bar:
        assert 0.9 * m.bar < expect < 1.1 * m.bar
    else:
        assert expect < m.bar / 3 and err < m.bar / 3
    rng = np.random.default_rng(400 + mi)
    if m.kind == "row":
        # bin 0 of the integer census: every frame at that chunk position differs, no other does
        xi, hi, _, _, y = P.simple_census(rng, NB, D, T, [150])
        ym, hit = P.mutated_bin0(xi, hi.astype(np.float64), D, NB, m.kind, m.arg)
        diff = ym != y.astype(np.complex128)
        assert len(hit) >= 9 and diff[hit].all() and diff.sum() == len(hit)
        return
    # a prototype edit: the coded impulses name it in every frame that reads an edited tap, at every bin looked at
    Ppad = next(v[1] for v in ((r.NB, r.Ppad) for r in P.PFB_ROWS if r.NB == NB and r.D == D) if v[1] >= Pb)
    bins = None if NB <= 400 else P.spread_bins(NB)
    _, h, tap, want = P.coded_bank(NB, D, Ppad, T=T, bins=bins)
    _, _, _, want_m = P.coded_bank(NB, D, Ppad, T=T, bins=bins, taps=P.mutate_taps(h, m.kind, m.arg))
    edited = np.arange(m.arg) if m.kind == "drop" else np.array([T - 2, T - 1])
    hit = np.isin(tap, edited)
    assert hit.sum() == len(edited)
    got_tap, _ = P.decode_bank(want_m)
    assert np.all(got_tap[hit] != tap[hit, None]) and np.array_equal(got_tap[~hit], np.broadcast_to(tap[:, None], want.shape)[~hit])
    if m.kind == "drop":
        # ... and bin 0 of the integer census sees it too (the first tap is never zero)
        xi, hi, _, _, y = P.simple_census(rng, NB, D, T, [150])
        ym, _ = P.mutated_bin0(xi, hi.astype(np.float64), D, NB, m.kind, m.arg)
        assert np.count_nonzero(ym != y.astype(np.complex128)) > 140
