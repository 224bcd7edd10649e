"""CPU side of the FIR census (tests/fir_census_ref.py, tests/test_gpu_fir_census.py): the Python restatement of the
matrix-core planner is pinned to rcf_internal.h itself (tests/native/mfma_plan_check.cpp, compiled here with g++), the GPU
shape table is held to reach every (NT, parts) the planner can answer, and the references are tested on themselves."""
import os
import subprocess

import numpy as np
import pytest

import fir_census_ref as R
from oracle import cbind as OC
from oracle import grspec as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# every chunk boundary 64 c - 1 | 64 c of bank2_steps and both parities next to and between them
PLAN_TS = sorted({t for c in range(1, 11) for t in (64 * c - 1, 64 * c, 64 * c + 1, 64 * c + 32, 64 * c + 33) if 64 <= t <= 640})
PLAN_CHANS = [8, 9, 31, 32, 33, 64, 65, 100, 160, 200, 256, 512]
PLAN_NKS = list(range(1, 141)) + list(range(140, 4201, 20))


def _build(name, extra=()):
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", *extra,
                           "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc"), "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", os.path.join(HERE, "native", "mfma_plan_check.cpp"), "-o", exe])
    return exe


def _ask(exe, triples):
    p = subprocess.run([exe], input="".join("%d %d %d\n" % t for t in triples).encode(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    rows = [tuple(int(v) for v in line.split()) for line in p.stdout.decode().splitlines()]
    assert len(rows) == len(triples) and all(r[:3] == t for r, t in zip(rows, triples))
    return rows


@pytest.fixture(scope="module")
def header_answers():
    """what rcf_internal.h answers over the grid: {(n_chans, n_k, T): (steps, nt, parts, applicable)}"""
    triples = [(c, k, T) for T in PLAN_TS for c in PLAN_CHANS for k in PLAN_NKS]
    triples += [(8, 1, T) for T in range(1, 700)]                       # bank2_steps at every length
    triples += [(r[2], nk, r[0]) for r in R.MFMA_ROWS for nk in r[3]]   # and the GPU table's own launches
    return {r[:3]: r[3:] for r in _ask(_build("mfma_plan_check"), triples)}


def test_planner_restatement_equals_the_header(header_answers):
    bad = [(t, got, (R.bank2_steps(t[2]),) + R.mfma_plan(*t))
           for t, got in header_answers.items() if got[:3] != (R.bank2_steps(t[2]),) + R.mfma_plan(*t)]
    assert not bad, bad[:10]
    bad = [t for t, got in header_answers.items() if bool(got[3]) != R.mfma2_applicable(1, t[2], 1 << 16, (1 << 16) + (1 << 22))]
    assert not bad, bad[:10]
    assert len(header_answers) > 180000
    # the chunk count steps exactly between 64 c - 1 and 64 c
    for c in range(1, 11):
        assert R.n_chunks(64 * c) == R.n_chunks(64 * c - 1) + 1 == c + 1, c
    assert not R.mfma2_applicable(1, 63, 1 << 16, 1 << 22) and R.mfma2_applicable(1, 64, 1 << 16, 1 << 22)


def test_gpu_table_reaches_every_plan_the_planner_can_answer(header_answers):
    grid = {t: v for t, v in header_answers.items() if t[0] in PLAN_CHANS and t[2] in PLAN_TS}
    reachable = {(v[1], v[2]) for v in grid.values()}
    table = R.plans_of(R.MFMA_ROWS)
    for _, _, T, c, nk, plan in table:                                   # the table's plans are the header's own
        assert header_answers[(c, nk, T)][1:3] == plan
    reached = {p[5] for p in table}
    print("reachable:", sorted(reachable))
    for i, j, T, c, nk, plan in table:
        print("row %2d push %d: T %3d (%d chunks) x %3d channels x %4d outputs -> NT %d, parts %d%s"
              % (i, j, T, R.n_chunks(T), c, nk, plan[0], plan[1], "  (uneven)" if R.uneven_split(T, plan[1]) else ""))
    assert reachable - reached == set(), sorted(reachable - reached)
    assert {1, 2} == {p[0] for p in reachable} and (1, 1) in reachable and (2, 1) in reachable
    # parts that do not divide the chunks: c_first = part * chunks / parts takes parts of different lengths
    for parts in (3, 5, 7, 8):
        assert any(p[5][1] == parts and R.uneven_split(p[2], parts) for p in table), parts
    # both tap parities and both sides of a chunk boundary run on the matrix cores
    Ts = {r[0] for r in R.MFMA_ROWS}
    assert any(T % 2 == 0 for T in Ts) and any(T % 2 == 1 for T in Ts)
    assert any(T % 64 == 63 for T in Ts) and any(T % 64 == 0 for T in Ts)
    assert all(R.mfma2_applicable(r[1], r[0], 1 << 16, (1 << 16) + (1 << 22)) and r[2] >= R.K_M2_MIN_CHANS for r in R.MFMA_ROWS)
    # the decimations and the pushes' output counts the issue asks for
    assert {r[1] for r in R.MFMA_ROWS} == {1, 2, 3, 4, 5, 8}
    for D in (1, 3):
        assert any(r[1] == D and p[0] == i and p[5][0] == 2 for i, r in enumerate(R.MFMA_ROWS) for p in table), D
    nks = {(p[5][0], p[4]) for p in table}
    assert {1, 15, 16, 17} <= {nk for _, nk in nks}
    for nt in (1, 2):
        for d in (-1, 0, 1):
            assert any(n == nt and (nk - d) % (64 * nt) == 0 and nk > 1 for n, nk in nks), (nt, d)
    for r in R.MFMA_ROWS:
        assert max(R.cuts_for(r[3], r[1])) <= 21000
        n = np.cumsum(R.cuts_for(r[3], r[1]))
        assert [R.n_outputs(int(b), r[1]) - R.n_outputs(int(a), r[1]) for a, b in zip(np.r_[0, n[:-1]], n)] == r[3]
    # the ring-wrap row: a push's outputs straddle the ring's end inside a 16-output tile of the launch
    r = next(r for r in R.MFMA_ROWS if r[4] == 1 << 11)
    ends = np.cumsum(r[3])
    assert any(a < r[4] < b and (r[4] - a) % 16 for a, b in zip(np.r_[0, ends[:-1]], ends))
    for i, j, T, c, nk, plan in R.plans_of(R.COMPLEX_ROWS):
        assert any(q[2:] == (T, c, nk, plan) for q in table)             # rows of the table, run again
    cp = {p[5] for p in R.plans_of(R.COMPLEX_ROWS)}
    assert any(p[1] == 1 for p in cp) and any(p[0] == 2 for p in cp)


def test_check_program_is_clean_under_sanitizers():
    exe = _build("mfma_plan_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                          "-fno-omit-frame-pointer"])
    triples = [(c, k, T) for T in (64, 127, 128, 449, 512, 640) for c in (8, 33, 512) for k in (1, 17, 129, 4000)]
    rows = _ask(exe, triples)
    assert [r[4:6] for r in rows] == [R.mfma_plan(*t) for t in triples]


def test_reference_sees_one_flipped_tap_in_exactly_its_outputs():
    rng = np.random.default_rng(1)
    T, D, C, n = 127, 3, 5, 2000
    x, taps, y = R.census(rng, T, D, C, n, 7, 7)
    assert y.shape == (C, R.n_outputs(n, D)) and y.dtype == np.complex64
    assert len({t.tobytes() for t in taps}) == C and np.all(taps == np.rint(taps)) and np.abs(taps).max() <= 7
    # the float64 matmul equals integer arithmetic
    k = 411
    want = sum(int(taps[2, t]) * complex(x[k * D - t]) for t in range(T))
    assert y[2, k] == want
    for c, t in ((0, 0), (3, T - 1), (4, 64)):
        t2 = taps.copy()
        t2[c, t] += 1
        y2 = R.fir_reference(x, t2, D).astype(np.complex64)
        ks = np.arange(y.shape[1])
        touched = (ks * D - t >= 0) & (x[np.clip(ks * D - t, 0, n - 1)] != 0)     # the window holds the tap on a non-zero sample
        changed = y2 != y
        assert not changed[np.arange(C) != c].any()
        assert np.array_equal(changed[c], touched), (c, t)
    # zero history: samples before a channel's start do not count, and its outputs start on the absolute grid
    start = 1001
    ys = R.fir_reference(x, taps, D, start=start)
    xz = x.copy()
    xz[:start] = 0
    assert np.array_equal(ys, R.fir_reference(xz, taps, D)[:, -(-start // D):])
    with pytest.raises(AssertionError):
        R.census(rng, 1 << 18, 1, 1, 8, 7, 7)                              # the 2^24 guard


def test_coded_variant_decodes_to_channel_and_tap_at_every_output():
    T, D, C = 449, 2, 65
    n = 3 * 449 + 17
    x, taps, want = R.coded(T, D, C, n, range(0, n, T))
    assert taps.max() < 2 ** 19 and (want >= 0).all()                      # impulses T apart: every window holds exactly one
    y = R.fir_reference(x, taps, D).astype(np.complex64)
    c, t = R.decode(y)
    assert np.array_equal(c, np.broadcast_to(np.arange(C)[:, None], c.shape)) and np.array_equal(t, np.broadcast_to(want, t.shape))
    assert set(want) == set(range(T))                                      # odd T, D = 2: the impulses alternate the parity
    # a packer that dropped the last tap: those outputs decode to "none", and the decoder says so
    t3 = taps.copy()
    t3[:, T - 1] = 0
    c3, t3d = R.decode(R.fir_reference(x, t3, D).astype(np.complex64))
    assert np.array_equal(t3d[0] != want, want == T - 1) and (t3d[0][want == T - 1] == -1).all()
    # outputs whose parts disagree are flagged, not decoded
    assert R.decode(np.array([3 + 4j, -2 - 2j, 2.5 + 2.5j]))[0].tolist() == [-2, -2, -2]
    x2, _, w2 = R.coded(T, D, C, n, [700])
    assert (w2 >= 0).sum() == -(-T // D) and w2[350] == 0 and w2[349] == -1


def test_offset_zero_is_an_exact_identity_rotator():
    taps = np.arange(1, 9, dtype=np.float32)
    ct, incr = OC.xlating_composite(taps, 4, 0.0, 1e6)
    assert np.array_equal(ct, taps.astype(np.complex64)) and incr.real == 1 and incr.imag == 0
    ph, _, _ = G.rotator_phases(incr, 3000)
    assert np.all(ph == 1)
    assert np.all(R.closed_form_phases(incr, 3000) == 1)


def test_rotator_allowance_is_recorded_and_under_the_iq_bar():
    incs = R.complex_increments()
    n = 4400
    assert max(sum(r[3]) for r in R.COMPLEX_ROWS) <= n
    assert all(np.array_equal(G.rotator_phases(i, 700)[0], OC.rotator_phases(i, 700)) for i in incs)   # the C restatement iterates alike
    measured = R.rotator_allowance(incs, n)
    print("rotator allowance: measured %.3e, recorded %.3e, used %.3e" % (measured, R.ROTATOR_ALLOWANCE_MEASURED, R.ROTATOR_ALLOWANCE))
    assert 0.9 * R.ROTATOR_ALLOWANCE_MEASURED <= measured <= R.ROTATOR_ALLOWANCE_MEASURED
    assert R.ROTATOR_ALLOWANCE == 2 * R.ROTATOR_ALLOWANCE_MEASURED + 2.0 ** -22 < 1e-5
    assert "%.1e" % R.ROTATOR_ALLOWANCE_MEASURED in R.__doc__


def test_summation_bound_holds_for_float32_sums_in_any_order():
    """the derived bound against float32 sums done on the CPU in the orders the oracle knows (sequential, 8 and 16 lanes,
    pairwise): a bound that one of them broke would be wrong, one that is orders of magnitude above all of them useless"""
    rng = np.random.default_rng(4)
    T, D, n = 449, 2, 3000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    taps = rng.standard_normal(T).astype(np.float32)
    ct, _ = OC.xlating_composite(taps, D, 212500.0, 1e6)
    exact = R.fir_reference(x, ct[None, :], D)[0]
    bound = R.summation_bound(ct, x, D, T, 7)[0]
    worst = 0.0
    for mode in (OC.SUM_SEQUENTIAL, OC.SUM_8_LANES, OC.SUM_16_LANES, OC.SUM_PAIRWISE):
        err = np.abs(OC.fir_summation(x, D, ct, mode).astype(np.complex128) - exact)
        assert (err <= bound).all(), mode
        worst = max(worst, float((err / bound).max()))
    assert worst > 1e-3, worst
    # worst case over 2 T terms, so ~1e-3 of a typical output: loose against rounding, two orders under a wrong sign
    assert (bound < 1e-2 * np.abs(exact).mean()).all()


def test_chain_case_is_exact_and_the_discriminator_oracle_does_not_depend_on_fusing():
    """The chained census feeds quadrature_demod_cf integer IQ: y[k] conj(y[k-1]) is then two exact products and an exact sum
    per component (below 2^24), so a fused multiply-add gives the same bits as GNU Radio's unfused form -- shown here by doing
    the products in float64 -- and the oracle's two statements of fast_atan2f (numpy selects, C branches) agree on them."""
    x, cuts, parents, children = R.chain_case(np.random.default_rng(11))
    assert np.abs(x.real).max() == 1 and len(children) == 2 * 12
    for tp, yp in parents:
        assert np.abs(yp.real).max() <= 8 and np.abs(yp.imag).max() <= 8
    for pi, T, D, tc, yc, fm in children:
        assert len(yc) == R.n_outputs(len(parents[pi][1]), D) == len(fm)
        a = yc.astype(np.complex128)
        b = np.concatenate([[0], a[:-1]])
        p = a * np.conj(b)                                                  # float64: exact for these integers
        assert np.abs(p.real).max() < 2 ** 24 and np.abs(p.imag).max() < 2 ** 24
        assert np.array_equal(p.real.astype(np.float32), p.real) and np.array_equal(p.imag.astype(np.float32), p.imag)
        fused_free = G.fast_atan2f(p.imag.astype(np.float32), p.real.astype(np.float32))
        assert np.array_equal(fused_free.view(np.uint32), fm.view(np.uint32)), (T, D)
        assert np.array_equal(OC.quad_demod(yc, 1.0).view(np.uint32), fm.view(np.uint32)), (T, D)
        assert np.abs(fm).max() > 1.0                                       # not a stream of zeros
