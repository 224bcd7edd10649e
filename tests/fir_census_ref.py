"""References for the exact census of the stage-2 FIR kernels (radiocapture-rf_amd/csrc/fir.hip): fir_mfma_kernel with its
split-K finish and the operand packer, the vector kernel fir_bank_kernel, and fir_small_kernel.  CPU only.

The idea.  A channel opened at offset 0 has composite taps equal to its real taps and a rotator increment of exactly
(1, -0): the rotator multiplies by 1.  If the taps and the samples are small integers, every partial sum of
    y[c, k] = sum_t taps[c, t] * x[k D - t]            (x before the channel's start sample counts as zero)
is an integer below 2^24, float32 arithmetic is exact in any order -- fused or not, split-K or not, matrix cores or vector
lanes -- and the GPU's output must equal the integer reference bit for bit under every launch plan.  One missing, doubled
or misplaced tap shows in a named output.

  mfma_plan, bank2_steps   the planner of rcf_internal.h restated (tests/test_fir_census_cpu.py pins them to the header)
  census                   random small-integer stream and per-channel taps with the exact reference
  coded                    taps[c, t] = 1 + t + 1024 c against unit impulses: every output IS the code of the tap it read
  summation_bound          the classical bound for the float32 sum when taps and samples are not integers (derived)
  rotator_allowance        how far GNU Radio's iterated float32 rotator strays from the closed form of rotator.hpp
  MFMA_ROWS                the shape table of tests/test_gpu_fir_census.py (here, so that the CPU test can hold its coverage)

Rotator allowance, as measured by rotator_allowance() on the CPU for the increments of COMPLEX_ROWS (offsets
COMPLEX_OFFSETS_HZ at 1 MHz, every decimation of the rows, 4400 outputs): 2.0e-06 at the largest (|deviation| of a unit
phasor; the offsets are the ones of a 6.25 kHz grid where the iteration strays least -- at some, such as 118.75 kHz with
D = 5, its rounding is biased and it reaches 3.7e-05).  The tests use 2 x that + 2^-22 = 4.24e-06, under the project's
1e-5 bar for channel IQ, and multiply it by |v_ref[k]|: it is RELATIVE to each output and only admits the reference's own
random walk.  The summation bound beside it is the worst case over 2 T terms, about 1e-3 of a typical output at 449 taps:
the allowance is a few thousandths of the tolerance and cannot be what makes a complex-tap case pass.
tests/test_fir_census_cpu.py::test_rotator_allowance_is_recorded_and_under_the_iq_bar prints the figure and holds this
docstring to it."""
import math

import numpy as np

K_M2_GROUP = 32          # rcf_internal.h kM2Group
K_M2_CHUNK_STEPS = 8     # kM2ChunkSteps
K_M2_MIN_CHANS = 8       # kM2MinChans


def bank2_steps(T):
    s = ((T // 2 + 1) + 3) // 4
    return (s + K_M2_CHUNK_STEPS - 1) // K_M2_CHUNK_STEPS * K_M2_CHUNK_STEPS


def n_chunks(T):
    return bank2_steps(T) // K_M2_CHUNK_STEPS


def mfma_plan(n_chans, n_k, T):
    """-> (nt, parts), rcf_internal.h mfma_plan operation for operation (the comparisons are on doubles)"""
    groups = (n_chans + K_M2_GROUP - 1) // K_M2_GROUP
    chunks = n_chunks(T)
    best, best_cost = (1, 1), 1e300
    for nt in (1, 2):
        wgs = groups * ((n_k + 64 * nt - 1) // (64 * nt))
        parts = 1
        while parts <= 8 and parts <= chunks:
            rounds = (wgs * parts + 511) // 512
            cost = float(rounds) * nt / parts * (0.94 if nt == 2 else 1.0)
            if parts > 1:
                cost += 0.06 + 0.01 * parts
            if cost < best_cost - 1e-9:
                best_cost, best = cost, (nt, parts)
            parts += 1
    return best


def mfma2_applicable(D, T, hist_cap, buf_samples):
    return D >= 1 and T >= 64 and 8 * bank2_steps(T) + 8 + D <= hist_cap and buf_samples * 8 < (1 << 31)


def uneven_split(T, parts):
    """the part boundaries c_first = part * chunks / parts of fir_mfma_kernel are not all the same length"""
    return n_chunks(T) % parts != 0


# ---------------------------------------------------------------------------------------------- exact reference
def n_outputs(n_samples, D):
    """outputs k = 0 .. with k D < n_samples: output k exists as soon as sample k D does"""
    return 0 if n_samples <= 0 else (n_samples - 1) // D + 1


def fir_reference(x, taps, D, start=0):
    """y[c, j] = sum_t taps[c, t] x[(k0 + j) D - t], k0 = ceil(start / D), x[s] = 0 for s < start: float64 (complex128)
    matmul over a sliding window.  Exact when every partial sum is an integer below 2^53; taps real or complex, one row
    per channel."""
    x = np.asarray(x)
    taps = np.atleast_2d(np.asarray(taps))
    T = taps.shape[1]
    k0 = -(-start // D)
    n_out = n_outputs(len(x), D)
    xz = x.astype(np.complex128)
    xz[:start] = 0
    xp = np.concatenate([np.zeros(T - 1, np.complex128), xz])
    cplx = np.iscomplexobj(taps)
    rev = np.ascontiguousarray(taps[:, ::-1].astype(np.complex128 if cplx else np.float64).T)   # rev[j, c] = taps[c, T-1-j]
    out = np.empty((taps.shape[0], max(0, n_out - k0)), np.complex128)
    for a in range(k0, n_out, 2048):
        b = min(n_out, a + 2048)
        w = xp[(np.arange(a, b) * D)[:, None] + np.arange(T)[None, :]]        # w[j, i] = x[k D - (T-1) + i]
        if cplx:
            y = w @ rev
        else:                                                                  # two real products: exact for integers
            y = (w.real @ rev) + 1j * (w.imag @ rev)
        out[:, a - k0:b - k0] = y.T
    return out


def int_stream(rng, n, x_max):
    return (rng.integers(-x_max, x_max + 1, n) + 1j * rng.integers(-x_max, x_max + 1, n)).astype(np.complex64)


def int_taps(rng, n_chans, T, tap_max):
    """one int-valued float32 tap vector per channel, all different, first and last tap never zero (a dropped end tap
    must change the sum)"""
    assert n_chans == 1 or (2 * tap_max) ** T >= 4 * n_chans, "too few different tap vectors: raise tap_max"
    taps = np.zeros((n_chans, T), np.float32)
    seen = set()
    for c in range(n_chans):
        while True:
            t = rng.integers(-tap_max, tap_max + 1, T).astype(np.float32)
            for col in (0, T - 1):
                if t[col] == 0:
                    t[col] = tap_max if rng.integers(2) else -tap_max
            if t.tobytes() not in seen:
                break
        seen.add(t.tobytes())
        taps[c] = t
    return taps


def census(rng, T, D, n_chans, n, x_max, tap_max):
    """-> (x complex64[n], taps float32[n_chans, T], y complex64[n_chans, n_outputs]) with y exact"""
    assert T * 2 * x_max * tap_max < 2 ** 24, "partial sums must stay exact in float32"
    x = int_stream(rng, n, x_max)
    taps = int_taps(rng, n_chans, T, tap_max)
    y = fir_reference(x, taps, D)
    assert np.abs(y.real).max(initial=0) < 2 ** 24 and np.abs(y.imag).max(initial=0) < 2 ** 24
    return x, taps, y.astype(np.complex64)


# ---------------------------------------------------------------------------------------------- coded variant
CODE_T, CODE_C = 1024, 512


def coded_taps(n_chans, T):
    assert n_chans <= CODE_C and T <= CODE_T
    return (1 + np.arange(T)[None, :] + CODE_T * np.arange(n_chans)[:, None]).astype(np.float32)


def coded(T, D, n_chans, n, positions):
    """-> (x, taps, want): x = unit impulses 1 + 1j at `positions` (at least T apart, so that no window holds two);
    want[k] = the tap index output k reads (-1: none, the output is zero).  Output k of channel c is then
    (1 + 1j) (1 + want[k] + 1024 c)."""
    positions = sorted(positions)
    assert all(b - a >= T for a, b in zip(positions, positions[1:])) and 0 <= positions[0] and positions[-1] < n
    x = np.zeros(n, np.complex64)
    x[positions] = 1 + 1j
    k = np.arange(n_outputs(n, D))
    want = np.full(len(k), -1)
    for p in positions:
        t = k * D - p
        hit = (t >= 0) & (t < T)
        want[hit] = t[hit]
    return x, coded_taps(n_chans, T), want


def decode(y):
    """complex outputs of a coded run -> (channel, tap) arrays, (-1, -1) where the output is zero; the real and the
    imaginary part must carry the same code (anything else decodes to (-2, -2))"""
    y = np.asarray(y)
    re, im = np.rint(y.real).astype(np.int64), np.rint(y.imag).astype(np.int64)
    ok = (re == y.real) & (im == y.imag) & (re == im) & (re >= 0)
    c = np.where(re > 0, (re - 1) // CODE_T, -1)
    t = np.where(re > 0, (re - 1) % CODE_T, -1)
    return np.where(ok, c, -2), np.where(ok, t, -2)


# ---------------------------------------------------------------------------------------------- complex taps: bounds
def summation_bound(ct, x, D, T, parts):
    """Per output, a bound on |float32 result - exact value| of v[k] = sum_t ct[t] x[k D - t] and the rotator multiply
    behind it.  Each component is a sum of 2 T products, accumulated by fused multiply-adds (one rounding each) in `parts`
    chains that are then added (parts - 1 roundings), and the rotator's complex multiply is two products and a sum per
    component of a value bounded by the same sums of magnitudes (4 roundings more):
        |err Re| <= (2 T + parts + 4) 2^-24 sum_t (|Re ct||Re x| + |Im ct||Im x|)
        |err Im| <= (2 T + parts + 4) 2^-24 sum_t (|Re ct||Im x| + |Im ct||Re x|)
    (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: any order of summing n terms is within (n - 1) u of
    the sum of magnitudes to first order, so the vector kernel's 64 lane chains are covered as well; the second-order
    term n^2 u^2 < 1e-8 relative is absorbed by the + 4.)  The rotation turns the error vector without stretching it
    (|phase| = 1 + O(1e-5)), so the bound on the complex error is the hypotenuse.  Evaluated in float64.
    ct: composite taps, one row per channel; parts: a number or one per output.  -> float64[channels, outputs]"""
    ct = np.atleast_2d(np.asarray(ct)).astype(np.complex128)
    assert ct.shape[1] == T
    a, b = np.abs(ct.real), np.abs(ct.imag)
    xr = np.abs(np.asarray(x).real.astype(np.float64)) + 0j
    xi = np.abs(np.asarray(x).imag.astype(np.float64)) + 0j
    sr = fir_reference(xr, a, D).real                     # sum |Re ct| |Re x|
    si = fir_reference(xi, a, D).real                     # sum |Re ct| |Im x|
    tr = fir_reference(xr, b, D).real                     # sum |Im ct| |Re x|
    ti = fir_reference(xi, b, D).real                     # sum |Im ct| |Im x|
    f = (2 * T + np.asarray(parts, dtype=np.float64) + 4) * 2.0 ** -24
    return np.hypot(f * (sr + ti), f * (si + tr))


def closed_form_phases(incr, n):
    """rotator.hpp's rotate_value restated in float64: the float32 increment's true angle times the output index, and the
    magnitude |incr|^(n mod 512) that GNU Radio's phase drifts to between its every-512 renormalisations; rounded to
    float32 like the kernel's (pr, pi)"""
    ir, ii = float(np.float32(incr.real)), float(np.float32(incr.imag))
    ang = math.atan2(ii, ir)
    lm = math.log(math.hypot(ir, ii))
    k = np.arange(n, dtype=np.float64)
    mag = np.exp((np.arange(n) % 512) * lm)
    return ((mag * np.cos(k * ang)).astype(np.float32) + 1j * (mag * np.sin(k * ang)).astype(np.float32)).astype(np.complex64)


def rotator_allowance(incrs, n, phases=None):
    """largest |GNU Radio's iterated float32 phase - closed form| over the given increments and outputs 0 .. n - 1.
    phases(incr, n): the iteration (default: oracle.grspec.rotator_phases, the reference's behaviour)"""
    if phases is None:
        from oracle import grspec as G
        phases = lambda inc, m: G.rotator_phases(inc, m)[0]
    worst = 0.0
    for inc in incrs:
        got = phases(np.complex64(inc), n).astype(np.complex128)
        worst = max(worst, float(np.abs(got - closed_form_phases(np.complex64(inc), n).astype(np.complex128)).max()))
    return worst


ROTATOR_ALLOWANCE_MEASURED = 2.0e-6       # see the module docstring; the CPU test holds it to what it measures
ROTATOR_ALLOWANCE = 2 * ROTATOR_ALLOWANCE_MEASURED + 2.0 ** -22


# ---------------------------------------------------------------------------------------------- the GPU shape table
def cuts_for(n_ks, D):
    """sample counts of consecutive pushes that yield n_ks[i] outputs in push i; the cuts fall off the decimation grid
    by a remainder that changes from push to push"""
    cuts, k_tot, n_prev = [], 0, 0
    for i, nk in enumerate(n_ks):
        k_tot += nk
        n_tot = (k_tot - 1) * D + 1 + (3 * i + 1) % D          # outputs so far = (n_tot - 1) // D + 1 = k_tot
        cuts.append(n_tot - n_prev)
        n_prev = n_tot
    return cuts


# One row = one front-end: (T, D, channels, outputs per push, out_capacity or 0).  Every push of every row is one
# matrix-core launch whose plan is mfma_plan(channels, outputs, T); tests/test_fir_census_cpu.py holds the set of plans
# reached to the set the planner can return at all.
MFMA_ROWS = [
    (64, 5, 160, [4000, 129, 4000], 0),          # even T, 2 chunks, parts = 1
    (64, 1, 512, [3968, 127, 3967], 0),          # D = 1 with NT = 2, parts = 1
    (127, 8, 8, [1, 17, 15, 16], 0),             # fewest channels of a launch, a one-output push first
    (127, 2, 9, [17, 1, 63, 64, 65], 0),
    (128, 3, 160, [3967, 3968, 3969, 128], 0),   # D = 3 with NT = 2, 3 chunks
    (191, 4, 33, [63, 16, 64, 65], 0),
    (192, 1, 65, [3969, 3968, 257], 0),          # D = 1 with NT = 2, split
    (192, 4, 33, [4100, 4150], 0),               # 4 chunks in 3 parts
    (255, 2, 9, [65, 15, 127, 129], 0),
    (256, 3, 65, [4000, 4000, 255], 0),          # 5 chunks
    (320, 2, 512, [3250, 65], 0),                # the one corner where the planner answers (2, 6)
    (349, 8, 37, [129, 17, 128], 0),
    (449, 2, 65, [1400, 3000, 1400, 3000], 1 << 12),   # 8 chunks in 7 parts, both tile widths
    (449, 5, 256, [3000, 3000], 0),
    (511, 3, 32, [64, 1, 63, 129], 0),
    (512, 1, 33, [127, 1000, 900, 127], 1 << 11),      # 9 chunks in 8 parts; the output ring wraps inside a 16-output tile
    (575, 4, 65, [2000, 1999], 0),               # 9 chunks in 5 parts
]

# rows run again with float samples, random float taps and non-zero offsets: (T, D, channels, outputs per push)
COMPLEX_ROWS = [
    (64, 5, 160, [4000, 129]),                   # parts = 1
    (128, 3, 160, [3967, 128]),                  # NT = 2
    (449, 2, 65, [1400, 3000]),                  # uneven split, both tile widths
]
COMPLEX_FS = 1e6
COMPLEX_OFFSETS_HZ = [-450000.0, -268750.0, -193750.0, 106250.0, 212500.0, 306250.0, 493750.0]


def complex_offsets(n_chans):
    """the channels' offsets: the seven of COMPLEX_OFFSETS_HZ in turn (channels that share one still differ in their taps)"""
    return [COMPLEX_OFFSETS_HZ[i % len(COMPLEX_OFFSETS_HZ)] for i in range(n_chans)]


def complex_increments():
    """every rotator increment the complex-tap cases use: (decimation of a row) x (offset)"""
    from oracle import cbind as OC
    return [OC.xlating_composite(np.ones(1, np.float32), D, f, COMPLEX_FS)[1]
            for D in sorted({r[1] for r in COMPLEX_ROWS}) for f in COMPLEX_OFFSETS_HZ]


def plans_of(rows):
    """[(row index, push index, T, channels, outputs, (nt, parts))]"""
    return [(i, j, r[0], r[2], nk, mfma_plan(r[2], nk, r[0])) for i, r in enumerate(rows) for j, nk in enumerate(r[3])]


# ---------------------------------------------------------------------------------------------- vector kernels
# fir_bank_kernel on a shared source: direct channels below the matrix cores' 64 taps.  Outputs per push around KR = 8 and
# across choose_kt's 256-output tile; the first pushes are all zero history at T = 63.
VECTOR_CHANS = [1, 2, 3, 16, 17]
VECTOR_T = [1, 2, 63]
VECTOR_D = [1, 7]
VECTOR_N_KS = [1, 7, 8, 9, 255, 257, 300]

# fir_small_kernel and the own-source fir_bank_kernel through chained channels.  Two parents (offset 0, 8 integer taps in
# [-1, 1], D = 2, samples in [-1, 1]: |parent| <= 8 per component), every child on each: taps in [-1, 1], so
# |child| <= 8 T <= 1600 and the discriminator's products y[k] conj(y[k-1]) stay below 2 * 1600^2 < 2^24.
CHAIN_PARENT = (8, 2)                                     # (T, D)
CHAIN_SMALL_T = [1, 5, 95, 96]                            # fir_small_outputs > 0
CHAIN_VECTOR_T = [97, 200]                                # one channel per workgroup of fir_bank_kernel
CHAIN_D = [1, 3]
CHAIN_PARENT_N_KS = [1, 7, 8, 9, 511, 512, 1100, 3]       # parent outputs per push: a D = 1 child crosses the 511-output tile


def chain_case(rng):
    """-> (x, cuts, parents, children): parents = [(taps, y)], children = [(parent index, T, D, taps, y, fm)] with y the
    exact complex64 outputs and fm = quadrature_demod_cf(y, 1)"""
    from oracle import grspec as G
    Tp, Dp = CHAIN_PARENT
    cuts = cuts_for(CHAIN_PARENT_N_KS, Dp)
    x = int_stream(rng, sum(cuts), 1)
    parents, children = [], []
    for pi in range(2):
        tp = int_taps(rng, 1, Tp, 1)[0]
        yp = fir_reference(x, tp, Dp)[0]
        parents.append((tp, yp.astype(np.complex64)))
        for T in CHAIN_SMALL_T + CHAIN_VECTOR_T:
            for D in CHAIN_D:
                tc = int_taps(rng, 1, T, 1)[0]
                yc = fir_reference(yp, tc, D)[0]
                assert max(np.abs(yc.real).max(), np.abs(yc.imag).max()) <= 2048
                yc = yc.astype(np.complex64)
                children.append((pi, T, D, tc, yc, G.quadrature_demod_cf(yc, 1.0)))
    return x, cuts, parents, children
