"""References for the exact census of the polyphase filterbanks (radiocapture-rf_amd/csrc/pfb.hip, pfb5.hip, pfbm.hip).
CPU only; the integer machinery is tests/fir_census_ref.py's.  Two facts, both read from the code:

1. Bin 0 of every bank is a plain integer FIR, bit for bit.
     out_0[n] = sum_rho u_rho[n],   u_rho[n] = sum_p h[NB p + rho] x[n D - rho - NB p]              (pfb.hip, "Math")
   The taps reach the device unchanged (rcf_pfb_open copies them into the zero-padded polyphase table); the twiddle table
   starts with (float)cos(0), (float)sin(0) = (1, 0), twiddle_powers starts from (1, 0), cmul by (1, 0) is exact in either
   spelling, output 0 of dft2/3/4/5 and of the PFA and Stockham compositions of fft_core.hpp is a sum of its inputs only,
   and the OS > 1 phase factor e^{-j 2 pi k n D / NB} is 1 at k = 0.  With integer-valued float32 taps and samples whose
   absolute sum T h_max x_max stays below 2^24 every partial sum is an exact integer in ANY order, so bin 0 must equal
   fir_census_ref.fir_reference(x, h, D) exactly -- for every family, shape, launch form and cut.  This sees every tap and
   every input position: halo rows, chunk and launch boundaries, ring wrap, zero history, the riders.

2. With one unit impulse per prototype span every output of every bin is one tap times one unit phasor.
   Taps h[i] = 1 + i, unit impulses at s_j = j S with S = NB Ppad + 1: S >= T and S = 1 mod D, so no frame sees two
   impulses and D impulses visit every tap exactly once.  Frame n of bin k is
       h[i] e^{-j 2 pi k s_j / NB},  i = n D - s_j,   when 0 <= i < T,   and exactly 0 otherwise:
   the FFT has a single non-zero input and each output carries only the rounding of its twiddle chain.  This names which
   tap and which branch-to-bin twiddle every output read -- the whole NB x NB matrix, which bin 0 cannot see.

  PFB_ROWS        one row per kernel instantiation pfb_shape.h names (tests/test_pfb_census_cpu.py holds the coverage)
  bank_census     a row's integer stream, prototype, cuts and the exact bin 0
  coded_bank      fact 2's stream with the expected tap and value of every (frame, bin); decode_bank reads a result back
  rider_case      the 256-bin bank with a stage-2 channel on bin 0: both exact, every intermediate checked below 2^24
  fm_case         a fused-discriminator bank whose bin-0 products y[n] conj(y[n-1]) are integers below 2^24
  MUTATIONS       the faults a relative-rms bar cannot see (tests/test_pfb_census_cpu.py: the gap)

No form needed an exception: every launch form the GPU test reaches is held to the exact bin-0 comparison."""
import collections

import numpy as np

from fir_census_ref import cuts_for, fir_reference, int_stream, int_taps, n_outputs

X_MAX = H_MAX = 7
TARGET_FRAMES = 200
RING = 64                # frames of the bins ring the GPU test opens a row's bank with: it wraps three times
LEAD_FRAMES = 2          # frames of the absolute grid that lie before the sample the bank is opened at


# ---------------------------------------------------------------------------------------------- pfb_shape.h restated
PFB1_NB = [64, 128, 256, 512, 1024]
PFB1_CHUNK = 16
PFB1_PPAD = {1: [4, 14, 16], 2: [4, 16]}                  # pfb1_round_p: 14 at OS = 1 only
# (R, R3, OS, P, grouped, fused): NB = R R R3
PFB5_SHAPES = [(20, 4, 2, 2, 1, 1), (20, 4, 2, 1, 0, 0), (20, 4, 1, 4, 0, 0), (20, 4, 4, 1, 0, 0),
               (20, 8, 4, 1, 1, 1), (20, 8, 2, 2, 1, 0), (20, 8, 2, 1, 0, 0), (20, 8, 1, 4, 0, 0),
               (20, 2, 2, 2, 1, 1), (20, 2, 2, 1, 0, 0), (20, 2, 1, 4, 0, 0), (20, 2, 4, 1, 0, 0),
               (20, 1, 2, 2, 1, 1), (20, 1, 2, 1, 0, 0), (20, 1, 1, 4, 0, 0), (20, 1, 4, 1, 0, 0)]
PFBM_SHAPES = [(10, 16), (12, 16), (20, 24), (20, 32), (24, 40), (32, 40)]
PFBM_P = 2


def pfbm_frames(NB):
    return 16 if NB <= 192 else (8 if NB <= 640 else 4)


def zero_history(NB, D, Ppad, n_lo, start_sample, halo_frames=0):
    """pfb_shape.h pfb_zero_history: the launch whose first frame is n_lo still reaches before the bank's start"""
    return (n_lo - halo_frames - (NB // D) * (Ppad - 1)) * D - (NB - 1) < start_sample


# ---------------------------------------------------------------------------------------------- the rows
Row = collections.namedtuple("Row", "family NB OS D P Ppad chunk T lead n_frames cuts zh_frames")


def push_frames(F, zh_frames, total=TARGET_FRAMES):
    """frames per push against the chunk F and the zero-history boundary (the first zh_frames frames of the bank are
    produced by launches that start before it): no frame at all, one frame, F - 1, F and F + 1 frames on BOTH sides of the
    boundary where they fit before it, the last launch that still reaches before the start (one frame) directly followed by
    the first that does not, several chunks and a remainder, two chunks, and what is left of `total` in pieces"""
    out, cum = [0], 0
    for c in (1, F - 1, F, F + 1):
        if cum + c <= zh_frames - 1:
            out.append(c)
            cum += c
    if cum < zh_frames - 1:
        out.append(zh_frames - 1 - cum)
    out.append(1)                                            # frame zh_frames - 1: the last masking launch
    out += [1, F - 1, F, F + 1, 0, 3 * F + 5, 2 * F]         # from frame zh_frames on: steady state
    while sum(out) < total:                                  # the rest, in pushes that fit the GPU test's ring of RING frames
        out.append(min(total - sum(out), RING - 3))
    return out


def bank_cuts(n_frames, D):
    """-> (lead, cuts): `lead` samples go in before the bank is opened (no multiple of D: the bank's first frame is the
    next one of the absolute grid), then push i of cuts[i] samples yields n_frames[i] frames.  The cuts are
    fir_census_ref.cuts_for's -- off the decimation grid by a remainder that changes from push to push; a push of no frame
    takes the samples that are left before the next frame of the grid from the push behind it (fewer than D)"""
    assert n_frames[-1] > 0
    nz = cuts_for([LEAD_FRAMES] + [c for c in n_frames if c > 0], D)
    lead, nz = nz[0], nz[1:]
    assert lead % D != 0
    cuts, total, j = [], lead, 0
    steal = 0
    for c in n_frames:
        if c == 0:
            z = min(D - 1 - (total - 1) % D, nz[j] - steal - 1)
            assert 1 <= z < D, "no room for a push without a frame"
            cuts.append(z)
            steal += z
            total += z
        else:
            cuts.append(nz[j] - steal)
            total += nz[j] - steal
            steal = 0
            j += 1
    k0 = -(-lead // D)
    at = lead
    for c, n in zip(n_frames, cuts):                         # what the planner will count (plan_pfb)
        assert n > 0 and max(n_outputs(at + n, D), k0) - max(n_outputs(at, D), k0) == c
        at += n
    return lead, cuts


def _row(family, NB, OS, P, Ppad, chunk):
    D = NB // OS
    T = NB * P - NB // 3                                     # no multiple of NB: the last row's zero-padded tail is read
    assert T % NB and -(-T // NB) == P
    lead0 = cuts_for([LEAD_FRAMES], D)[0]
    k0 = -(-lead0 // D)
    zh = next(m for m in range(4096) if not zero_history(NB, D, Ppad, k0 + m, lead0))
    assert zh >= 1
    n_frames = push_frames(chunk, zh)
    lead, cuts = bank_cuts(n_frames, D)
    assert lead == lead0
    return Row(family, NB, OS, D, P, Ppad, chunk, T, lead, n_frames, cuts, zh)


def _rows():
    rows = []
    for NB in PFB1_NB:
        for OS in (1, 2):
            for Ppad in PFB1_PPAD[OS]:
                rows.append(_row(1, NB, OS, Ppad, Ppad, PFB1_CHUNK))
    for R, R3, OS, P, _, _ in PFB5_SHAPES:
        rows.append(_row(2, R * R * R3, OS, P, P, 16 // R3))
    for R1, R2 in PFBM_SHAPES:
        for P in (2, 1):                                     # a two-row prototype, and a one-row one beside a row of zeros
            rows.append(_row(3, R1 * R2, 2, P, PFBM_P, pfbm_frames(R1 * R2)))
    return rows


PFB_ROWS = _rows()


def row_id(r):
    return "f%d_%dbins_os%d_p%d%s" % (r.family, r.NB, r.OS, r.Ppad, "" if r.P == r.Ppad else "_proto%d" % r.P)


def row_bound(r):
    """the largest absolute partial sum of a row's census (x 2: a coded or complex row may add both components)"""
    return r.T * X_MAX * H_MAX * 2


def launches_zero_history(r):
    """per push: does its launch run the masking instantiation (None: no launch)"""
    k0 = -(-r.lead // r.D)
    out, m = [], 0
    for c in r.n_frames:
        out.append(zero_history(r.NB, r.D, r.Ppad, k0 + m, r.lead) if c else None)
        m += c
    return out


def bank_census(r, rng, x_max=X_MAX, h_max=H_MAX):
    """-> (x complex64[lead + sum(cuts)], h float32[T], y complex64[frames]): y the exact bin 0 of the bank opened after
    `lead` samples -- frame m of the bank is frame ceil(lead / D) + m of the absolute grid, zero history before `lead`"""
    assert r.T * 2 * x_max * h_max < 2 ** 24, "partial sums must stay exact in float32"
    x = int_stream(rng, r.lead + sum(r.cuts), x_max)
    h = int_taps(rng, 1, r.T, h_max)[0]
    y = fir_reference(x, h, r.D, start=r.lead)[0]
    assert len(y) == sum(r.n_frames)
    assert np.abs(y.real).max() < 2 ** 24 and np.abs(y.imag).max() < 2 ** 24
    return x, h, y.astype(np.complex64)


def simple_census(rng, NB, D, T, n_frames, x_max=X_MAX, h_max=H_MAX, lead=0):
    """a census without a row: pushes of n_frames[i] frames each (all > 0) -> (x, h, cuts, y)"""
    assert T * 2 * x_max * h_max < 2 ** 24
    if lead:
        cuts = cuts_for([lead] + list(n_frames), D)
        lead, cuts = cuts[0], cuts[1:]
    else:
        cuts = cuts_for(n_frames, D)
    x = int_stream(rng, lead + sum(cuts), x_max)
    h = int_taps(rng, 1, T, h_max)[0]
    y = fir_reference(x, h, D, start=lead)[0]
    assert len(y) == sum(n_frames)
    return x, h, lead, cuts, y.astype(np.complex64)


# ---------------------------------------------------------------------------------------------- coded impulses
def coded_span(NB, Ppad):
    return NB * Ppad + 1


def coded_bank(NB, D, Ppad, T=None, bins=None, taps=None):
    """-> (x complex64, h float32[T], tap int64[frames], want complex128[frames, len(bins)]).  x: unit impulses (1 + 0j)
    at s_j = j S, j < D; h[i] = 1 + i (or `taps`, to evaluate a mutated prototype); tap[n]: the one tap index frame n
    reads, -1 where it reads none (the value is then exactly 0) -- the same for every bin; want[n, b] the exact value at
    bin bins[b] (default: all bins): h[tap] e^{-j 2 pi k s_j / NB}, the phase from (k s_j) mod NB in integers"""
    assert NB % D == 0
    S = coded_span(NB, Ppad)
    if T is None:                                            # every branch carries a tap: T >= NB
        T = NB * Ppad - (NB // 3 if Ppad > 1 else 0)
    assert 1 <= T <= NB * Ppad < S and S % D == 1 % D
    h = (1.0 + np.arange(T)).astype(np.float32) if taps is None else np.asarray(taps, np.float32)
    assert len(h) == T
    n = (D - 1) * S + T + D
    x = np.zeros(n, np.complex64)
    x[np.arange(D) * S] = 1.0
    frames = np.arange(n_outputs(n, D), dtype=np.int64)
    j = np.minimum(frames * D // S, D - 1)                   # the latest impulse at or before sample n D
    i = frames * D - j * S
    tap = np.where(i < T, i, -1)
    ks = np.arange(NB, dtype=np.int64) if bins is None else np.asarray(bins, dtype=np.int64)
    ph = (ks[None, :] * ((j * S) % NB)[:, None]) % NB
    amp = np.where(tap >= 0, h.astype(np.float64)[np.maximum(tap, 0)], 0.0)
    want = amp[:, None] * np.exp(-2j * np.pi * ph / NB)
    return x, h, tap, want


def decode_bank(y):
    """outputs of a coded run -> (tap index read: round(|y|) - 1, so -1 where the magnitude rounds to 0; phase)"""
    y = np.asarray(y).astype(np.complex128)
    return np.rint(np.abs(y)).astype(np.int64) - 1, np.angle(y)


def spread_bins(NB, count=64):
    """`count` bins of a bank too large to read whole: 1, NB/2 - 1, NB/2, NB/2 + 1, NB - 1; one bin in every aligned run of
    64 bins that holds none of these yet, at an offset that changes from run to run; and, up to `count`, bins at changing
    offsets in `count` equal segments of the bin range.  The kernels hand bins to threads as t + W pass with W a multiple
    of 64 (pfb5.hip: W = 320, the wave is (bin mod 320) / 64) or as bin mod NB/16 (pfb.hip's epilogue, four such residues
    per wave), so this puts a bin on every (wave, pass) position of the first and on every wave of the second:
    tests/test_pfb_census_cpu.py holds both"""
    if NB <= count:
        return list(range(NB))
    out = {1, NB // 2 - 1, NB // 2, NB // 2 + 1, NB - 1}
    for run in range(-(-NB // 64)):
        if not any(k // 64 == run for k in out):
            out.add(min(NB - 1, 64 * run + (13 * run + 5) % 64))
    assert len(out) <= count
    for g in range(count):
        lo, hi = -(-g * NB // count), -(-(g + 1) * NB // count)
        if len(out) < count:
            out.add(lo + (37 * g + 11) % (hi - lo))
    assert len(out) == count
    return sorted(out)


# the coded test's shapes: the smallest-P row of each bin count -> (NB, OS, Ppad, all bins?)
CODED_SHAPES = [(64, 1, 4, True), (64, 2, 4, True), (128, 1, 4, True), (128, 2, 4, True), (256, 1, 4, True), (256, 2, 4, True),
                (160, 2, 2, True), (192, 2, 2, True), (400, 2, 1, True),
                (512, 1, 4, False), (512, 2, 4, False), (1024, 1, 4, False), (1024, 2, 4, False),
                (480, 2, 2, False), (640, 2, 2, False), (960, 2, 2, False), (1280, 2, 2, False),
                (800, 2, 1, False), (1600, 2, 1, False), (1600, 4, 1, False), (3200, 4, 1, False)]


# ---------------------------------------------------------------------------------------------- special launch forms
def rider_case(rng):
    """the 256-bin bank (OS 1, 14 rows: the kernel that carries the stage-2 rider) with a channel of 11 integer taps,
    decimation 3, on bin 0.  x, h in {-1, 0, 1}, |t| <= 7 -> dict(x, h, cuts, n_frames, y0, t2, D2, y2); every
    intermediate -- the bank's partial sums and the channel's -- is checked below 2^24 here"""
    NB, D, T, D2, T2 = 256, 256, 256 * 14 - 85, 3, 11
    n_frames = [40, 100, 100, 100, 100, 100]                 # the first launch masks; each later one carries the one before
    x, h, lead, cuts, y0 = simple_census(rng, NB, D, T, n_frames, 1, 1)
    assert not zero_history(NB, D, 14, n_frames[0], 0)
    t2 = int_taps(rng, 1, T2, 7)[0]
    worst0 = fir_reference(np.abs(x.real) + 1j * np.abs(x.imag), np.abs(h), D)[0]
    assert max(worst0.real.max(), worst0.imag.max()) < 2 ** 24
    worst2 = fir_reference(np.abs(y0.real) + 1j * np.abs(y0.imag), np.abs(t2), D2)[0]
    assert max(worst2.real.max(), worst2.imag.max()) < 2 ** 24
    y2 = fir_reference(y0, t2, D2)[0].astype(np.complex64)
    return dict(NB=NB, D=D, x=x, h=h, cuts=cuts, n_frames=n_frames, y0=y0, t2=t2, D2=D2, y2=y2)


def fm_case(rng):
    """400 bins at OS 2, two rows: the fused discriminator's shape.  x, h in {-1, 0, 1} -> dict(..., y0, fm, exact): fm =
    quadrature_demod_cf(y0, 1); exact[n]: both products of each component of y0[n] conj(y0[n - 1]) and their sum are
    integers below 2^24, so neither the order nor fusing can show.  With these magnitudes that holds for ALL outputs
    (share left out: 0, asserted)"""
    from oracle import grspec as G
    NB, D, P = 400, 200, 2
    T = NB * P - NB // 3
    n_frames = [21, 16, 15, 17, 53, 80]
    x, h, lead, cuts, y0 = simple_census(rng, NB, D, T, n_frames, 1, 1)
    a = y0.astype(np.complex128)
    b = np.concatenate([[0], a[:-1]])
    mag = np.maximum(np.abs(a.real * b.real) + np.abs(a.imag * b.imag), np.abs(a.imag * b.real) + np.abs(a.real * b.imag))
    exact = mag < 2 ** 24
    assert exact.all()
    return dict(NB=NB, D=D, x=x, h=h, cuts=cuts, n_frames=n_frames, y0=y0, fm=G.quadrature_demod_cf(y0, 1.0), exact=exact)


# ---------------------------------------------------------------------------------------------- the gap
# What a relative rms over a bin of noise cannot see.  kind "drop": the first n taps of the prototype are zeroed; "swap":
# its last two change places; "row": frames at chunk position `pos` of every 16-frame chunk lose polyphase row `row` (-1:
# the oldest, the last row of the table; 0: the newest).  bar: the bar of the existing bank tests on that shape.  proto:
# "lp2" = low_pass_2(1, fs, 0.4 bw, 0.2 bw, 60 dB, Blackman-Harris), "chan" = the reference's channel
# filter at 20 Msps / 12.5 kHz.  The stimulus is the existing tests': unit noise, 150 frames.
#
# For white noise the error's expectation is known without a draw (expected_rel_rms): the edited taps' share of the
# prototype's energy.  Six of the ten sit 3x to 10^5x under their bar.  The other four -- the lost NEWEST row (b) at every
# bin count and the 199 dropped taps -- sit AT it (at_bar): expectation 0.94 to 1.01 x the bar, so one draw of 150 frames
# (nine or ten affected frames) lands under it and the next one over it; of the twelve draws default_rng(0 .. 11) the (b)
# rows are under the bar on 3 (256 bins), 4 (64) and 7 (1024), the 199 taps on 8.  A test that passes a fault on every other stream does not
# hold it, which is the point; but the inequality "under the bar" is then a property of the draw, and `seed` is the
# smallest seed on which it holds (for the six others: 0, as it does on every draw tried).
Mutation = collections.namedtuple("Mutation", "name NB D proto kind arg bar seed at_bar")
MUTATIONS = [
    Mutation("256 bins: first 8 taps dropped", 256, 256, "lp2", "drop", 8, 2e-5, 0, False),
    Mutation("256 bins: first 199 taps dropped", 256, 256, "lp2", "drop", 199, 2e-5, 0, True),
    Mutation("256 bins: last two taps swapped", 256, 256, "lp2", "swap", None, 2e-5, 0, False),
    Mutation("256 bins: (a) first frame of a chunk loses its oldest row", 256, 256, "lp2", "row", (0, -1), 2e-5, 0, False),
    Mutation("256 bins: (b) last frame of a chunk loses its newest row", 256, 256, "lp2", "row", (15, 0), 2e-5, 1, True),
    Mutation("64 bins: (a)", 64, 64, "lp2", "row", (0, -1), 2e-5, 0, False),
    Mutation("64 bins: (b)", 64, 64, "lp2", "row", (15, 0), 2e-5, 4, True),
    Mutation("1024 bins: (a)", 1024, 1024, "lp2", "row", (0, -1), 2e-5, 0, False),
    Mutation("1024 bins: (b)", 1024, 1024, "lp2", "row", (15, 0), 2e-5, 1, True),
    Mutation("1600 bins, channel filter: last two taps swapped", 1600, 800, "chan", "swap", None, 1e-5, 0, False),
]
GAP_FRAMES = 150


def expected_rel_rms(m, proto):
    """the relative rms of mutation m's error in bin 0 for unit WHITE noise over GAP_FRAMES frames, in expectation:
    sqrt(share of the frames it touches x energy of the taps it edits / energy of the prototype)"""
    h = np.asarray(proto, np.float64)
    if m.kind == "drop":
        share, lost = 1.0, np.sum(h[:m.arg] ** 2)
    elif m.kind == "swap":
        share, lost = 1.0, 2.0 * (h[-1] - h[-2]) ** 2
    else:
        pos, row = m.arg
        P_ = -(-len(h) // m.NB)
        p = row % P_
        n = np.arange(GAP_FRAMES)
        share = np.count_nonzero((n % 16 == pos) & (n * m.D >= p * m.NB)) / GAP_FRAMES
        lost = np.sum(h[p * m.NB:(p + 1) * m.NB] ** 2)
    return float(np.sqrt(share * lost / np.sum(h ** 2)))


def mutate_taps(h, kind, arg):
    h = np.array(h, copy=True)
    if kind == "drop":
        h[:arg] = 0
    elif kind == "swap":
        h[-1], h[-2] = h[-2], h[-1]
    else:
        raise ValueError(kind)
    return h


def row_taps(h, NB, row):
    """h with polyphase row `row` zeroed (row < 0 counts from the last row the prototype reaches)"""
    P = -(-len(h) // NB)
    p = row % P
    out = np.array(h, copy=True)
    out[p * NB:(p + 1) * NB] = 0
    return out


def mutated_bin0(x, h, D, NB, kind, arg, chunk=16):
    """bin 0 (the plain FIR, float64) of the mutated bank -> (y, affected frames)"""
    y = fir_reference(x, h, D)[0]
    if kind != "row":
        return fir_reference(x, mutate_taps(h, kind, arg), D)[0], np.arange(len(y))
    pos, row = arg
    bad = fir_reference(x, row_taps(h, NB, row), D)[0]
    n = np.arange(len(y))
    hit = (n % chunk == pos) & (n * D >= (row % -(-len(h) // NB)) * NB)      # (a row that still reads before the stream's start loses nothing)
    return np.where(hit, bad, y), np.flatnonzero(hit)
