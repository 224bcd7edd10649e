// nid_wave.hpp -- what tsbk.hip and p25lc.hip share of a P25 frame (gfx950): a dibit of the slicer's word ring, the NID as
// the lanes 0 .. 31 gather it, and behind the option RCF_NID_BCH the wave form of its BCH(63,16,23) decoder; the arithmetic is
// nid_core.hpp.  A wave is a channel; the received word is wave-uniform (the two ballots of the NID's dibits).
//   syndromes       lane m < 22 runs Horner over the 63 bits for S[m] = r(alpha^(m + 1))
//   Berlekamp-      a fixed 22 rounds in rs_decode's idiom (p25lc.hip): coefficient i of the locator and of the shadow
//   Massey          polynomial in lane i; a round is one lane-reversed read of S, a product, an xor-reduction over the wave
//                   and one shifted read of the shadow polynomial
//   Chien           lane e < 63 is the bit of x^e and evaluates the locator at 1 / alpha^e; the ballot of the zeros IS the
//                   error pattern, which must have as many members as the locator's degree
//   re-check        the syndromes of the corrected word
// No Forney step: the code is binary, an error's value is 1.  Every cross-lane read stands in wave-uniform control flow; all
// trip counts are constants; no LDS, no stores.
#pragma once
#include "item_wave.hpp"
#include "nid_core.hpp"

namespace rcfx {

namespace {

// r: the received word as a polynomial (uniform) -> the code word within kNidT bits of it and *fix, the bits changed, or r as
// it is and *fix = kNidFixBad
__device__ __forceinline__ uint64_t nid_decode_wave(uint64_t r, int lane, int *fix)
{
    const uint32_t S = nid_syndrome(r, lane);
    uint32_t C = lane == 0 ? 1u : 0u, B = C, b = 1;
    int Ln = 0, m = 1;
    for (int rd = 0; rd < kNidRoots; ++rd) {
        const uint32_t Sr = lane_read(S, rd - lane);
        // (the reduction leaves d in every lane; read as a scalar it keeps the branches below and Ln, m, b out of the vector unit)
        const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_xor(lane <= rd ? p25lc_gf_mul(C, Sr) : 0u));
        const uint32_t Bs = lane_read(B, lane - m);
        if (d == 0) { ++m; continue; }               // (uniform)
        const uint32_t Cn = C ^ p25lc_gf_mul(p25lc_gf_mul(d, p25lc_gf_inv(b)), lane >= m ? Bs : 0u);
        if (2 * Ln <= rd) { B = C; Ln = rd + 1 - Ln; b = d; m = 1; } else ++m;
        C = Cn;
    }
    const uint32_t xi = lane < kNidBits ? nid_xinv(lane) : 0u;
    uint32_t v = 0;
    for (int j = kNidT; j >= 0; --j) v = p25lc_gf_mul(v, xi) ^ lane_read(C, j);
    const uint64_t roots = __ballot(lane < kNidBits && v == 0);
    const bool ok = Ln <= kNidT && __popcll(roots) == Ln;
    const uint64_t fixed = r ^ roots;
    const bool left = __ballot(nid_syndrome(fixed, lane) != 0) != 0;
    const bool bad = !ok || left;
    *fix = __builtin_amdgcn_readfirstlane(bad ? kNidFixBad : Ln);     // (the same in every lane: it came through the reductions)
    return bad ? r : fixed;
}

// the four counters of rcf_nid_state_t as a launch collects them
struct NidCount {
    int decoded = 0, fixed = 0, bits = 0, bad = 0;
    __device__ __forceinline__ void add(int fix)
    {
        const int good = fix != kNidFixBad ? 1 : 0;
        decoded += 1;
        bad += 1 - good;
        fixed += good & (fix != 0 ? 1 : 0);
        bits += good * fix;
    }
    template <class State> __device__ __forceinline__ void store(State *st) const
    {
        st->nid_decoded += decoded; st->nid_fixed += fixed; st->nid_bits += bits; st->nid_bad += bad;
    }
};

// stream dibit p of the slicer's word ring (p inside the whole words: the caller's condition)
template <class State> __device__ __forceinline__ int ring_dibit(const FramesLaunch<State> &L, int64_t p)
{
    return tsbk_word_dibit(L.word_ring[(uint64_t)(p >> 4) & L.word_mask], (int)(p & 15));
}

// The NID of the frame at s, info dibits 24 .. 55: its two words as received and word0, what names nac and duid -- nid0, or
// with the option (nid: uniform) the decoded first word, then with fix its nid_fix, counted in nc
struct Nid {
    uint32_t nid0, nid1, word0;
    int fix;
};
template <class State> __device__ __forceinline__ Nid read_nid(const FramesLaunch<State> &L, int64_t s, int lane, bool nid, NidCount &nc)
{
    const int dn = lane < 32 ? ring_dibit(L, s + tsbk_frame_pos(24 + lane)) : 0;
    const uint64_t nhi = __ballot(dn & 2), nlo = __ballot(dn & 1);
    Nid r{slice_word_be(nhi, nlo, 2, 0), slice_word_be(nhi, nlo, 2, 1), 0u, 0};
    r.word0 = r.nid0;
    if (nid) {                                       // (uniform)
        r.word0 = nid_word0_of(nid_decode_wave(nid_poly(r.nid0, r.nid1), lane, &r.fix));
        nc.add(r.fix);
    }
    return r;
}

}  // namespace

}  // namespace rcfx
