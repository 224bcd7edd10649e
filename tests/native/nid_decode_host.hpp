// nid_decode_host.hpp -- radiocapture-rf_amd/csrc/nid_wave.hpp on the host, for the check programs of the two P25 stages: a
// dibit of the slicer's word ring, the wave form of the NID's BCH(63,16,23) decoder step by step over the 64 lanes, and the
// NID of a frame as the lanes 0 .. 31 gather it.  Include it with RCF_DEVFN and RCF_DEVCONST defined.
#pragma once
#include "../../radiocapture-rf_amd/csrc/nid_core.hpp"
#include "wave_host.hpp"

namespace {

static_assert(State{}.k_last == kTsbkNoFrame, "a fresh stage has accepted no hit");

int ring_dibit(const Rings &R, int64_t p) { return tsbk_word_dibit(R.word(p >> 4), (int)(p & 15)); }

// nid_decode_wave of nid_wave.hpp
uint64_t nid_decode_wave(uint64_t r, int *fix)
{
    Lanes S, C, B;
    for (int l = 0; l < 64; ++l) { S[l] = nid_syndrome(r, l); C[l] = B[l] = l == 0 ? 1u : 0u; }
    uint32_t b = 1;
    int Ln = 0, m = 1;
    for (int rd = 0; rd < kNidRoots; ++rd) {
        Lanes term, Bs;
        for (int l = 0; l < 64; ++l) {
            term[l] = l <= rd ? p25lc_gf_mul(C[l], S[(rd - l) & 63]) : 0u;
            Bs[l] = B[(l - m) & 63];
        }
        const uint32_t d = wave_xor(term);
        if (d == 0) { ++m; continue; }
        Lanes Cn;
        for (int l = 0; l < 64; ++l) Cn[l] = C[l] ^ p25lc_gf_mul(p25lc_gf_mul(d, p25lc_gf_inv(b)), l >= m ? Bs[l] : 0u);
        if (2 * Ln <= rd) { memcpy(B, C, sizeof(B)); Ln = rd + 1 - Ln; b = d; m = 1; } else ++m;
        memcpy(C, Cn, sizeof(C));
    }
    bool root[64], nz[64];
    for (int l = 0; l < 64; ++l) {
        const uint32_t xi = l < kNidBits ? nid_xinv(l) : 0u;
        uint32_t v = 0;
        for (int j = kNidT; j >= 0; --j) v = p25lc_gf_mul(v, xi) ^ C[j];
        root[l] = l < kNidBits && v == 0;
    }
    const uint64_t roots = ballot(root);
    const bool ok = Ln <= kNidT && slice_popcount64(roots) == Ln;
    const uint64_t fixed = r ^ roots;
    for (int l = 0; l < 64; ++l) nz[l] = nid_syndrome(fixed, l) != 0;
    const bool bad = !ok || ballot(nz) != 0;
    *fix = bad ? kNidFixBad : Ln;
    return bad ? r : fixed;
}

struct NidCount { int64_t decoded = 0, fixed = 0, bits = 0, bad = 0; };
void count(NidCount &nc, int fix)
{
    ++nc.decoded;
    if (fix == kNidFixBad) ++nc.bad;
    else if (fix) { ++nc.fixed; nc.bits += fix; }
}

// the NID of the frame at s: its two words as received, and with the option the decoded first word and nid_fix
void read_nid(const Rings &R, int64_t s, bool nid, NidCount &nc, uint32_t *nid0, uint32_t *nid1, uint32_t *nidc, int *fix)
{
    bool hb[64], lb[64];
    for (int l = 0; l < 64; ++l) {
        const int dn = l < 32 ? ring_dibit(R, s + tsbk_frame_pos(24 + l)) : 0;
        hb[l] = dn & 2; lb[l] = dn & 1;
    }
    const uint64_t nhi = ballot(hb), nlo = ballot(lb);
    *nid0 = *nidc = slice_word_be(nhi, nlo, 2, 0);
    *nid1 = slice_word_be(nhi, nlo, 2, 1);
    *fix = -1;
    if (nid) {
        *nidc = nid_word0_of(nid_decode_wave(nid_poly(*nid0, *nid1), fix));
        count(nc, *fix);
    }
}

}  // namespace
