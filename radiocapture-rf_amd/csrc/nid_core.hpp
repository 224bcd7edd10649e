// nid_core.hpp -- the arithmetic of the P25 NID's BCH(63,16,23) decoder (the option RCF_NID_BCH of the TSBK and the voice
// stage; definition: include/rcf.h at rcf_chan_tsbk_ex): what one lane of the wave form (nid_wave.hpp) computes, and how
// the result enters a record.  The code is the binary subfield subcode of RS(63,41,23) over GF(64) with the roots alpha^1 ..
// alpha^22, so the field is p25lc_core.hpp's, used as it stands.  No HIP types in here, like the other *_core.hpp: the CPU
// suite compiles this very source with g++ (tests/native/nid_core_check.cpp).
//
// The word: code bit i (0 .. 62) is info bit 48 + i of the frame -- nac in the bits 0 .. 11, duid in 12 .. 15 -- and the
// coefficient of x^(62 - i).  The 64th bit of the NID takes no part.  `r` below is the word as a polynomial: bit e of it is
// the coefficient of x^e, so r = (nid0 : nid1) >> 1 for the NID's two words in stream order.
#pragma once
#include "p25lc_core.hpp"

namespace rcfx {

namespace {

constexpr int kNidBits = 63, kNidT = 11, kNidRoots = 2 * kNidT;
constexpr int kNidFixBad = 15;                   // nid_fix of a word with no code word within kNidT bits
constexpr uint32_t kNidFlagBch = 0x100u;         // TsbkLaunch::flags, P25lcLaunch::flags: the stage decodes the NID
constexpr uint64_t kNidGenerator = 06331141367235453ull;     // degree 47: the lcm of the minimal polynomials of alpha^1 .. alpha^22

RCF_DEVFN uint64_t nid_poly(uint32_t nid0, uint32_t nid1) { return (((uint64_t)nid0 << 32) | nid1) >> 1; }
// the NID's first word with the code word's bits in it: code bit i < 32 is bit e = 62 - i of the polynomial
RCF_DEVFN uint32_t nid_word0_of(uint64_t poly) { return (uint32_t)(poly >> 31); }
// lane m < 22: S[m] = r(alpha^(m + 1)), Horner from x^62 down; the other lanes 0
RCF_DEVFN uint32_t nid_syndrome(uint64_t r, int lane)
{
    const uint32_t am = p25lc_gf_alpha(lane + 1);
    uint32_t S = 0;
    for (int e = kNidBits - 1; e >= 0; --e) S = p25lc_gf_mul(S, am) ^ (uint32_t)((r >> e) & 1u);
    return lane < kNidRoots ? S : 0u;
}
// 1 / X of the bit whose locator is X = alpha^e: where lane e < 63 evaluates the error locator
RCF_DEVFN uint32_t nid_xinv(int e) { return p25lc_gf_alpha((63 - e) % 63); }
// the systematic code word of 16 data bits (nac << 4 | duid), as a polynomial: the data in x^62 .. x^47, the remainder below
RCF_DEVFN uint64_t nid_encode(uint32_t data16)
{
    uint64_t v = (uint64_t)(data16 & 0xffffu) << 47;
    for (int e = kNidBits - 1; e >= 47; --e)
        if (v >> e & 1u) v ^= kNidGenerator << (e - 47);
    return ((uint64_t)(data16 & 0xffffu) << 47) | v;
}

// ---- what the option adds to a record (without it all of these bits are 0)
RCF_DEVFN uint32_t nid_tsbk_word7(int fix) { return ((uint32_t)(fix & 15) << 16) | (1u << 20); }
RCF_DEVFN uint32_t nid_p25lc_word7(int fix) { return (uint32_t)(fix & 15) << 28; }
constexpr uint32_t kNidP25lcWord0 = 1u << 9;

}  // namespace

}  // namespace rcfx
