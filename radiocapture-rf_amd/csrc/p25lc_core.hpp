// p25lc_core.hpp -- the arithmetic of the P25 voice-channel stage (p25lc.hip; definition: include/rcf.h at rcf_chan_p25lc):
// which data unit a frame is and where its inner code words sit, the Hamming (10,6,3) and Golay (23,12,7) decoders of one
// word, GF(64) with the pieces of the Reed-Solomon decoder that one lane computes, and the packing of a record.  Frames,
// hits and the status-symbol map are tsbk_core.hpp's, used as they stand.  No HIP types in here, like tsbk_core.hpp:
// RCF_DEVFN is the function qualifier and RCF_DEVCONST the qualifier of the tables, so that the CPU suite compiles this very
// source with g++ (tests/native/p25lc_core_check.cpp; tests/native/p25es_core_check.cpp for the options at the file's end).
//
// Golay: a 2048-entry table from the 11-bit syndrome to the error pattern of weight <= 3, built at compile time.  The code is
// perfect, so the table IS the complete decoder -- one syndrome (twelve shift / xor rounds) and one load per word -- where an
// algorithmic decoder (error trapping with toggled bits) walks 23 rotations per word and, as the reference's shows, is easy
// to leave incomplete.  8 KiB of constant memory, read by at most 36 lanes per frame.
#pragma once
#include "tsbk_core.hpp"

namespace rcfx {

namespace {

constexpr int kP25lcFrameDibits = 864;   // the longest voice data unit: an LDU
// a frame is decided once the stream's whole words hold the 864 dibits and the 24 of a sync word that may begin inside them
constexpr int kP25lcDecideDibits = kP25lcFrameDibits + kTsbkSyncDibits;
// the frame walk's constants: the trunking stage's with the longer frame
struct P25lcWalk : TsbkWalk {
    static constexpr int kDecide = kP25lcDecideDibits, kLongest = kP25lcFrameDibits;
};
constexpr int kP25lcRecWords = 8;        // uint32 words of a record
constexpr int kP25lcHdu = 0, kP25lcLdu1 = 1, kP25lcTlc = 2, kP25lcFrame = 3;   // a record's kind
constexpr int kP25lcMaxSyms = 36, kP25lcMaxT = 8;                               // RS(36,20,17): the longest word, the most errors
constexpr uint32_t kP25lcFlagCorrect = 1u;                                      // P25lcLaunch::flags

// ---- the data units.  kind of a frame with this duid and fd dibits: decoded only if its last needed dibit lies inside
RCF_DEVFN int p25lc_kind(int duid, int fd)
{
    return duid == 0x0 && fd > 389 ? kP25lcHdu : duid == 0x5 && fd > 788 ? kP25lcLdu1 : duid == 0xF && fd > 204 ? kP25lcTlc : kP25lcFrame;
}
RCF_DEVFN int p25lc_inner_words(int kind) { return kind == kP25lcHdu ? 36 : kind == kP25lcLdu1 ? 24 : 12; }
RCF_DEVFN int p25lc_word_bits(int kind) { return kind == kP25lcHdu ? 18 : kind == kP25lcLdu1 ? 10 : 24; }
RCF_DEVFN int p25lc_rs_n(int kind) { return kind == kP25lcHdu ? 36 : 24; }
RCF_DEVFN int p25lc_rs_k(int kind) { return kind == kP25lcHdu ? 20 : 12; }
RCF_DEVFN int p25lc_rs_t(int kind) { return kind == kP25lcHdu ? 8 : 6; }
// the first info bit of inner word w (always even: a word is whole dibits); LDU1: four words behind every second voice frame
RCF_DEVFN int p25lc_word_bit0(int kind, int w)
{
    return kind == kP25lcHdu ? 112 + 18 * w : kind == kP25lcLdu1 ? 112 + 288 + 184 * (w >> 2) + 10 * (w & 3) : 112 + 24 * w;
}
constexpr int kP25lcLsdDibit = 752;      // the LDU1's 32 low-speed data bits: info bits 1504 .. 1535
// inner word w of a frame, its first bit highest; dibit(r): the frame's dibit r
template <class Dibit> RCF_DEVFN uint32_t p25lc_gather(Dibit &&dibit, int kind, int w)
{
    const int j0 = p25lc_word_bit0(kind, w) >> 1, nd = p25lc_word_bits(kind) >> 1;
    uint32_t v = 0;
    for (int d = 0; d < 12; ++d)
        if (d < nd) v = (v << 2) | (uint32_t)dibit(tsbk_frame_pos(j0 + d));
    return v;
}

// ---- the inner codes.  status: 0 good, 1 fixed, 2 bad (data as read)
RCF_DEVFN uint32_t p25lc_parity(uint32_t v) { return (uint32_t)slice_popcount64(v) & 1u; }
// Hamming (10,6,3): the four check rows; the syndrome of an error in bit i (from the first) is nibble i of the constant
RCF_DEVFN uint32_t p25lc_hamming(uint32_t w, int *status)
{
    const uint32_t syn = p25lc_parity(w & 0x398u) << 3 | p25lc_parity(w & 0x354u) << 2 | p25lc_parity(w & 0x2E2u) << 1 | p25lc_parity(w & 0x1E1u);
    *status = syn ? 2 : 0;
    for (int i = 0; i < 10; ++i)
        if (syn == (uint32_t)((0xEDB73C8421ull >> (4 * (9 - i))) & 15u)) { w ^= 1u << (9 - i); *status = 1; }
    return (w >> 4) & 63u;
}
// Golay (23,12,7), generator 0xC75, systematic: the 12 data bits first.  The syndrome: the word modulo the generator
constexpr uint32_t kP25lcGolayPoly = 0xC75u;
constexpr uint32_t p25lc_golay_syndrome(uint32_t cw23)
{
    for (int i = 22; i >= 11; --i)
        if (cw23 & (1u << i)) cw23 ^= kP25lcGolayPoly << (i - 11);
    return cw23;
}
struct P25lcGolayTable { uint32_t e[2048]; };
constexpr P25lcGolayTable p25lc_make_golay_table()
{
    P25lcGolayTable r{};
    uint32_t one[23] = {};
    for (int a = 0; a < 23; ++a) one[a] = p25lc_golay_syndrome(1u << a);
    for (int a = 0; a < 23; ++a) {
        r.e[one[a]] = 1u << a;
        for (int b = a + 1; b < 23; ++b) {
            r.e[one[a] ^ one[b]] = 1u << a | 1u << b;
            for (int c = b + 1; c < 23; ++c) r.e[one[a] ^ one[b] ^ one[c]] = 1u << a | 1u << b | 1u << c;
        }
    }
    return r;
}
RCF_DEVCONST P25lcGolayTable kP25lcGolay = p25lc_make_golay_table();
// the code word nearest to the 23 bits
RCF_DEVFN uint32_t p25lc_golay23(uint32_t cw23) { return cw23 ^ kP25lcGolay.e[p25lc_golay_syndrome(cw23) & 2047u]; }
// extended (24,12,8): the 24th bit takes no part -> the 12 data bits
RCF_DEVFN uint32_t p25lc_golay24(uint32_t w, int *status)
{
    const uint32_t r = (w >> 1) & 0x7fffffu, c = p25lc_golay23(r);
    *status = c != r ? 1 : 0;
    return c >> 11;
}
// shortened (18,6,8): six leading zero data bits; a nearest code word that sets one of them is none of this code's
RCF_DEVFN uint32_t p25lc_golay18(uint32_t w, int *status)
{
    const uint32_t r = (w >> 1) & 0x1ffffu, c = p25lc_golay23(r);
    if (c >> 17) { *status = 2; return (w >> 12) & 63u; }
    *status = c != r ? 1 : 0;
    return (c >> 11) & 63u;
}
// a word's data as p25_general reads it: its first 6 or 12 bits
RCF_DEVFN uint32_t p25lc_systematic(int kind, uint32_t w) { return kind == kP25lcHdu ? (w >> 12) & 63u : kind == kP25lcLdu1 ? (w >> 4) & 63u : (w >> 12) & 0xfffu; }
RCF_DEVFN uint32_t p25lc_inner(int kind, uint32_t w, int *status)
{
    return kind == kP25lcHdu ? p25lc_golay18(w, status) : kind == kP25lcLdu1 ? p25lc_hamming(w, status) : p25lc_golay24(w, status);
}

// ---- GF(64): x^6 + x + 1, alpha = 2.  Products by shift and xor; powers of alpha and inverses through the two tables
struct P25lcGf { uint8_t exp[64], log[64]; };
constexpr P25lcGf p25lc_make_gf()
{
    P25lcGf r{};
    uint32_t v = 1;
    for (int e = 0; e < 63; ++e) {
        r.exp[e] = (uint8_t)v;
        r.log[v] = (uint8_t)e;
        v <<= 1;
        if (v & 0x40u) v ^= 0x43u;
    }
    r.exp[63] = 1;
    return r;
}
RCF_DEVCONST P25lcGf kP25lcGf = p25lc_make_gf();
RCF_DEVFN uint32_t p25lc_gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 6; ++i) p ^= (0u - ((b >> i) & 1u)) & (a << i);
    for (int i = 10; i >= 6; --i) p ^= (0u - ((p >> i) & 1u)) & (0x43u << (i - 6));
    return p;
}
RCF_DEVFN uint32_t p25lc_gf_alpha(int e) { return kP25lcGf.exp[e % 63]; }                            // e >= 0
RCF_DEVFN uint32_t p25lc_gf_inv(uint32_t a) { return kP25lcGf.exp[(63 - kP25lcGf.log[a & 63u]) % 63]; }   // a != 0
// RS(n, k, d): symbol i (0 .. n - 1, data first) is the coefficient of x^(n - 1 - i); the roots are alpha^1 .. alpha^(2 t).
// 1 / X of symbol i's locator X = alpha^(n - 1 - i): where the Chien search and Forney evaluate
RCF_DEVFN uint32_t p25lc_rs_xinv(int n, int i) { return p25lc_gf_alpha(63 - ((n - 1 - i) % 63)); }

// ---- a record.  nid0: the NID's first word in stream order (tsbk_core.hpp), whose top 16 bits are nac and duid
RCF_DEVFN uint32_t p25lc_word0(int kind, bool rs_bad, int n_rs, uint32_t dist, uint32_t nid0)
{
    return (uint32_t)(kind & 3) | (rs_bad ? 4u : 0u) | ((uint32_t)(n_rs & 15) << 4) | ((dist & 63u) << 10) | (nid0 & 0xffff0000u);
}
RCF_DEVFN uint32_t p25lc_word7(int fd, int n_fixed, int n_bad) { return (uint32_t)fd | ((uint32_t)(n_fixed & 63) << 16) | ((uint32_t)(n_bad & 63) << 22); }
// payload word q (0 .. 3) of k six-bit symbols, the first bit highest: it starts `off` bits into symbol `first` and is cut
// from the seven symbols first .. first + 6 (acc: those, symbols >= k as 0)
RCF_DEVFN int p25lc_pay_first(int q) { return (32 * q) / 6; }
RCF_DEVFN uint32_t p25lc_pay_word(uint64_t acc, int q) { return (uint32_t)(acc >> (10 - (32 * q - 6 * p25lc_pay_first(q)))); }

// ---- the options of rcf_chan_p25lc_opt (include/rcf.h): LDU2's encryption sync, and inner words given up as erasures.
// Everything above stands as it is; what an option changes is a function of its own down here.
constexpr uint32_t kP25lcFlagEs = 2u, kP25lcFlagErasures = 4u;                  // P25lcLaunch::flags: the call's options << 1
constexpr int kP25lcLdu2 = 4;                                                   // a record's kind: bit 2 of it is word 0 bit 3
constexpr int kP25lcMaxD1 = 2 * kP25lcMaxT;                                     // d - 1 of RS(36,20,17): the most erasures, the joint locator's highest degree
RCF_DEVFN int p25lc_kind(int duid, int fd, uint32_t flags) { return (flags & kP25lcFlagEs) && duid == 0xA && fd > 788 ? kP25lcLdu2 : p25lc_kind(duid, fd); }
// an LDU2's 24 Hamming words sit where the LDU1's do: the kind to gather and to decode inner words by
RCF_DEVFN int p25lc_words_kind(int kind) { return kind == kP25lcLdu2 ? kP25lcLdu1 : kind; }
RCF_DEVFN int p25lc_rs_k_es(int kind) { return kind == kP25lcLdu2 ? 16 : p25lc_rs_k(kind); }      // RS(24,16,9)
RCF_DEVFN int p25lc_rs_t_es(int kind) { return kind == kP25lcLdu2 ? 4 : p25lc_rs_t(kind); }
RCF_DEVFN bool p25lc_has_lsd(int kind) { return kind == kP25lcLdu1 || kind == kP25lcLdu2; }
// extended (24,12,8) with the 24th bit taking part: three bits changed and the received overall parity is not the corrected
// word's -> four errors detected: BAD, data as read.  Otherwise p25lc_golay24's answer
RCF_DEVFN uint32_t p25lc_golay24_detect(uint32_t w, int *status)
{
    const uint32_t r = (w >> 1) & 0x7fffffu, c = p25lc_golay23(r);
    if (slice_popcount64(c ^ r) == 3 && p25lc_parity(c) != (w & 1u)) { *status = 2; return (w >> 12) & 0xfffu; }
    *status = c != r ? 1 : 0;
    return c >> 11;
}
RCF_DEVFN uint32_t p25lc_inner(int kind, uint32_t w, int *status, bool erasures)
{
    return erasures && kind == kP25lcTlc ? p25lc_golay24_detect(w, status) : p25lc_inner(p25lc_words_kind(kind), w, status);
}
// X of symbol i, the factor (1 + X x) it contributes to the erasure locator
RCF_DEVFN uint32_t p25lc_rs_x(int n, int i) { return p25lc_gf_alpha(n - 1 - i); }
// word 0 with the kind's third bit in bit 3 and n_rs's fifth in bit 8: p25lc_word0's value for kind < 4 and n_rs < 16
RCF_DEVFN uint32_t p25lc_word0_wide(int kind, bool rs_bad, int n_rs, uint32_t dist, uint32_t nid0)
{
    return p25lc_word0(kind, rs_bad, n_rs, dist, nid0) | ((uint32_t)(kind & 4) << 1) | ((uint32_t)(n_rs & 16) << 4);
}

}  // namespace

}  // namespace rcfx
