// edacs_core.hpp -- the arithmetic of the EDACS control-frame stage (edacs.hip; definition: include/rcf.h at rcf_chan_edacs):
// the frame walk's constants, a hit's polarity, where a copy's bit sits in a frame, GF(64) as its two
// tables, a coefficient's syndrome term, the classification of a syndrome pair, one trial of the Chien search, what the
// found positions do to a copy, the election and the packing of a record.  No HIP types in here, like slice_core.hpp:
// RCF_DEVFN is the function qualifier and RCF_DEVCONST the qualifier of the one table, so that the CPU suite compiles this
// very source with g++ (tests/native/edacs_core_check.cpp).
#pragma once
#include "slice_core.hpp"
#ifndef RCF_DEVCONST
#define RCF_DEVCONST __constant__ const
#endif

namespace rcfx {

namespace {

constexpr int kEdacsSyncBits = 48;       // the frame sync
constexpr int kEdacsFrameBits = 288;     // sync word and six copies of 40 bits
constexpr int kEdacsCopyBits = 40;
constexpr int kEdacsCopies = 6;
constexpr int kEdacsCodeBits = 48;       // BCH(48,36): eight colour bits (0 here) in front of a copy's 40
constexpr int kEdacsRecWords = 8;        // uint32 words of a record
constexpr int64_t kEdacsNoFrame = -((int64_t)1 << 60);   // k_last before the first accepted hit

// the frame walk's constants (slice_core.hpp at slice_walk_trips).  kAccept is buf = buf[find + 288:]: the next frame's sync word
// ends a whole frame behind the last accepted one, or later -- so every frame has its 288 bits and no hit cuts one short
struct EdacsWalk {
    static constexpr int kSync = kEdacsSyncBits, kAccept = kEdacsFrameBits, kDecide = kEdacsFrameBits, kLongest = kEdacsFrameBits, kPerWord = 32;
    static constexpr bool kCut = false;
};
// the stage's own names for the widening and the accept rule, for sources that walk the hits themselves
RCF_DEVFN int64_t edacs_widen_k(uint32_t item, int64_t n_symbols) { return slice_widen_k(item, n_symbols); }
RCF_DEVFN bool edacs_accept(int64_t k, int64_t k_last) { return k >= k_last + EdacsWalk::kAccept; }
// a hit of a slicer that searches both polarities matched the inverted word when its distance is past the half
RCF_DEVFN bool edacs_inverted(uint32_t dist, bool sync_both) { return sync_both && dist > (uint32_t)(kEdacsSyncBits / 2); }
RCF_DEVFN uint32_t edacs_hit_dist(uint32_t dist, bool inverted) { return inverted ? (uint32_t)kEdacsSyncBits - dist : dist; }
// Coefficient j (0 .. 39) of copy c's received polynomial is copy bit 39 - j, frame bit 48 + 40 c + 39 - j (the frame's
// bit 0 is the sync word's first)
RCF_DEVFN int edacs_coef_bit(int c, int j) { return kEdacsSyncBits + kEdacsCopyBits * c + (kEdacsCopyBits - 1 - j); }
// packet_framer inverts the middle copy of each three
RCF_DEVFN bool edacs_copy_inverted(int c) { return c == 1 || c == 4; }
// bit p of the stream out of the word of the slicer's ring that holds it, as that word lies in memory
RCF_DEVFN int edacs_word_bit(uint32_t mem, int p) { return (int)(slice_bswap32(mem) >> (31 - (p & 31))) & 1; }

// ---- GF(64), alpha^6 = alpha + 1: alpha^e for e = 0 .. 62 (a[63] = 0, as in the reference's table) and the logarithm
// (l[0] unused: 63)
struct EdacsGf { uint8_t a[64], l[64]; };
constexpr EdacsGf edacs_make_gf()
{
    EdacsGf g{};
    uint32_t v = 1;
    for (int e = 0; e < 63; ++e) {
        g.a[e] = (uint8_t)v;
        g.l[v] = (uint8_t)e;
        v <<= 1;
        if (v & 64u) v = (v & 63u) ^ 3u;
    }
    g.a[63] = 0;
    g.l[0] = 63;
    return g;
}
RCF_DEVCONST EdacsGf kEdacsGf = edacs_make_gf();
RCF_DEVFN uint32_t edacs_alpha(int e) { return kEdacsGf.a[e & 63]; }                 // e = 0 .. 62
RCF_DEVFN int edacs_log(uint32_t v) { return kEdacsGf.l[v & 63u]; }                  // v = 1 .. 63
RCF_DEVFN int edacs_mod63(int v) { return v >= 63 ? v - 63 : v; }                    // v = 0 .. 125

// what a set coefficient j (0 .. 62) adds to the syndromes: alpha^j to S1 (bits 0-5), alpha^(3 j) to S3 (bits 6-11)
RCF_DEVFN uint32_t edacs_syn_term(int j) { return edacs_alpha(j) | (edacs_alpha((3 * j) % 63) << 6); }

// ---- a syndrome pair (S1 bits 0-5, S3 bits 6-11): 0 the copy stands (S1 = 0, whatever S3 is: the reference's
// fall-through), 1 one error at *p, 2 the Chien search decides, over x^2 + alpha^e1 x + alpha^e2 as the reference's
// register walk reads it
RCF_DEVFN int edacs_classify(uint32_t syn, int *p, int *e1, int *e2)
{
    const uint32_t s1 = syn & 63u, s3 = (syn >> 6) & 63u;
    *p = 0; *e1 = 0; *e2 = 0;
    if (s1 == 0) return 0;
    const int l1 = edacs_log(s1);
    const uint32_t cube = edacs_alpha((3 * l1) % 63);
    if (s3 == cube) { *p = l1; return 1; }
    const int la = edacs_log(cube ^ s3);
    *e1 = edacs_mod63(edacs_mod63(2 * l1) - la + 63);
    *e2 = edacs_mod63(l1 - la + 63);
    return 2;
}
// trial i (1 .. 63) of the search: is position i % 63 a root
RCF_DEVFN bool edacs_chien_trial(int e1, int e2, int i)
{
    return (1u ^ edacs_alpha((e1 + i) % 63) ^ edacs_alpha((e2 + 2 * i) % 63)) == 0u;
}
// Copy status from its class and the mask of the positions found (bit p: position p; class 1: the one bit): 0 clean or
// stands, 1 one position, 2 two positions, 3 failed -- a search that does not end with exactly two positions, or any
// position past 47.  *flip: the positions 0 .. 39 as bits of the copy's value (coefficient j = bit j); 40 .. 47 are the
// zero colour bits and change nothing
RCF_DEVFN int edacs_copy_status(int cls, uint64_t pos, uint64_t *flip)
{
    *flip = 0;
    if (cls == 0) return 0;
    if (cls == 2 && slice_popcount64(pos) != 2) return 3;
    if (pos >> kEdacsCodeBits) return 3;
    *flip = pos & (((uint64_t)1 << kEdacsCopyBits) - 1);
    return cls;
}

// ---- message_election over three copies' statuses and corrected values (40 bits, the first bit highest): none decoded --
// no message; exactly one -- that one; else the first value two decoded copies share
RCF_DEVFN bool edacs_elect(int st0, int st1, int st2, uint64_t v0, uint64_t v1, uint64_t v2, uint64_t *m)
{
    const bool d0 = st0 != 3, d1 = st1 != 3, d2 = st2 != 3;
    const int n = (d0 ? 1 : 0) + (d1 ? 1 : 0) + (d2 ? 1 : 0);
    *m = 0;
    if (n == 0) return false;
    if (n == 1) { *m = d0 ? v0 : d1 ? v1 : v2; return true; }
    if (d0 && ((d1 && v0 == v1) || (d2 && v0 == v2))) { *m = v0; return true; }
    if (d1 && d2 && v1 == v2) { *m = v1; return true; }
    return false;
}
// extended addressing: the first four bits of an elected message are or-ed with 0xA
RCF_DEVFN uint64_t edacs_esk(uint64_t m, bool esk) { return esk ? m | ((uint64_t)0xA << 36) : m; }

// ---- a record's words.  statuses: two bits per copy, copy c in the bits 2 c
RCF_DEVFN uint32_t edacs_word0(bool inverted, bool has1, bool has2, uint32_t hit_dist, uint32_t statuses)
{
    return (inverted ? 1u : 0u) | (has1 ? 2u : 0u) | (has2 ? 4u : 0u) | ((hit_dist & 63u) << 4) | ((statuses & 0xfffu) << 10);
}
// word q (0, 1) of a message's two: its five octets in memory order, the rest 0
RCF_DEVFN uint32_t edacs_msg_word(uint64_t m, int q) { return q == 0 ? slice_word_mem((uint32_t)(m >> 8)) : (uint32_t)(m & 0xffu); }

}  // namespace

}  // namespace rcfx
