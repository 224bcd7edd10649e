// tsbk_core.hpp -- the arithmetic of the P25 trunking stage (tsbk.hip; definition: include/rcf.h at rcf_chan_tsbk): the
// frame walk's constants, where an info dibit sits in a frame, the deinterleaver's index map, the rate-1/2
// trellis as transition maps with their composition (what the wave scans), for the option RCF_TRELLIS_VITERBI the code
// words as min-plus matrices with theirs, the CRC's per-bit terms and the packing of a record.  No HIP types in here, like
// slice_core.hpp, whose mask-to-word helpers it uses: RCF_DEVFN is the function qualifier and RCF_DEVCONST the qualifier of
// the one table, so that the CPU suite compiles this very source with g++ (tests/native/tsbk_core_check.cpp,
// trellis_core_check.cpp).
#pragma once
#include "slice_core.hpp"
#ifndef RCF_DEVCONST
#define RCF_DEVCONST __constant__ const
#endif

namespace rcfx {

namespace {

constexpr int kTsbkSyncDibits = 24;      // the 48-bit frame sync
constexpr int kTsbkFrameDibits = 360;    // the longest TSDU: three blocks
// a frame is decided once the stream's whole words hold its 360 dibits and the 24 of a sync word that may follow them: every
// hit that can shorten the frame is in the hit ring by then, however the input was cut
constexpr int kTsbkDecideDibits = kTsbkFrameDibits + kTsbkSyncDibits;
constexpr int kTsbkCodeWords = 49;       // code words of a block: 98 dibits
constexpr int kTsbkRecWords = 8;         // uint32 words of a record
constexpr int64_t kTsbkNoFrame = -((int64_t)1 << 60);   // k_last before the first accepted hit

// the frame walk's constants (slice_core.hpp at slice_walk_trips).  kAccept is buf.find(sync, fsoffset + 6): a sync word that
// begins inside the last accepted one is no frame
struct TsbkWalk {
    static constexpr int kSync = kTsbkSyncDibits, kAccept = kTsbkSyncDibits, kDecide = kTsbkDecideDibits, kLongest = kTsbkFrameDibits, kPerWord = 16;
    static constexpr bool kCut = true;
};
// the stage's own names for the widening and the accept rule, for sources that walk the hits themselves
RCF_DEVFN int64_t tsbk_widen_k(uint32_t item, int64_t n_symbols) { return slice_widen_k(item, n_symbols); }
RCF_DEVFN bool tsbk_accept(int64_t k, int64_t k_last) { return k >= k_last + TsbkWalk::kAccept; }
// frame dibit of info dibit j: every 36th dibit is a status symbol (procStatus)
RCF_DEVFN int tsbk_frame_pos(int j) { return j + j / 35; }
// block b's info dibits are 56 + 98 b .. 153 + 98 b; the blocks whose last dibit lies inside a frame of fd dibits
RCF_DEVFN int tsbk_block_dibit(int b, int p) { return 56 + 98 * b + p; }
RCF_DEVFN int tsbk_blocks_in(int fd)
{
    int n = 0;
    for (int b = 0; b < 3; ++b) n += tsbk_frame_pos(tsbk_block_dibit(b, 97)) < fd ? 1 : 0;
    return n;
}
// data_deinterleave: the first of the two block dibits (0 .. 96) of code word t (0 .. 48)
RCF_DEVFN int tsbk_deinterleave(int t)
{
    const int m = t & 3;
    return t >= 48 ? 24 : 2 * (t >> 2) + (m ? 2 + 24 * m : 0);
}
// dibit p (0 .. 15) of a word of the slicer's ring as it lies in memory
RCF_DEVFN int tsbk_word_dibit(uint32_t mem, int p) { return (int)(slice_bswap32(mem) >> (30 - 2 * p)) & 3; }

// ---- trellis_1_2_decode.  Row `state` of the standard's table, candidate d in the nibble 4 d
RCF_DEVFN uint32_t tsbk_trellis_row(int state) { return state == 0 ? 0xF1C2u : state == 1 ? 0x3D0Eu : state == 2 ? 0x4A79u : 0x86B5u; }
RCF_DEVFN int tsbk_pop4(uint32_t v) { return (int)(0x4332322132212110ull >> (4 * (v & 15u))) & 7; }
// the state after code word c (4 bits) in `state`: the candidate with the most bits equal, the lowest of equals -- over all
// 64 pairs what the reference's count(4) / count(3) / best-guess ladder gives; *exact: a candidate equals c
RCF_DEVFN int tsbk_next_state(int state, uint32_t c, bool *exact)
{
    const uint32_t row = tsbk_trellis_row(state);
    int best = 0, best_dist = 5;
    for (int d = 0; d < 4; ++d) {
        const int dist = tsbk_pop4(((row >> (4 * d)) & 15u) ^ c);
        if (dist < best_dist) { best_dist = dist; best = d; }
    }
    *exact = best_dist == 0;
    return best;
}
// a code word as a transition map: the state after it from state s in the bits 2 s, 2 s + 1
RCF_DEVFN uint32_t tsbk_map(uint32_t c)
{
    uint32_t m = 0;
    bool e;
    for (int s = 0; s < 4; ++s) m |= (uint32_t)tsbk_next_state(s, c, &e) << (2 * s);
    return m;
}
constexpr uint32_t kTsbkIdentity = 0xE4u;
// first, then `then`: the map of two code words in a row (associative: what the inclusive scan combines)
RCF_DEVFN uint32_t tsbk_compose(uint32_t first, uint32_t then)
{
    uint32_t m = 0;
    for (int s = 0; s < 4; ++s) m |= ((then >> (2 * ((first >> (2 * s)) & 3u))) & 3u) << (2 * s);
    return m;
}

// ---- the option RCF_TRELLIS_VITERBI (rcf.h at rcf_chan_tsbk_opt): the path of least cost that ends in state 0, the
// lexicographically smallest of equals.  All of it is min-plus algebra over 4 x 4 matrices of small integers: a code word
// is the matrix M[s][d] = popcount(W[s][d] xor c), a run of code words their product, and column 0 of the product of the
// words t .. 48 is beta_t, the least cost from each state before word t to the end.  The wave scans the products.
constexpr uint32_t kTsbkFlagViterbi = 0x200u;    // TsbkLaunch::flags, next to kNidFlagBch
constexpr uint32_t kTsbkNoPath = 255u;           // an entry no path reaches; a path's cost is at most 4 x 49 = 196
// row s in row[s], entry d in its byte d
struct TsbkMat { uint32_t row[4]; };
RCF_DEVFN uint32_t tsbk_mat_at(const TsbkMat &m, int s, int d) { return (m.row[s] >> (8 * d)) & 255u; }
// the matrix of code word c; flush: the 49th word, whose dibit is 0, so only d = 0 is a path
RCF_DEVFN TsbkMat tsbk_mat(uint32_t c, bool flush)
{
    TsbkMat m;
    for (int s = 0; s < 4; ++s) {
        const uint32_t row = tsbk_trellis_row(s);
        uint32_t v = 0;
        for (int d = 0; d < 4; ++d) v |= (flush && d ? kTsbkNoPath : (uint32_t)tsbk_pop4(((row >> (4 * d)) & 15u) ^ c)) << (8 * d);
        m.row[s] = v;
    }
    return m;
}
RCF_DEVFN TsbkMat tsbk_mat_identity()
{
    TsbkMat m;
    for (int s = 0; s < 4; ++s) m.row[s] = 0xffffffffu ^ (255u << (8 * s));
    return m;
}
// first, then `then`: (A x B)[s][d] = min over m of A[s][m] + B[m][d], kTsbkNoPath absorbing (associative: the sums of real
// paths stay below it)
RCF_DEVFN TsbkMat tsbk_mat_compose(const TsbkMat &first, const TsbkMat &then)
{
    TsbkMat r;
    for (int s = 0; s < 4; ++s) {
        uint32_t v = 0;
        for (int d = 0; d < 4; ++d) {
            uint32_t best = kTsbkNoPath;
            for (int m = 0; m < 4; ++m) {
                const uint32_t sum = tsbk_mat_at(first, s, m) + tsbk_mat_at(then, m, d);
                if (sum < best) best = sum;
            }
            v |= best << (8 * d);
        }
        r.row[s] = v;
    }
    return r;
}
// column 0 of a suffix product: beta[s] in byte s
RCF_DEVFN uint32_t tsbk_mat_beta(const TsbkMat &suffix)
{
    return (suffix.row[0] & 255u) | (suffix.row[1] & 255u) << 8 | (suffix.row[2] & 255u) << 16 | (suffix.row[3] & 255u) << 24;
}
// the forward step as a transition map (tsbk_map's encoding): from state s the lowest d with the least M[s][d] + beta_next[d]
RCF_DEVFN uint32_t tsbk_viterbi_map(const TsbkMat &m, uint32_t beta_next)
{
    uint32_t map = 0;
    for (int s = 0; s < 4; ++s) {
        uint32_t best = 0, least = 2 * kTsbkNoPath + 1;
        for (int d = 0; d < 4; ++d) {
            const uint32_t sum = tsbk_mat_at(m, s, d) + ((beta_next >> (8 * d)) & 255u);
            if (sum < least) { least = sum; best = (uint32_t)d; }
        }
        map |= best << (2 * s);
    }
    return map;
}
// bits in which code word c differs from the path's word W[prev][state]
RCF_DEVFN int tsbk_branch_dist(int prev, int state, uint32_t c) { return tsbk_pop4(((tsbk_trellis_row(prev) >> (4 * state)) & 15u) ^ c); }
// what the option adds to a record's word 7 (without it these bits are 0): the path's cost, and that the block went this way
RCF_DEVFN uint32_t tsbk_viterbi_word7(int cost) { return ((uint32_t)(cost & 255) << 21) | (1u << 29); }

// ---- crc16 of the reference: register 0, every bit shifted in, xor 0x1021 when bit 16 falls out; good: 0xffff.  From 0 the
// register is linear in the bits: bit p (0 .. 95, the first one 0) adds x^(95 - p) mod the polynomial -- these terms
struct TsbkCrcTerms { uint16_t t[96]; };
constexpr TsbkCrcTerms tsbk_make_crc_terms()
{
    TsbkCrcTerms r{};
    uint32_t v = 1;
    for (int e = 0; e < 96; ++e) {
        r.t[95 - e] = (uint16_t)v;
        v <<= 1;
        if (v & 0x10000u) v = (v & 0xffffu) ^ 0x1021u;
    }
    return r;
}
RCF_DEVCONST TsbkCrcTerms kTsbkCrcTerms = tsbk_make_crc_terms();
// what decoded dibit t (0 .. 47) of a block adds to the register
RCF_DEVFN uint32_t tsbk_crc_term(int t, int dibit)
{
    return ((dibit & 2) ? (uint32_t)kTsbkCrcTerms.t[2 * t] : 0u) ^ ((dibit & 1) ? (uint32_t)kTsbkCrcTerms.t[2 * t + 1] : 0u);
}

// ---- a record's word 0; nid0: the NID's first word in stream order, whose top 16 bits are nac and duid as the record holds them
RCF_DEVFN uint32_t tsbk_word0(int b, bool crc_bad, int next_bit, int n_inexact, uint32_t dist, uint32_t nid0)
{
    return (uint32_t)(b & 3) | (crc_bad ? 4u : 0u) | ((uint32_t)(next_bit & 1) << 3) | ((uint32_t)(n_inexact & 63) << 4) |
           ((dist & 63u) << 10) | (nid0 & 0xffff0000u);
}
RCF_DEVFN int tsbk_duid(uint32_t nid0) { return (int)(nid0 >> 16) & 15; }

}  // namespace

}  // namespace rcfx
