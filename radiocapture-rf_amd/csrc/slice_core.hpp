// slice_core.hpp -- the arithmetic of the hard-decision stage (slice.hip; definition: include/rcf.h at rcf_chan_slicer): the
// decision of a soft symbol, the assembly of packed words from the lane masks of a chunk of 64 symbols, and the sync-word
// window with its Hamming distance.  No HIP types in here: RCF_DEVFN is the function qualifier, so that the CPU suite
// compiles this very source with g++ and walks it over the streams the numpy restatement sees (tests/test_slicer_cpu.py).
//
// A chunk is the 64 symbols k = 64 c .. 64 c + 63 of the stage's stream; bit j of a lane mask belongs to symbol 64 c + j
// (what a ballot over the wave gives).  The bit stream is MSB first: the chunk's symbol 0 comes first.  With bps bits per
// symbol a chunk is bps 64-bit UNITS of the stream, the first-received bit of a unit its bit 63, and 2 bps words of 32 / bps
// symbols each.
#pragma once
#include <stdint.h>
#ifndef RCF_DEVFN
#define RCF_DEVFN __device__ __forceinline__
#endif

namespace rcfx {

namespace {

// binary_slicer_fb: 1 for s >= 0 (a NaN: 0)
RCF_DEVFN int slice_binary(float s) { return s >= 0.0f ? 1 : 0; }
// op25 fsk4_slicer_fb (rcf.p25.slice_dibits): dibits 3, 2, 0, 1 below, between and above the three levels (a NaN: 1)
RCF_DEVFN int slice_fsk4(float s, float l0, float l1, float l2) { return s < l0 ? 3 : s < l1 ? 2 : s < l2 ? 0 : 1; }

RCF_DEVFN uint32_t slice_brev32(uint32_t v)
{
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    return (v >> 16) | (v << 16);
}
RCF_DEVFN uint32_t slice_bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
// the 16 bits of v, bit i to bit 2 i
RCF_DEVFN uint32_t slice_spread16(uint32_t v)
{
    v &= 0xffffu;
    v = (v | (v << 8)) & 0x00ff00ffu;
    v = (v | (v << 4)) & 0x0f0f0f0fu;
    v = (v | (v << 2)) & 0x33333333u;
    return (v | (v << 1)) & 0x55555555u;
}

// Word q of a chunk (q < 2 bps) in stream order -- the first-received bit is bit 31 -- from the lane masks of the decisions'
// higher bit (hi; unused at bps 1) and lower bit (lo).  Symbols whose lanes are clear in both contribute zeros.
RCF_DEVFN uint32_t slice_word_be(uint64_t hi, uint64_t lo, int bps, int q)
{
    if (bps == 1) return slice_brev32((uint32_t)(lo >> (32 * q)));
    const uint32_t h = slice_brev32((uint32_t)(hi >> (16 * q)) & 0xffffu) >> 16;      // symbol 16 q first: bit 15
    const uint32_t l = slice_brev32((uint32_t)(lo >> (16 * q)) & 0xffffu) >> 16;
    return (slice_spread16(h) << 1) | slice_spread16(l);
}
// ... and as it is stored: stream byte j is byte j & 3 of the word in memory (little-endian), so that a uint8 view of the
// word ring is unpacked_to_packed_bb(bps, GR_MSB_FIRST)'s byte stream
RCF_DEVFN uint32_t slice_word_mem(uint32_t be) { return slice_bswap32(be); }
// unit u of a chunk (u < bps): 64 bits of the stream, the first-received bit highest
RCF_DEVFN uint64_t slice_unit(uint64_t hi, uint64_t lo, int bps, int u)
{
    return ((uint64_t)slice_word_be(hi, lo, bps, 2 * u) << 32) | slice_word_be(hi, lo, bps, 2 * u + 1);
}

RCF_DEVFN uint64_t slice_shl(uint64_t v, int s) { return s >= 64 ? 0 : v << s; }     // s >= 0
RCF_DEVFN uint64_t slice_shr(uint64_t v, int s) { return s >= 64 ? 0 : v >> s; }
// The last 64 bits of the stream before bit offset o of a chunk (0 <= o < 128: the stage stands o / bps symbols into the
// chunk), seen as part of the 192 bits (the 64 before the chunk : unit 0 : unit 1): which of them fall into part p
// (0 .. 2), at their places; the other bits of the part are 0.  This is how the state's `tail` comes back into a chunk
// that a block enters in the middle.
RCF_DEVFN uint64_t slice_place_tail(uint64_t tail, int o, int p)
{
    const int s = 128 - o;                           // the 192-bit value (tail << s), 0 < s <= 128
    return p == 2 ? slice_shl(tail, s) : p == 1 ? (s < 64 ? slice_shr(tail, 64 - s) : slice_shl(tail, s - 64))
                                                : (s < 64 ? 0 : slice_shr(tail, 128 - s));
}
// The last 64 bits of the stream ending with the symbol of lane j, the oldest bit highest: a funnel shift over
// (before : unit 0) or, from the chunk's 33rd symbol on at bps 2, (unit 0 : unit 1)
RCF_DEVFN uint64_t slice_window(uint64_t before, uint64_t unit0, uint64_t unit1, int bps, int j)
{
    const int e = bps * (j + 1);                     // stream bits of the chunk up to and with symbol j: 1 .. 128
    const uint64_t older = e <= 64 ? before : unit0, newer = e <= 64 ? unit0 : unit1;
    const int sh = (e <= 64 ? 64 : 128) - e;         // 0 .. 63
    return (newer >> sh) | (sh ? older << (64 - sh) : 0);
}
RCF_DEVFN int slice_popcount64(uint64_t v)
{
    v = v - ((v >> 1) & 0x5555555555555555ull);
    v = (v & 0x3333333333333333ull) + ((v >> 2) & 0x3333333333333333ull);
    v = (v + (v >> 4)) & 0x0f0f0f0f0f0f0f0full;
    return (int)((v * 0x0101010101010101ull) >> 56);
}
// Hamming distance of the window's low sync_bits bits (8 .. 64) from the sync word's
RCF_DEVFN int slice_sync_dist(uint64_t window, uint64_t sync_word, int sync_bits)
{
    const uint64_t m = sync_bits >= 64 ? ~0ull : (1ull << sync_bits) - 1;
    return slice_popcount64((window ^ sync_word) & m);
}
// The hit rule: within max_errors of the sync word, or -- sync_both -- of its inverse, whose distance is sync_bits - dist
RCF_DEVFN bool slice_is_hit(int dist, int sync_bits, int max_errors, int sync_both)
{
    return dist <= max_errors || (sync_both && dist >= sync_bits - max_errors);
}
// ... and what makes the two polarities tell apart: the ranges 0 .. max_errors and sync_bits - max_errors .. sync_bits do not meet
RCF_DEVFN bool slice_sync_both_ok(int sync_bits, int max_errors, int sync_both)
{
    return sync_both == 0 || (sync_both == 1 && sync_bits > 0 && 2 * max_errors < sync_bits);
}
// a hit's item in the hit ring
RCF_DEVFN uint32_t slice_hit_item(int dist, int64_t k) { return ((uint32_t)dist << 26) | (uint32_t)((uint64_t)k & 0x3ffffffu); }
// ... and its k again: the largest value <= n_symbols - 1 with the item's low 26 bits (rcf.h at rcf_chan_slicer)
RCF_DEVFN int64_t slice_widen_k(uint32_t item, int64_t n_symbols)
{
    const int64_t low = (int64_t)(item & 0x3ffffffu), last = n_symbols - 1;
    return low + ((last - low) >> 26) * ((int64_t)1 << 26);
}

// ---- The frame walk of the decoders behind a slicer (TSBK, P25 voice, EDACS): item_wave.hpp's frame_walk on the device,
// tests/native/wave_host.hpp's walk on the host.  A stage names its constants in a struct W:
//   kSync      symbols of the sync word: a hit's k is its last symbol, the frame starts at s = k - (kSync - 1)
//   kAccept    a hit is accepted when its k is at least this far behind the last accepted one's
//   kDecide    a frame is decided once the symbols s .. s + kDecide - 1 are in whole words
//   kLongest   symbols of the longest frame
//   kPerWord   symbols per word of the slicer's ring: 16 (dibits) or 32 (bits)
//   kCut       the next accepted hit cuts the frame short (the walk looks ahead for it in the same 64 hits)
// The trips of one launch from the host's n_k (the block's new symbols at most), whatever the device's counters say: the hits
// to look at are this block's (at most one per new symbol) and those of an undecided frame's kDecide symbols and the unfinished
// word; a decided frame costs one trip, with kCut at most two, and 64 rejected hits one
template <class W> RCF_DEVFN int slice_walk_trips(int n_k)
{
    const int bound = n_k + W::kDecide + 32;
    return (W::kCut ? 2 : 1) * (bound / W::kAccept + 1) + bound / 64 + 2;
}

// What a chunk does to the packed stream, for the lanes [a, b) of it that are new (0 <= a < b <= 64; the masks carry those
// lanes only).  `partial` is the unfinished word so far, in stream order with its missing bits 0 -- it belongs to the word
// `a` falls into.  The words [a / spw, b / spw) of the chunk become whole, spw = 32 / bps symbols per word: lane i (0 .. 3)
// has the i-th of them (false: there is none), in stream order ...
RCF_DEVFN bool slice_lane_word(uint64_t hi, uint64_t lo, int bps, int a, int b, uint32_t partial, int lane, uint32_t *be)
{
    const int spw = 32 / bps, qa = a / spw, qb = b / spw, q = qa + lane;
    if (q >= qb) return false;
    *be = slice_word_be(hi, lo, bps, q) | (lane == 0 ? partial : 0u);
    return true;
}
// ... and this is the unfinished word after the chunk (0 when the chunk's new lanes end on a word boundary)
RCF_DEVFN uint32_t slice_partial_after(uint64_t hi, uint64_t lo, int bps, int a, int b, uint32_t partial)
{
    const int spw = 32 / bps, qa = a / spw, qb = b / spw;
    return b % spw ? slice_word_be(hi, lo, bps, qb) | (qb == qa ? partial : 0u) : 0u;
}

}  // namespace

}  // namespace rcfx
