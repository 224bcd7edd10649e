// osw_core.hpp -- the arithmetic of the SmartNet OSW stage (osw.hip; definition: include/rcf.h at rcf_chan_osw): where a
// hit starts, the framing decision of one step with its lock counter, where a deinterleaved bit sits in a packet, the
// correction mask of a parity syndrome, the fields and the packing of a record.  No HIP types in here, like slice_core.hpp:
// RCF_DEVFN is the function qualifier, so that the CPU suite compiles this very source with g++
// (tests/native/osw_core_check.cpp).
#pragma once
#include "slice_core.hpp"

namespace rcfx {

namespace {

constexpr int kOswSyncBits = 8;          // the frame sync, 10101100
constexpr int kOswPacketBits = 76;       // 38 data and 38 parity bits, interleaved
constexpr int kOswFrameBits = 84;        // sync word and packet
constexpr int kOswDataBits = 38;
constexpr int kOswDecideB = 92;          // a candidate at h0 is decided once the bits up to h0 + 91 are in whole words: every
                                         // hit that starts in h0 + 8 .. h0 + 84 is there by then
constexpr int kOswRecWords = 8;          // uint32 words of a record
constexpr int kOswLockFull = 5;          // locked stops counting up here; is_locked from here on
constexpr uint32_t kOswRelUnknown = 65535u;

// The trips of one launch from the host's n_k (the block's new symbols at most).  What a launch leaves undecided is less than
// 92 + 32 bits behind the cursor or behind h0, so B = n_k + 124 bounds the bits in play and the hits to look at: a decided step
// moves pos by at least 8 bits (B / 8 + 1 steps), a trip without one moves next_hit by at least 56 (B / 56 + 1), one trip
// ends the launch undecided and one skips a frame that the word ring has lost
RCF_DEVFN int osw_trips(int n_k)
{
    const int b = n_k + kOswDecideB + 32;
    return b / kOswSyncBits + 1 + b / 56 + 1 + 2;
}

// where a hit item's sync word starts: k - 7
RCF_DEVFN int64_t osw_hit_start(uint32_t item, int64_t n_symbols)
{
    return slice_widen_k(item, n_symbols) - (kOswSyncBits - 1);
}

// ---- one step of the framing (receive_engine 252-281, 521-525).  What is known: have0 / h0, the first hit with h >= pos;
// have1 / h1, the first hit with h >= h0 + 8 (asked for only in case B once W >= h0 + 92); W, the bits in whole words.
enum : int { kOswWait = 0, kOswReject = 1, kOswAccept = 2 };
// case A: the frame is at pos whatever the hits say
RCF_DEVFN bool osw_case_a(int32_t locked, bool have0, int64_t h0, int64_t pos) { return locked >= 4 || (locked == 3 && have0 && h0 == pos); }
// is the step at pos ready to be decided
RCF_DEVFN bool osw_ready(int32_t locked, bool have0, int64_t h0, int64_t pos, int64_t W)
{
    if (osw_case_a(locked, have0, h0, pos)) return W >= pos + kOswFrameBits;
    return have0 && W >= h0 + kOswDecideB;
}
// ... and its decision, ready given: kOswReject (pos = h0 + 8) or kOswAccept with *rel_nz (the sync word is not at the cursor)
// and *rel (bits 16-31 of word 0)
RCF_DEVFN int osw_decide(int32_t locked, bool have0, int64_t h0, bool have1, int64_t h1, int64_t pos, bool *rel_nz, uint32_t *rel)
{
    if (osw_case_a(locked, have0, h0, pos)) {
        *rel_nz = !(have0 && h0 == pos);
        *rel = *rel_nz ? kOswRelUnknown : 0u;
        return kOswAccept;
    }
    if (locked <= 2 && !(have1 && h1 - h0 == kOswFrameBits)) { *rel_nz = false; *rel = 0u; return kOswReject; }
    const int64_t d = h0 - pos;
    *rel_nz = d != 0;
    *rel = d > (int64_t)kOswRelUnknown ? kOswRelUnknown : (uint32_t)d;
    return kOswAccept;
}
// an accepted frame: the counter's move (263-265), is_locked (267-270) and where the packet's sync word is (275-281)
RCF_DEVFN int32_t osw_lock_step(int32_t locked, bool rel_nz)
{
    if (rel_nz) return locked > INT32_MIN ? locked - 1 : locked;
    return locked < kOswLockFull ? locked + 1 : locked;
}
RCF_DEVFN bool osw_is_locked(int32_t locked) { return locked >= kOswLockFull; }
RCF_DEVFN int64_t osw_sync_pos(int32_t locked_now, int64_t pos, int64_t h0) { return locked_now > 2 ? pos : h0; }
// a clean packet behind a jump gives the step back (319-320)
RCF_DEVFN int32_t osw_lock_clean(int32_t locked, bool rel_nz, uint64_t psyn) { return psyn == 0 && rel_nz ? locked + 1 : locked; }

// ---- the packet.  deinterleave (198-203): out[o] = b[(o >> 2) + 19 (o & 3)]; data[i] = out[2 i], parity[i] = out[2 i + 1]
RCF_DEVFN int osw_in_bit(int o) { return (o >> 2) + 19 * (o & 3); }
RCF_DEVFN int osw_data_bit(int i) { return osw_in_bit(2 * i); }          // i = 0 .. 37: the packet's bit
RCF_DEVFN int osw_parity_bit(int i) { return osw_in_bit(2 * i + 1); }
// bit p of the stream out of the word of the slicer's ring that holds it, as that word lies in memory
RCF_DEVFN int osw_word_bit(uint32_t mem, int p) { return (int)(slice_bswap32(mem) >> (31 - (p & 31))) & 1; }
// Masks: bit i belongs to data[i] / psyn[i] (what a ballot over the lanes 0 .. 37 gives).
// psyn from the masks of data and parity: parity[i] ^ data[i] ^ data[i - 1]
RCF_DEVFN uint64_t osw_psyn(uint64_t data, uint64_t parity) { return (parity ^ data ^ (data << 1)) & (((uint64_t)1 << kOswDataBits) - 1); }
// the correction (313-318): data[x] flips where psyn[x] and psyn[x + 1] are both set, x = 0 .. 36 -- psyn is not modified
// on the way, so the sequential loop is this one mask
RCF_DEVFN uint64_t osw_flip_mask(uint64_t psyn) { return psyn & (psyn >> 1); }
// data[a .. a + n - 1] as a number, the first bit highest
RCF_DEVFN uint32_t osw_field(uint64_t data, int a, int n) { return slice_brev32((uint32_t)(data >> a)) >> (32 - n); }   // n = 1 .. 32
RCF_DEVFN uint32_t osw_lid(uint64_t data) { return osw_field(data, 0, 16) ^ 0xcc38u; }
RCF_DEVFN uint32_t osw_individual(uint64_t data) { return (uint32_t)(data >> 16) & 1u; }
RCF_DEVFN uint32_t osw_cmd(uint64_t data) { return osw_field(data, 17, 10) ^ 0xd5u; }

// ---- a record's words
RCF_DEVFN uint32_t osw_word0(bool rel_nz, uint64_t psyn, bool is_locked, uint64_t data, uint64_t flips, uint32_t rel)
{
    return (rel_nz ? 0u : 1u) | (psyn ? 2u : 0u) | (is_locked ? 4u : 0u) | (osw_individual(data) << 3) |
           ((uint32_t)slice_popcount64(flips) << 4) | ((uint32_t)slice_popcount64(psyn) << 10) | (rel << 16);
}
// word q (0, 1) of a 38-bit mask's two: its bits in stream order, bit 0 first, as the word ring stores a word
RCF_DEVFN uint32_t osw_mask_word(uint64_t mask, int q) { return slice_word_mem(slice_word_be(0, mask, 1, q)); }
// word j of the record
RCF_DEVFN uint32_t osw_rec_word(int j, uint32_t word0, int64_t sync_pos, uint64_t data, uint64_t psyn, int32_t locked)
{
    return j == 0 ? word0 : j == 1 ? (uint32_t)(uint64_t)sync_pos : j == 2 ? (osw_lid(data) | (osw_cmd(data) << 16)) :
           j < 5 ? osw_mask_word(data, j - 3) : j < 7 ? osw_mask_word(psyn, j - 5) : (uint32_t)locked;
}

}  // namespace

}  // namespace rcfx
