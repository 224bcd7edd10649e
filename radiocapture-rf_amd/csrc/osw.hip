// osw.hip -- SmartNet outbound signalling words behind a channel's slicer (gfx950): what the reference's consumer does per
// 84-bit frame in Python strings (moto_control_demod.py: receive_engine's framing with its lock counter, deinterleave, the
// parity syndrome with its correction, the two xor masks), every such stage of a block (or of a group's block) in one launch
// behind slice_kernel's, so that the hits and words of this block are there.  include/rcf.h at rcf_chan_osw DEFINES the
// stage, tests/osw_ref.py restates it; the arithmetic is osw_core.hpp, which the CPU suite compiles for the host as it stands.
//
// The slicer's layout: a WAVE is a channel, four channels per workgroup.  The framing is a loop over steps whose decisions
// are wave-uniform: a trip loads 64 hits of the slicer's hit ring from the state's next_hit on, a lane each; a ballot of
// h >= pos and find-first give h0, a ballot of h >= h0 + 8 gives h1 (at most eight hits start in h0 .. h0 + 7, so h1 is in the
// same 64 unless h0 sits in the last eight lanes -- then the trip is repeated from h0).  A step that cannot be decided yet
// -- the bits are not all in whole words, or case B has no hit -- ends the launch; the state stays where it is and the next
// launch looks again.  Per decided frame the lanes 0 .. 37 are the data bits: each loads its data and its parity bit from
// the word ring through the deinterleave map, two ballots are the masks D and P', and the rest is mask arithmetic that every
// lane does alike: psyn = P' ^ D ^ (D << 1), the correction D ^ (psyn & (psyn >> 1)), the fields; the lanes 0 .. 7 store the
// record's eight words.
// Trips.  At the end of a launch what is undecided is less than 92 + 32 bits behind the cursor or behind h0 (a step waits
// for W >= pos + 84 or W >= h0 + 92, and n_symbols < W + 32), hits and bits before them cost nothing, and a block adds at most
// n_k symbols, so B = n_k + 124 bounds both the bits in play and the hits to look at.  Every decided step moves pos by at
// least 8 bits: at most B / 8 + 1 steps.  A trip without a step moves next_hit by at least 56: at most B / 56 + 1.  One trip
// ends the launch undecided, one skips a frame the word ring has lost (after it pos is inside the ring: once a launch).
// All trip counts come from the host's n_k; the counters read from the device only clamp.  Every ring index is masked.  Plain
// vector stores only; nothing is shared between waves; no LDS.
#include "item_wave.hpp"
#include "osw_core.hpp"

namespace rcfx {

namespace {

constexpr int kOswWaves = kItemWaves;

__global__ __launch_bounds__(64 * kOswWaves) void osw_kernel(const OswLaunch *__restrict__ items, int n_items)
{
    int lane;
    const int w = item_of_wave(n_items, &lane);
    if (w < 0) return;
    const OswLaunch L = items[w];
    OswState *st = L.st;
    const int64_t n_sym = L.src->n_symbols, n_words = L.src->n_words, n_hits = L.src->n_hits, W = 32 * n_words;
    int64_t n_records = st->n_records, n_frames = st->n_frames, n_bad = st->n_bad, n_rejects = st->n_rejects, n_lost = st->n_lost;
    int64_t i = st->next_hit, pos = st->pos;
    int32_t locked = st->locked, is_locked = st->is_locked;
    const int64_t word_cap = (int64_t)L.word_mask + 1, lost = hits_lost(i, n_hits, L.hit_mask);
    n_lost += lost;
    bool resync = lost != 0;                         // after a loss: pos moves to the first retained hit at or behind it
    const int trips = osw_trips(L.n_k);
    for (int t = 0; t < trips; ++t) {
        const bool valid = i + lane < n_hits;
        const uint32_t item = valid ? L.hit_ring[(uint64_t)(i + lane) & L.hit_mask] : 0u;
        const int64_t h = osw_hit_start(item, n_sym);
        const uint64_t ge = __ballot(valid && h >= pos);
        const bool have0 = ge != 0;
        int64_t h0 = 0;
        if (!have0) {
            const int64_t adv = n_hits - i < 64 ? (n_hits - i > 0 ? n_hits - i : 0) : 64;
            i += adv;
            if (adv == 64) continue;                                                         // all before the cursor; there may be more
        } else {
            const int a = __builtin_ctzll(ge);
            i += a;
            if (a > 64 - kOswSyncBits - 1) continue;                                         // h1 may lie past these 64: again, from h0
            h0 = rl_i64(h, a);
        }
        if (resync) { resync = false; if (have0) pos = h0; }
        if (!osw_ready(locked, have0, h0, pos, W)) break;                                    // not all there yet: the next launch
        const uint64_t ge1 = have0 ? __ballot(valid && h >= h0 + kOswSyncBits) : 0;
        const bool have1 = ge1 != 0;
        const int64_t h1 = have1 ? rl_i64(h, __builtin_ctzll(ge1)) : 0;
        bool rel_nz;
        uint32_t rel;
        if (osw_decide(locked, have0, h0, have1, h1, pos, &rel_nz, &rel) == kOswReject) { pos = h0 + kOswSyncBits; ++n_rejects; continue; }
        const int32_t l1 = osw_lock_step(locked, rel_nz);
        const int64_t s = osw_sync_pos(l1, pos, h0);
        if ((s >> 5) < n_words - word_cap) { ++n_lost; pos = 32 * (n_words - word_cap); resync = true; continue; }   // its first word is overwritten
        locked = l1; is_locked = osw_is_locked(l1) ? 1 : 0; ++n_frames;
        // ---- data bit `lane` and its parity bit through the deinterleave map; the masks
        int d = 0, p = 0;
        if (lane < kOswDataBits) {
            const int64_t pd = s + kOswSyncBits + osw_data_bit(lane), pp = s + kOswSyncBits + osw_parity_bit(lane);
            d = osw_word_bit(L.word_ring[(uint64_t)(pd >> 5) & L.word_mask], (int)(pd & 31));
            p = osw_word_bit(L.word_ring[(uint64_t)(pp >> 5) & L.word_mask], (int)(pp & 31));
        }
        uint64_t data = __ballot(d != 0);
        const uint64_t psyn = osw_psyn(data, __ballot(p != 0)), flips = psyn ? osw_flip_mask(psyn) : 0;
        data ^= flips;
        if (psyn) ++n_bad;
        locked = osw_lock_clean(locked, rel_nz, psyn);
        uint32_t *rec = L.rec_ring + ((uint64_t)n_records & L.rec_mask) * kOswRecWords;
        if (lane < kOswRecWords) rec[lane] = osw_rec_word(lane, osw_word0(rel_nz, psyn, is_locked != 0, data, flips, rel), s, data, psyn, locked);
        ++n_records;
        pos = s + kOswFrameBits;
    }
    if (lane == 0) {
        st->n_records = n_records; st->n_frames = n_frames; st->n_bad = n_bad; st->n_rejects = n_rejects; st->n_lost = n_lost;
        st->locked = locked; st->is_locked = is_locked; st->next_hit = i; st->pos = pos;
    }
}

}  // namespace

// ring_mask: unused -- every record carries the masks of its three rings
void launch_osw(const OswLaunch *d_items, int n_items, int max_n_k, uint64_t, hipStream_t s)
{
    launch_item_waves(osw_kernel, d_items, n_items, max_n_k, s);
}

}  // namespace rcfx
