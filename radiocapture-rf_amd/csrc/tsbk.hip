// tsbk.hip -- P25 trunking blocks behind a channel's slicer (gfx950): what the reference's consumer does per frame in Python
// (p25_general.procTSDU, subprocTSBK: strip the status symbols, read the NID, deinterleave each 196-bit block, run the
// rate-1/2 trellis, check the CRC), every such stage of a block (or of a group's block) in one launch directly behind
// slice_kernel's, so that the hits and words of this block are there.  include/rcf.h at rcf_chan_tsbk DEFINES the stage,
// tests/tsbk_ref.py restates it; the arithmetic is tsbk_core.hpp, which the CPU suite compiles for the host as it stands.
//
// The slicer's layout: a WAVE is a channel, four channels per workgroup.  The wave walks the slicer's hit ring from the
// state's next_hit on, 64 hits a trip with a lane each: the accept rule picks the first hit far enough behind the last
// accepted one, the hits behind it give the frame's length.  A frame whose 384 dibits are not all in whole words yet stays
// where it is -- next_hit does not pass it -- and is looked at again in the next launch.  Per decided frame the lanes 0 .. 31
// gather the NID's dibits, and per block the lanes 0 .. 48 are its code words: each gathers its two dibits through the
// status-symbol and deinterleave maps, forms its transition map (four next states in 8 bits), and an inclusive scan of the
// maps under composition -- six cross-lane steps instead of a 49-step dependent chain -- gives every lane its state.  The two
// ballots of the state bits become the three words through the slicer's mask-to-word helper.  The CRC is linear in the
// bits, so it is the xor-reduction over the wave of each lane's two per-bit terms (a 192-byte constant table): six more
// cross-lane steps, where lane 0's loop over 96 bits would be 96 dependent shift / test / xor rounds with every other lane
// idle.  The lanes 0 .. 7 store a record's eight words.
// All trip counts come from the host's n_k; the counters read from the device only clamp.  Every ring index is masked.  Plain
// vector stores only; nothing is shared between waves; no LDS.
// The option RCF_NID_BCH (kNidFlagBch in the launch record's flags): the NID's 63 bits go through nid_wave.hpp's decoder
// before the DUID is looked at, behind a wave-uniform branch that a stage without the option never enters.
// The option RCF_TRELLIS_VITERBI (kTsbkFlagViterbi, likewise): a lane's transition map comes from the least-cost path instead
// of the nearest candidate.  A suffix scan of the code words' min-plus matrices -- six cross-lane steps, four packed registers
// a lane -- leaves beta_t in lane t; with its right neighbour's beta the lane forms the map of the forward step, and the same
// inclusive scan as without the option gives the states.  A ballot counts the words off the path, an add-reduction sums the cost.
#include "item_wave.hpp"
#include "tsbk_core.hpp"
#include "nid_wave.hpp"

namespace rcfx {

namespace {

constexpr int kTsbkWaves = kItemWaves;

// stream dibit p of the slicer's word ring (p inside the whole words: the caller's condition)
__device__ __forceinline__ int ring_dibit(const TsbkLaunch &L, int64_t p)
{
    return tsbk_word_dibit(L.word_ring[(uint64_t)(p >> 4) & L.word_mask], (int)(p & 15));
}

// lane t's transition map on the least-cost path through the code words c of the lanes 0 .. 48 (tsbk_core.hpp).  Out of
// line: inlined, its unrolled compositions raise the kernel's registers past 128 and cost a stage without the option a wave
// of occupancy
__device__ __noinline__ uint32_t viterbi_map_wave(uint32_t c, int lane)
{
    const TsbkMat own = lane < kTsbkCodeWords ? tsbk_mat(c, lane == kTsbkCodeWords - 1) : tsbk_mat_identity();
    TsbkMat suffix = own;                            // the product of the lanes lane .. 63
    for (int d = 1; d < 64; d <<= 1) {
        TsbkMat after;
        for (int s = 0; s < 4; ++s) after.row[s] = (uint32_t)__shfl_down((int)suffix.row[s], d);
        if (lane + d < 64) suffix = tsbk_mat_compose(suffix, after);
    }
    const uint32_t beta_next = (uint32_t)__shfl_down((int)tsbk_mat_beta(suffix), 1);
    if (lane >= kTsbkCodeWords) return kTsbkIdentity;
    return tsbk_viterbi_map(own, lane == kTsbkCodeWords - 1 ? 0u : beta_next);
}

__global__ __launch_bounds__(64 * kTsbkWaves) void tsbk_kernel(const TsbkLaunch *__restrict__ items, int n_items)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * kTsbkWaves + (threadIdx.x >> 6));
    if (w >= n_items) return;                        // (no workgroup barrier below: a wave leaves on its own)
    const TsbkLaunch L = items[w];
    TsbkState *st = L.st;
    const bool nid = L.flags & kNidFlagBch, viterbi = L.flags & kTsbkFlagViterbi;
    NidCount nc;
    int64_t vit_decoded = 0, vit_clean = 0, vit_bits = 0, vit_words = 0;
    const int64_t n_sym = L.src->n_symbols, n_words = L.src->n_words, n_hits = L.src->n_hits;
    int64_t n_records = st->n_records, n_frames = st->n_frames, n_blocks = st->n_blocks, n_crc_bad = st->n_crc_bad, n_lost = st->n_lost;
    int64_t i = st->next_hit, k_last = st->k_last;
    const int64_t hit_cap = (int64_t)L.hit_mask + 1, word_cap = (int64_t)L.word_mask + 1;
    if (i < n_hits - hit_cap) { n_lost += n_hits - hit_cap - i; i = n_hits - hit_cap; }      // hits that left the ring unexamined
    // the host's bounds, whatever the counters say: the hits to look at are this block's (at most one per new symbol) and those
    // of an undecided frame's 384 dibits and the unfinished word; a decided frame costs at most two trips, 64 rejected hits one
    const int bound = L.n_k + kTsbkDecideDibits + 32;
    const int trips = 2 * (bound / kTsbkSyncDibits + 1) + bound / 64 + 2;
    for (int t = 0; t < trips && i < n_hits; ++t) {
        const bool valid = i + lane < n_hits;
        const uint32_t item = valid ? L.hit_ring[(uint64_t)(i + lane) & L.hit_mask] : 0u;
        const int64_t k = tsbk_widen_k(item, n_sym);
        const uint64_t acc = __ballot(valid && tsbk_accept(k, k_last));
        if (!acc) { i += n_hits - i < 64 ? n_hits - i : 64; continue; }                      // all rejected
        const int a = __builtin_ctzll(acc);
        if (a > 32) { i += a; continue; }            // take the chunk again from the accepted hit on: the next frame's hit is among the 24 behind it
        const int64_t k0 = rl_i64(k, a), s = k0 - (kTsbkSyncDibits - 1);
        const uint32_t dist = (uint32_t)__builtin_amdgcn_readlane((int)item, a) >> 26;
        i += a;
        if (16 * n_words < s + kTsbkDecideDibits) break;                                      // not all there yet: the next launch
        const uint64_t nxt = __ballot(valid && lane > a && tsbk_accept(k, k0));
        int fd = kTsbkFrameDibits;
        if (nxt) {
            const int64_t gap = rl_i64(k, __builtin_ctzll(nxt)) - k0;
            if (gap < fd) fd = (int)gap;
        }
        ++i; k_last = k0; ++n_frames;
        if ((s >> 4) < n_words - word_cap) { ++n_lost; continue; }                            // its first word is overwritten
        // ---- the NID: info dibits 24 .. 55
        const int dn = lane < 32 ? ring_dibit(L, s + tsbk_frame_pos(24 + lane)) : 0;
        const uint64_t nhi = __ballot(dn & 2), nlo = __ballot(dn & 1);
        const uint32_t nid0 = slice_word_be(nhi, nlo, 2, 0), nid1 = slice_word_be(nhi, nlo, 2, 1);
        uint32_t nidc = nid0, w7 = (uint32_t)fd;     // nac and duid as the record holds them; word 7
        if (nid) {                                   // (uniform)
            int fix;
            nidc = nid_word0_of(nid_decode_wave(nid_poly(nid0, nid1), lane, &fix));
            w7 |= nid_tsbk_word7(fix);
            nc.add(fix);
        }
        const int nb = tsbk_duid(nidc) == 7 ? tsbk_blocks_in(fd) : 0;
        uint32_t *rec = L.rec_ring + ((uint64_t)n_records & L.rec_mask) * kTsbkRecWords;
        if (nb == 0) {                               // a frame record
            const uint32_t v = lane == 0 ? tsbk_word0(3, false, 0, 0, dist, nidc) : lane == 1 ? (uint32_t)(uint64_t)k0 :
                               lane == 5 ? slice_word_mem(nid0) : lane == 6 ? slice_word_mem(nid1) : lane == 7 ? w7 : 0u;
            if (lane < kTsbkRecWords) rec[lane] = v;
            ++n_records;
            continue;
        }
        for (int b = 0; b < nb; ++b) {
            // ---- code word `lane`: its two dibits through the deinterleaver and past the status symbols
            uint32_t c = 0, map = kTsbkIdentity;
            if (lane < kTsbkCodeWords) {
                const int j = tsbk_block_dibit(b, tsbk_deinterleave(lane));
                c = (uint32_t)(ring_dibit(L, s + tsbk_frame_pos(j)) << 2 | ring_dibit(L, s + tsbk_frame_pos(j + 1)));
                map = tsbk_map(c);
            }
            if (viterbi) map = viterbi_map_wave(c, lane);                                     // (uniform)
            for (int d = 1; d < 64; d <<= 1) {       // the inclusive scan: the map of the code words 0 .. lane
                const uint32_t before = (uint32_t)__shfl_up((int)map, d);
                if (lane >= d) map = tsbk_compose(before, map);
            }
            const int state = (int)(map & 3u);       // from state 0
            const int prev = __shfl_up(state, 1);
            bool exact;
            (void)tsbk_next_state(lane ? prev : 0, c, &exact);
            int n_inexact = __popcll(__ballot(lane < kTsbkCodeWords && !exact));
            uint32_t w7b = w7;
            if (viterbi) {                           // (uniform) the words off the chosen path and the path's cost
                int cost = lane < kTsbkCodeWords ? tsbk_branch_dist(lane ? prev : 0, state, c) : 0;
                n_inexact = __popcll(__ballot(cost != 0));
                for (int m = 32; m; m >>= 1) cost += __shfl_xor(cost, m);
                w7b |= tsbk_viterbi_word7(cost);
                ++vit_decoded; vit_clean += cost == 0 ? 1 : 0; vit_bits += cost; vit_words += n_inexact;
            }
            const bool out = lane < 48;              // the first 48 states are the 96 bits
            const uint64_t hi = __ballot(out && (state & 2)), lo = __ballot(out && (state & 1));
            uint32_t crc = out ? tsbk_crc_term(lane, state) : 0u;
            for (int m = 32; m; m >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, m);
            const bool crc_bad = crc != 0xffffu;
            const int jn = tsbk_frame_pos(tsbk_block_dibit(b, 98));                           // the info bit behind the block
            const int next_bit = jn < fd ? ring_dibit(L, s + jn) >> 1 : 0;
            rec = L.rec_ring + ((uint64_t)n_records & L.rec_mask) * kTsbkRecWords;
            const uint32_t v = lane == 0 ? tsbk_word0(b, crc_bad, next_bit, n_inexact, dist, nidc) : lane == 1 ? (uint32_t)(uint64_t)k0 :
                               lane < 5 ? slice_word_mem(slice_word_be(hi, lo, 2, lane - 2)) :
                               lane == 5 ? slice_word_mem(nid0) : lane == 6 ? slice_word_mem(nid1) : w7b;
            if (lane < kTsbkRecWords) rec[lane] = v;
            ++n_records; ++n_blocks;
            n_crc_bad += crc_bad ? 1 : 0;
        }
    }
    if (lane == 0) {
        st->n_records = n_records; st->n_frames = n_frames; st->n_blocks = n_blocks; st->n_crc_bad = n_crc_bad; st->n_lost = n_lost;
        st->next_hit = i; st->k_last = k_last;
        if (nid) { st->nid_decoded += nc.decoded; st->nid_fixed += nc.fixed; st->nid_bits += nc.bits; st->nid_bad += nc.bad; }
        if (viterbi) { st->vit_decoded += vit_decoded; st->vit_clean += vit_clean; st->vit_bits += vit_bits; st->vit_words += vit_words; }
    }
}

}  // namespace

// ring_mask: unused -- every record carries the masks of its three rings
void launch_tsbk(const TsbkLaunch *d_items, int n_items, int max_n_k, uint64_t, hipStream_t s)
{
    launch_item_waves(tsbk_kernel, d_items, n_items, max_n_k, s);
}

}  // namespace rcfx
