// tsbk.hip -- P25 trunking blocks behind a channel's slicer (gfx950): what the reference's consumer does per frame in Python
// (p25_general.procTSDU, subprocTSBK: strip the status symbols, read the NID, deinterleave each 196-bit block, run the
// rate-1/2 trellis, check the CRC), every such stage of a block (or of a group's block) in one launch directly behind
// slice_kernel's, so that the hits and words of this block are there.  include/rcf.h at rcf_chan_tsbk DEFINES the stage,
// tests/tsbk_ref.py restates it; the arithmetic is tsbk_core.hpp, which the CPU suite compiles for the host as it stands.
//
// The slicer's layout: a WAVE is a channel, four channels per workgroup.  The walk over the slicer's hit ring -- the accept
// rule, the frame's length from the hits behind it, the frame that waits for its 384 dibits -- is item_wave.hpp's frame_walk
// with tsbk_core.hpp's TsbkWalk.  Per decided frame the lanes 0 .. 31 gather the NID's dibits (nid_wave.hpp), and per block
// the lanes 0 .. 48 are its code words: each gathers its two dibits through the status-symbol and deinterleave maps, forms
// its transition map (four next states in 8 bits), and an inclusive scan of the maps under composition -- six cross-lane steps instead of a 49-step dependent chain -- gives every lane its state.  The two
// ballots of the state bits become the three words through the slicer's mask-to-word helper.  The CRC is linear in the
// bits, so it is the xor-reduction over the wave of each lane's two per-bit terms (a 192-byte constant table): six more
// cross-lane steps, where lane 0's loop over 96 bits would be 96 dependent shift / test / xor rounds with every other lane
// idle.  The lanes 0 .. 7 store a record's eight words.
// Plain vector stores only; nothing is shared between waves; no LDS.
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
    int lane;
    const int w = item_of_wave(n_items, &lane);
    if (w < 0) return;
    const TsbkLaunch L = items[w];
    TsbkState *st = L.st;
    const bool nid = L.flags & kNidFlagBch, viterbi = L.flags & kTsbkFlagViterbi;
    NidCount nc;
    int64_t vit_decoded = 0, vit_clean = 0, vit_bits = 0, vit_words = 0;
    int64_t n_records = st->n_records, n_blocks = st->n_blocks, n_crc_bad = st->n_crc_bad;
    FrameWalk walk(st);
    frame_walk<TsbkWalk>(L, lane, walk, [&](int64_t s, int fd, int64_t k0, uint32_t dist) __attribute__((always_inline)) {
        const Nid id = read_nid(L, s, lane, nid, nc);
        const uint32_t nid0 = id.nid0, nid1 = id.nid1, nidc = id.word0;                       // nidc: nac and duid as the record holds them
        const uint32_t w7 = (uint32_t)fd | (nid ? nid_tsbk_word7(id.fix) : 0u);              // word 7
        const int nb = tsbk_duid(nidc) == 7 ? tsbk_blocks_in(fd) : 0;
        uint32_t *rec = L.rec_ring + ((uint64_t)n_records & L.rec_mask) * kTsbkRecWords;
        if (nb == 0) {                               // a frame record
            const uint32_t v = lane == 0 ? tsbk_word0(3, false, 0, 0, dist, nidc) : lane == 1 ? (uint32_t)(uint64_t)k0 :
                               lane == 5 ? slice_word_mem(nid0) : lane == 6 ? slice_word_mem(nid1) : lane == 7 ? w7 : 0u;
            if (lane < kTsbkRecWords) rec[lane] = v;
            ++n_records;
            return;
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
                cost = wave_add(cost);
                w7b |= tsbk_viterbi_word7(cost);
                ++vit_decoded; vit_clean += cost == 0 ? 1 : 0; vit_bits += cost; vit_words += n_inexact;
            }
            const bool out = lane < 48;              // the first 48 states are the 96 bits
            const uint64_t hi = __ballot(out && (state & 2)), lo = __ballot(out && (state & 1));
            const bool crc_bad = wave_xor(out ? tsbk_crc_term(lane, state) : 0u) != 0xffffu;
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
    });
    if (lane == 0) {
        st->n_records = n_records; st->n_blocks = n_blocks; st->n_crc_bad = n_crc_bad;
        walk.store(st);
        if (nid) nc.store(st);
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
