// edacs.hip -- EDACS control frames behind a channel's slicer (gfx950): what the reference's consumer does per 288-bit frame
// in Python strings (edacs_control_demod.py: get_next_frame, packet_framer, bch_decode, message_election), every such stage
// of a block (or of a group's block) in one launch behind slice_kernel's, so that the hits and words of this block are
// there.  include/rcf.h at rcf_chan_edacs DEFINES the stage, tests/edacs_ref.py restates it; the arithmetic is
// edacs_core.hpp, which the CPU suite compiles for the host as it stands.
//
// The slicer's layout: a WAVE is a channel, four channels per workgroup.  The walk over the slicer's hit ring is
// item_wave.hpp's frame_walk with edacs_core.hpp's EdacsWalk: the accept rule picks the first hit a whole frame behind the last
// accepted one, and a frame waits for its 288 bits.  Per decided frame the lanes 0 .. 39 are the coefficients of the six copies'
// received polynomials: each gathers its six bits (polarity and the middle copies' inversion applied), a ballot per copy is
// the copy's 40-bit value, and the twelve 6-bit syndromes S1, S3 -- packed two copies to a register -- are three
// xor-reductions over the wave of six steps each, where the reference walks 48 coefficients four times per copy.  What
// follows is wave-uniform: the class of each syndrome pair, and for a pair that needs the Chien search its 63 trials are 63
// lanes and the error positions a ballot; corrections are xor masks on the copies' values, the election compares them, and
// the lanes 0 .. 7 store the record's eight words.
// Every ring index is masked.  Plain vector stores only; nothing is shared between waves; no LDS.
#include "item_wave.hpp"
#include "edacs_core.hpp"

namespace rcfx {

namespace {

constexpr int kEdacsWaves = kItemWaves;

__global__ __launch_bounds__(64 * kEdacsWaves) void edacs_kernel(const EdacsLaunch *__restrict__ items, int n_items)
{
    int lane;
    const int w = item_of_wave(n_items, &lane);
    if (w < 0) return;
    const EdacsLaunch L = items[w];
    EdacsState *st = L.st;
    int64_t n_records = st->n_records, n_msgs = st->n_msgs, n_msgs_none = st->n_msgs_none;
    const bool sync_both = L.flags & kEdacsFlagBoth, esk = L.flags & kEdacsFlagEsk;
    const uint32_t term = lane < kEdacsCopyBits ? edacs_syn_term(lane) : 0u;                // what this lane's coefficient adds to (S1, S3)
    FrameWalk walk(st);
    frame_walk<EdacsWalk>(L, lane, walk, [&](int64_t s, int, int64_t k0, uint32_t raw) __attribute__((always_inline)) {
        const bool inverted = edacs_inverted(raw, sync_both);
        // ---- coefficient `lane` of the six copies; the copies' values; the syndromes, two copies to a register
        uint64_t val[kEdacsCopies];
        uint32_t syn[kEdacsCopies / 2] = {0u, 0u, 0u};
#pragma unroll
        for (int c = 0; c < kEdacsCopies; ++c) {
            int bit = 0;
            if (lane < kEdacsCopyBits) {
                const int64_t p = s + edacs_coef_bit(c, lane);
                bit = edacs_word_bit(L.word_ring[(uint64_t)(p >> 5) & L.word_mask], (int)(p & 31)) ^ (inverted != edacs_copy_inverted(c) ? 1 : 0);
            }
            val[c] = __ballot(bit != 0);
            if (bit) syn[c >> 1] ^= term << (12 * (c & 1));
        }
#pragma unroll
        for (int q = 0; q < kEdacsCopies / 2; ++q) syn[q] = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_xor(syn[q]));
        // ---- per copy, wave-uniform: class, positions, correction
        int status[kEdacsCopies];
        uint32_t statuses = 0;
#pragma unroll
        for (int c = 0; c < kEdacsCopies; ++c) {
            int p, e1, e2;
            const int cls = edacs_classify((syn[c >> 1] >> (12 * (c & 1))) & 0xfffu, &p, &e1, &e2);
            uint64_t pos = 0, flip;
            if (cls == 1) pos = (uint64_t)1 << p;
            else if (cls == 2) pos = __ballot(lane < 63 && edacs_chien_trial(e1, e2, lane ? lane : 63));   // lane = position i % 63
            status[c] = edacs_copy_status(cls, pos, &flip);
            val[c] ^= flip;
            statuses |= (uint32_t)status[c] << (2 * c);
        }
        uint64_t m1, m2;
        const bool has1 = edacs_elect(status[0], status[1], status[2], val[0], val[1], val[2], &m1);
        const bool has2 = edacs_elect(status[3], status[4], status[5], val[3], val[4], val[5], &m2);
        if (has1) m1 = edacs_esk(m1, esk);
        if (has2) m2 = edacs_esk(m2, esk);
        uint32_t *rec = L.rec_ring + ((uint64_t)n_records & L.rec_mask) * kEdacsRecWords;
        const uint32_t v = lane == 0 ? edacs_word0(inverted, has1, has2, edacs_hit_dist(raw, inverted), statuses) :
                           lane == 1 ? (uint32_t)(uint64_t)k0 :
                           lane < 4 ? edacs_msg_word(m1, lane - 2) : lane < 6 ? edacs_msg_word(m2, lane - 4) : 0u;
        if (lane < kEdacsRecWords) rec[lane] = v;
        ++n_records;
        n_msgs += (has1 ? 1 : 0) + (has2 ? 1 : 0);
        n_msgs_none += (has1 ? 0 : 1) + (has2 ? 0 : 1);
    });
    if (lane == 0) {
        st->n_records = n_records; st->n_msgs = n_msgs; st->n_msgs_none = n_msgs_none;
        walk.store(st);
    }
}

}  // namespace

// ring_mask: unused -- every record carries the masks of its three rings
void launch_edacs(const EdacsLaunch *d_items, int n_items, int max_n_k, uint64_t, hipStream_t s)
{
    launch_item_waves(edacs_kernel, d_items, n_items, max_n_k, s);
}

}  // namespace rcfx
