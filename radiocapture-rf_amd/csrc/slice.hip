// slice.hip -- hard decisions behind a channel's symbol loop (gfx950): binary_slicer_fb (moto_control_demod.py:114,
// edacs_control_demod.py:86) or op25's fsk4_slicer_fb (p25_control_demod.py:167-168, logging_receiver.py:250-251), the
// packing of unpacked_to_packed_bb(bps, GR_MSB_FIRST), and the consumers' search for the frame-sync word
// (p25_control_demod.py:337, moto_control_demod.py:216, edacs_control_demod.py:523), every slicer of a block (or of a
// group's block) in one launch behind the three loops' launches.  include/rcf.h at rcf_chan_slicer DEFINES the stage,
// tests/slicer_ref.py restates it; the arithmetic is slice_core.hpp, which the CPU suite compiles for the host as it stands.
//
// The work is elementwise on the few hundred symbols a block gives a channel, so -- unlike the loops, where a lane is a
// channel -- a WAVE is a channel and its lanes are symbols; four channels per workgroup.  The wave reads the loop's counter,
// takes new = min(n_out - src0 - n_symbols, n_k) symbols and walks them in chunks of 64 aligned to multiples of 64 of the
// stage's own symbol index k: a whole chunk is then exactly 2 (binary) or 4 (FSK4) whole words, and only the first and the
// last chunk of a block meet the unfinished word of the state record.  Per chunk: one coalesced 256-byte load of soft
// symbols, the decisions' bits as lane masks (ballot), the words assembled from the masks by the lanes 0 .. 3, each lane's
// 64-bit window as a funnel shift over (the 64 bits before : the chunk's bits), and the hits' places in the ring from a
// ballot of the hit lanes and a prefix popcount.  The trip count comes from the host's n_k, never from the device counter.
// Plain vector stores only; nothing is shared between waves.
#include "item_wave.hpp"
#include "slice_core.hpp"

namespace rcfx {

namespace {

constexpr int kSliceWaves = kItemWaves;

__global__ __launch_bounds__(64 * kSliceWaves) void slice_kernel(const SliceLaunch *__restrict__ items, int n_items)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * kSliceWaves + (threadIdx.x >> 6));
    if (w >= n_items) return;                        // (no workgroup barrier below: a wave leaves on its own)
    const SliceLaunch L = items[w];
    SliceState *st = L.st;
    const int64_t n_sym0 = st->n_symbols;
    int64_t n_words = st->n_words, n_hits = st->n_hits;
    uint32_t partial = st->partial;
    uint64_t tail = st->tail;
    const int64_t avail = *L.src_n_out - L.src0 - n_sym0;
    const int n_new = (int)(avail < 0 ? 0 : avail > (int64_t)L.n_k ? (int64_t)L.n_k : avail);
    if (n_new <= 0) return;
    const int bps = L.bps, spw = 32 / bps;
    const int sync_syms = L.sync_bits / bps;
    const int64_t k_end = n_sym0 + n_new;
    const int trips = (L.n_k + 126) >> 6;            // ceil((n_k + 63) / 64): the host's bound, whatever the counter says
    const uint64_t below = lane ? ~0ull >> (64 - lane) : 0ull;           // the lanes before this one
    uint64_t before = 0;                             // the 64 bits of the stream in front of the chunk
    int64_t kb = n_sym0 & ~(int64_t)63;
    for (int t = 0; t < trips && kb < k_end; ++t, kb += 64) {
        const int a = (int)(n_sym0 > kb ? n_sym0 - kb : 0);              // the chunk's new lanes [a, b)
        const int b = (int)(k_end - kb < 64 ? k_end - kb : 64);
        const int64_t k = kb + lane;
        const bool valid = lane >= a && lane < b;
        const float s = valid ? L.soft_ring[(uint64_t)(L.src0 + k) & L.soft_mask] : 0.0f;
        const int d = bps == 1 ? slice_binary(s) : slice_fsk4(s, L.levels[0], L.levels[1], L.levels[2]);
        const uint64_t hi = __ballot(valid && (d & 2)), lo = __ballot(valid && (d & 1));
        // ---- words: those the chunk makes whole go out from the lanes 0 .. 3, the rest stays in `partial`
        uint32_t be;
        if (slice_lane_word(hi, lo, bps, a, b, partial, lane, &be)) L.word_ring[(uint64_t)(n_words + lane) & L.word_mask] = slice_word_mem(be);
        partial = slice_partial_after(hi, lo, bps, a, b, partial);
        n_words += b / spw - a / spw;
        // ---- the chunk as units of the stream; in the block's first chunk the lanes before `a` and the bits in front of
        // the chunk come out of the state's tail
        uint64_t u0 = slice_unit(hi, lo, bps, 0), u1 = bps == 2 ? slice_unit(hi, lo, bps, 1) : 0ull;
        if (t == 0) {
            const int o = bps * a;
            before = slice_place_tail(tail, o, 0);
            u0 |= slice_place_tail(tail, o, 1);
            u1 |= slice_place_tail(tail, o, 2);
        }
        const uint64_t win = slice_window(before, u0, u1, bps, lane);
        // ---- sync hits, in increasing k: place = hits so far + hit lanes before this one; of more hits than the ring
        // holds only the newest are stored (two lanes of one store never meet in a slot)
        if (L.sync_bits) {
            const int dist = slice_sync_dist(win, L.sync_word, L.sync_bits);
            const bool hit = valid && k >= (int64_t)(sync_syms - 1) && slice_is_hit(dist, L.sync_bits, L.sync_max_errors, L.sync_both);
            const uint64_t hits = __ballot(hit);
            const int n_here = __popcll(hits), mine = __popcll(hits & below);
            if (hit && n_here - mine <= (int)L.hit_mask + 1)
                L.hit_ring[(uint64_t)(n_hits + mine) & L.hit_mask] = slice_hit_item(dist, k);
            n_hits += n_here;
        }
        tail = rl_u64(win, b - 1);                   // the stream's last 64 bits so far
        before = bps == 2 ? u1 : u0;
    }
    if (lane == 0) {
        st->n_words = n_words; st->n_symbols = k_end; st->n_hits = n_hits;
        st->partial = partial; st->tail = tail;
    }
}

}  // namespace

// ring_mask: unused -- every record carries the masks of its three rings (the hit ring has a capacity of its own)
void launch_slice(const SliceLaunch *d_items, int n_items, int max_n_k, uint64_t, hipStream_t s)
{
    launch_item_waves(slice_kernel, d_items, n_items, max_n_k, s);
}

}  // namespace rcfx
