// item_wave.hpp -- what the kernels in the slicer's layout share (slice.hip, tsbk.hip, edacs.hip, osw.hip, p25lc.hip): a WAVE is an
// item (a channel's stage), four items per workgroup, nothing shared between the waves.  Here are the lane reads and
// reductions, the item prologue, the frame walk of the decoders behind a slicer and the launcher.
#pragma once
#include "rcf_internal.h"
#include "slice_core.hpp"

namespace rcfx {

namespace {

constexpr int kItemWaves = 4;

__device__ __forceinline__ uint64_t rl_u64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int64_t rl_i64(int64_t v, int src) { return (int64_t)rl_u64((uint64_t)v, src); }
// v of lane src mod 64
__device__ __forceinline__ uint32_t lane_read(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src & 63); }
// the reduction of v over the wave under op (associative, commutative), in every lane: six cross-lane steps
template <class Op> __device__ __forceinline__ uint32_t wave_reduce(uint32_t v, Op op)
{
    for (int m = 32; m; m >>= 1) v = op(v, (uint32_t)__shfl_xor((int)v, m));
    return v;
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return a ^ b; }); }
__device__ __forceinline__ int wave_add(int v) { return (int)wave_reduce((uint32_t)v, [](uint32_t a, uint32_t b) { return a + b; }); }

// The item prologue: *lane and the wave's item index (uniform), or -1 -- the wave has no item and leaves (the kernels have no
// workgroup barrier: a wave leaves on its own)
__device__ __forceinline__ int item_of_wave(int n_items, int *lane)
{
    *lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * kItemWaves + (threadIdx.x >> 6));
    return w < n_items ? w : -1;
}

// The hits that left the slicer's hit ring unexamined: next_hit i moves to the oldest hit the ring holds; how many it passed
__device__ __forceinline__ int64_t hits_lost(int64_t &i, int64_t n_hits, uint32_t hit_mask)
{
    const int64_t hit_cap = (int64_t)hit_mask + 1, lost = i < n_hits - hit_cap ? n_hits - hit_cap - i : 0;
    i += lost;
    return lost;
}

// ---- The frame walk (TSBK, P25 voice, EDACS; W: the stage's constants, slice_core.hpp at slice_walk_trips).  The wave walks
// the slicer's hit ring from the state's next_hit on, 64 hits a trip with a lane each.  The accept rule picks the first hit
// at least W::kAccept behind the last accepted one; with W::kCut the accepted hits behind it in the same 64 give the frame's
// length (the next one is among the kAccept hits behind it, so a hit accepted past lane 32 has the chunk taken again from
// it on).  A frame whose W::kDecide symbols are not all in whole words yet stays where it is -- next_hit does not pass it --
// and is looked at again in the next launch.  A decided frame whose first word the word ring has overwritten is counted as
// lost, like the hits that left the hit ring unexamined.  The trips come from the host's n_k; the counters read from the
// device only clamp.  Every ring index is masked.  Every cross-lane operation stands in wave-uniform control flow: i, k_last
// and all that is decided from the ballots are the same in every lane.
// This part of a stage's state is the walk's:
struct FrameWalk {
    int64_t i, k_last, n_frames, n_lost;
    template <class State> __device__ __forceinline__ explicit FrameWalk(const State *st)
        : i(st->next_hit), k_last(st->k_last), n_frames(st->n_frames), n_lost(st->n_lost) {}
    template <class State> __device__ __forceinline__ void store(State *st) const
    {
        st->next_hit = i; st->k_last = k_last; st->n_frames = n_frames; st->n_lost = n_lost;
    }
};
// body(s, fd, k0, dist) for every decided frame the word ring still holds: s its first symbol, fd its length in symbols, k0
// its hit's k and dist the hit's distance field.  (The body is inlined: one call site.)
template <class W, class State, class Body>
__device__ __forceinline__ void frame_walk(const FramesLaunch<State> &L, int lane, FrameWalk &wk, Body &&body)
{
    constexpr int kWordShift = W::kPerWord == 16 ? 4 : 5;
    const int64_t n_sym = L.src->n_symbols, n_words = L.src->n_words, n_hits = L.src->n_hits;
    const int64_t word_cap = (int64_t)L.word_mask + 1;
    int64_t i = wk.i, k_last = wk.k_last, n_frames = wk.n_frames, n_lost = wk.n_lost;
    n_lost += hits_lost(i, n_hits, L.hit_mask);
    const int trips = slice_walk_trips<W>(L.n_k);
    for (int t = 0; t < trips && i < n_hits; ++t) {
        const bool valid = i + lane < n_hits;
        const uint32_t item = valid ? L.hit_ring[(uint64_t)(i + lane) & L.hit_mask] : 0u;
        const int64_t k = slice_widen_k(item, n_sym);
        const uint64_t acc = __ballot(valid && k >= k_last + W::kAccept);
        if (!acc) { i += n_hits - i < 64 ? n_hits - i : 64; continue; }                      // all rejected
        const int a = __builtin_ctzll(acc);
        if (W::kCut && a > 32) { i += a; continue; }                                         // take the chunk again from the accepted hit on
        const int64_t k0 = rl_i64(k, a), s = k0 - (W::kSync - 1);
        const uint32_t dist = (uint32_t)__builtin_amdgcn_readlane((int)item, a) >> 26;
        i += a;
        if (W::kPerWord * n_words < s + W::kDecide) break;                                   // not all there yet: the next launch
        int fd = W::kLongest;
        if (W::kCut) {
            const uint64_t nxt = __ballot(valid && lane > a && k >= k0 + W::kAccept);
            if (nxt) {
                const int64_t gap = rl_i64(k, __builtin_ctzll(nxt)) - k0;
                if (gap < fd) fd = (int)gap;
            }
        }
        ++i; k_last = k0; ++n_frames;
        if ((s >> kWordShift) < n_words - word_cap) { ++n_lost; continue; }                  // its first word is overwritten
        body(s, fd, k0, dist);
    }
    wk.i = i; wk.k_last = k_last; wk.n_frames = n_frames; wk.n_lost = n_lost;
}

// one wave per record, kItemWaves to a workgroup (the records carry their rings' masks: no ring_mask)
template <class Rec>
void launch_item_waves(void (*kernel)(const Rec *, int), const Rec *d_items, int n_items, int max_n_k, hipStream_t s)
{
    if (n_items <= 0 || max_n_k <= 0) return;
    hipLaunchKernelGGL(kernel, dim3((n_items + kItemWaves - 1) / kItemWaves), dim3(64 * kItemWaves), 0, s, d_items, n_items);
}

}  // namespace

}  // namespace rcfx
