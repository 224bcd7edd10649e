// wave_host.hpp -- what the check programs of the decoders behind a slicer share: a wave on the host -- the 64 lanes as a loop,
// a ballot as the mask that loop builds, a reduction as the xor over the lanes' array -- the slicer's two streams, the file
// reader, and the frame walk of radiocapture-rf_amd/csrc/item_wave.hpp's frame_walk, lane by lane, over a stage's constants
// (slice_core.hpp at slice_walk_trips).  Include it behind the stage's *_core.hpp, with RCF_DEVFN defined.
#pragma once
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../radiocapture-rf_amd/csrc/slice_core.hpp"

namespace {

using namespace rcfx;

typedef uint32_t Lanes[64];

uint64_t ballot(const bool (&b)[64])
{
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)b[l] << l;
    return m;
}
uint32_t wave_xor(const Lanes &v)
{
    uint32_t r = 0;
    for (int l = 0; l < 64; ++l) r ^= v[l];
    return r;
}

struct Rings {
    std::vector<uint32_t> words, hits;          // the streams from word base_words / hit base_hits on: ring index i & mask of a ring that has lost nothing yet
    uint32_t word_mask, hit_mask;
    int64_t base_words = 0, base_hits = 0;
    uint32_t word(int64_t i) const { return words.at((size_t)(i - base_words)); }    // (.at: a read outside what the slicer has written aborts)
    uint32_t hit(int64_t i) const { return hits.at((size_t)(i - base_hits)); }
    bool holds(int64_t n_words, int64_t n_hits) const { return n_words - base_words <= (int64_t)words.size() && n_hits - base_hits <= (int64_t)hits.size(); }
};

template <class T> std::vector<T> read_file(const char *path)
{
    std::vector<T> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    T buf[4096];
    for (size_t n; (n = fread(buf, sizeof(T), 4096, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

void print_records(const std::vector<uint32_t> &out)
{
    for (size_t r = 0; r + 8 <= out.size(); r += 8)
        for (int q = 0; q < 8; ++q) printf("%08x%s", out[r + q], q == 7 ? "\n" : " ");
}

// a stage's counters: n_a and n_b are its own two (blocks and crc_bad, decoded and rs_bad, msgs and msgs_none)
struct State {
    int64_t n_records = 0, n_frames = 0, n_a = 0, n_b = 0, n_lost = 0, next_hit = 0, k_last = -((int64_t)1 << 60);   // (kTsbkNoFrame, kEdacsNoFrame)
};

// one launch of the frame walk (one wave); frame(s, fd, k0, dist) decodes one decided frame
template <class W, class Frame>
void walk(const Rings &R, State &st, int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k, Frame &&frame)
{
    constexpr int kWordShift = W::kPerWord == 16 ? 4 : 5;
    int64_t i = st.next_hit, k_last = st.k_last;
    const int64_t hit_cap = (int64_t)R.hit_mask + 1, word_cap = (int64_t)R.word_mask + 1;
    if (i < n_hits - hit_cap) { st.n_lost += n_hits - hit_cap - i; i = n_hits - hit_cap; }
    const int trips = slice_walk_trips<W>(n_k);
    for (int t = 0; t < trips && i < n_hits; ++t) {
        bool valid[64], accb[64];
        uint32_t item[64];
        int64_t k[64];
        for (int l = 0; l < 64; ++l) {
            valid[l] = i + l < n_hits;
            item[l] = valid[l] ? R.hit(i + l) : 0u;
            k[l] = slice_widen_k(item[l], n_sym);
            accb[l] = valid[l] && k[l] >= k_last + W::kAccept;
        }
        const uint64_t acc = ballot(accb);
        if (!acc) { i += n_hits - i < 64 ? n_hits - i : 64; continue; }
        const int a = __builtin_ctzll(acc);
        if (W::kCut && a > 32) { i += a; continue; }
        const int64_t k0 = k[a], s = k0 - (W::kSync - 1);
        const uint32_t dist = item[a] >> 26;
        i += a;
        if (W::kPerWord * n_words < s + W::kDecide) break;
        int fd = W::kLongest;
        if (W::kCut) {
            bool nb_[64];
            for (int l = 0; l < 64; ++l) nb_[l] = valid[l] && l > a && k[l] >= k0 + W::kAccept;
            const uint64_t nxt = ballot(nb_);
            if (nxt) {
                const int64_t gap = k[__builtin_ctzll(nxt)] - k0;
                if (gap < fd) fd = (int)gap;
            }
        }
        ++i; k_last = k0; ++st.n_frames;
        if ((s >> kWordShift) < n_words - word_cap) { ++st.n_lost; continue; }
        frame(s, fd, k0, dist);
    }
    st.next_hit = i; st.k_last = k_last;
}

// the launches of a stream program's command line, a quadruple <n_words n_hits n_symbols n_k> each from argv[first] on:
// launch(n_words, n_hits, n_symbols, n_k) per quadruple; false: the streams' files do not hold a launch
template <class Launch> bool for_launches(const Rings &R, int argc, char **argv, int first, Launch &&launch)
{
    for (int i = first; i + 3 < argc; i += 4) {
        const int64_t n_words = atoll(argv[i]), n_hits = atoll(argv[i + 1]);
        if (!R.holds(n_words, n_hits)) return false;
        launch(n_words, n_hits, atoll(argv[i + 2]), atoi(argv[i + 3]));
    }
    return true;
}

}  // namespace
