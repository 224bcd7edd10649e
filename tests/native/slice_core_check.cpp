// slice_core_check.cpp -- radiocapture-rf_amd/csrc/slice_core.hpp compiled for the host: a stand-alone walk of the
// hard-decision stage over a file of float32 soft symbols, block by block as slice_kernel (slice.hip) walks them -- the 64
// lanes of a wave as a loop, a ballot as the mask that loop builds -- with every decision, word and window coming from the
// header's own functions.  Prints the counts and an FNV-1a digest of the words (as bytes in memory order) followed by the
// hit items; tests/test_slicer_cpu.py holds it to the numpy restatement's (tests/slicer_ref.py).
//   slice_core_check <soft.f32> <bps> <sync_word hex> <sync_bits> <max_errors> [cut ...]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define RCF_DEVFN static inline
#include "../../radiocapture-rf_amd/csrc/slice_core.hpp"

using namespace rcfx;

namespace {

struct State { int64_t n_words = 0, n_symbols = 0, n_hits = 0; uint32_t partial = 0; uint64_t tail = 0; };
struct Params { int bps, sync_bits, max_errors; uint64_t sync_word; float levels[3]; };

// one block: n_new symbols from soft[st.n_symbols] on (slice_kernel's loop, one wave)
void block(const Params &p, State &st, const std::vector<float> &soft, int n_new, std::vector<uint32_t> &words, std::vector<uint32_t> &hits)
{
    if (n_new <= 0) return;
    const int bps = p.bps, spw = 32 / bps, sync_syms = p.sync_bits / bps;
    const int64_t n_sym0 = st.n_symbols, k_end = n_sym0 + n_new;
    uint64_t before = 0;
    int t = 0;
    for (int64_t kb = n_sym0 & ~(int64_t)63; kb < k_end; kb += 64, ++t) {
        const int a = (int)(n_sym0 > kb ? n_sym0 - kb : 0);
        const int b = (int)(k_end - kb < 64 ? k_end - kb : 64);
        uint64_t hi = 0, lo = 0;
        for (int lane = a; lane < b; ++lane) {
            const float s = soft[(size_t)(kb + lane)];
            const int d = bps == 1 ? slice_binary(s) : slice_fsk4(s, p.levels[0], p.levels[1], p.levels[2]);
            hi |= (uint64_t)((d >> 1) & 1) << lane;
            lo |= (uint64_t)(d & 1) << lane;
        }
        for (int lane = 0; lane < 4; ++lane) {
            uint32_t be;
            if (slice_lane_word(hi, lo, bps, a, b, st.partial, lane, &be)) words.push_back(slice_word_mem(be));
        }
        st.partial = slice_partial_after(hi, lo, bps, a, b, st.partial);
        st.n_words += b / spw - a / spw;
        uint64_t u0 = slice_unit(hi, lo, bps, 0), u1 = bps == 2 ? slice_unit(hi, lo, bps, 1) : 0ull;
        if (t == 0) {
            const int o = bps * a;
            before = slice_place_tail(st.tail, o, 0);
            u0 |= slice_place_tail(st.tail, o, 1);
            u1 |= slice_place_tail(st.tail, o, 2);
        }
        for (int lane = a; lane < b; ++lane) {
            const int64_t k = kb + lane;
            const uint64_t win = slice_window(before, u0, u1, bps, lane);
            if (p.sync_bits && k >= sync_syms - 1) {
                const int dist = slice_sync_dist(win, p.sync_word, p.sync_bits);
                if (dist <= p.max_errors) { hits.push_back(slice_hit_item(dist, k)); ++st.n_hits; }
            }
            if (lane == b - 1) st.tail = win;
        }
        before = bps == 2 ? u1 : u0;
    }
    st.n_symbols = k_end;
}

uint64_t fnv(uint64_t h, uint32_t w)
{
    for (int i = 0; i < 4; ++i) { h ^= (w >> (8 * i)) & 0xffu; h *= 0x100000001b3ull; }
    return h;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 6) { fprintf(stderr, "usage: %s soft.f32 bps sync_word_hex sync_bits max_errors [cut ...]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> soft;
    float buf[4096];
    for (size_t n; (n = fread(buf, sizeof(float), 4096, f)) > 0;) soft.insert(soft.end(), buf, buf + n);
    fclose(f);
    Params p{atoi(argv[2]), atoi(argv[4]), atoi(argv[5]), strtoull(argv[3], nullptr, 16), {-2.0f, 0.0f, 2.0f}};
    if (p.bps != 1 && p.bps != 2) return 2;
    if (p.sync_bits < 64) p.sync_word &= (1ull << p.sync_bits) - 1;
    std::vector<int64_t> edges{0};
    for (int i = 6; i < argc; ++i) edges.push_back(atoll(argv[i]));
    edges.push_back((int64_t)soft.size());
    State st;
    std::vector<uint32_t> words, hits;
    for (size_t i = 0; i + 1 < edges.size(); ++i) {
        if (edges[i + 1] < edges[i] || edges[i + 1] > (int64_t)soft.size()) return 2;
        block(p, st, soft, (int)(edges[i + 1] - edges[i]), words, hits);
    }
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t w : words) h = fnv(h, w);
    for (uint32_t w : hits) h = fnv(h, w);
    printf("symbols %" PRId64 " words %" PRId64 " hits %" PRId64 " digest %016" PRIx64 "\n", st.n_symbols, st.n_words, st.n_hits, h);
    return st.n_words == (int64_t)words.size() && st.n_hits == (int64_t)hits.size() ? 0 : 1;
}
