// tsbk_core_check.cpp -- radiocapture-rf_amd/csrc/tsbk_core.hpp compiled for the host: a stand-alone walk of the P25
// trunking stage over the slicer's two streams, launch by launch as tsbk_kernel (tsbk.hip) walks them -- the 64 lanes of a
// wave as a loop, a ballot as the mask that loop builds, a shuffle as an index into the lanes' array -- with every index map,
// transition map, composition, CRC term and record word coming from the header's own functions.
//   tsbk_core_check stream <words.u32> <hits.u32> <first_hit> <word_cap> <hit_cap> <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; prints the five counters, then every record as 8 hex words
//   tsbk_core_check scan <seed> <n>       n random blocks of 49 code words: the six-step scan against the 49-step walk
//   tsbk_core_check pairs                 all 64 (state, code word) pairs: next state and whether a candidate is exact
//   tsbk_core_check widen <item hex> <n_symbols>
// tests/test_tsbk_cpu.py holds the output to the numpy restatement's (tests/tsbk_ref.py).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "../../radiocapture-rf_amd/csrc/tsbk_core.hpp"

using namespace rcfx;

namespace {

struct State { int64_t n_records = 0, n_frames = 0, n_blocks = 0, n_crc_bad = 0, n_lost = 0, next_hit = 0, k_last = kTsbkNoFrame; };
struct Rings {
    std::vector<uint32_t> words, hits;          // the whole streams: ring index i & mask of a ring that has lost nothing yet
    uint32_t word_mask, hit_mask;
    uint32_t word(int64_t i) const { return words.at((size_t)i); }       // (.at: a read outside what the slicer has written aborts)
    uint32_t hit(int64_t i) const { return hits.at((size_t)i); }
};

int ring_dibit(const Rings &R, int64_t p) { return tsbk_word_dibit(R.word(p >> 4), (int)(p & 15)); }

uint64_t ballot(const bool (&b)[64])
{
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)b[l] << l;
    return m;
}

// the inclusive scan of 64 maps under composition, six steps (tsbk_kernel's loop)
void scan64(uint32_t (&map)[64])
{
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t before[64];
        for (int l = 0; l < 64; ++l) before[l] = map[l >= d ? l - d : l];
        for (int l = 0; l < 64; ++l)
            if (l >= d) map[l] = tsbk_compose(before[l], map[l]);
    }
}

// one block of a frame -> its record
void decode_block(const Rings &R, int64_t s, int fd, int b, uint32_t dist, uint32_t nid0, uint32_t nid1, int64_t k0, uint32_t (&rec)[8], bool *crc_bad)
{
    uint32_t c[64] = {0}, map[64];
    for (int l = 0; l < 64; ++l) {
        map[l] = kTsbkIdentity;
        if (l < kTsbkCodeWords) {
            const int j = tsbk_block_dibit(b, tsbk_deinterleave(l));
            c[l] = (uint32_t)(ring_dibit(R, s + tsbk_frame_pos(j)) << 2 | ring_dibit(R, s + tsbk_frame_pos(j + 1)));
            map[l] = tsbk_map(c[l]);
        }
    }
    scan64(map);
    bool inexact[64], hi_b[64], lo_b[64];
    uint32_t crc = 0;
    for (int l = 0; l < 64; ++l) {
        const int state = (int)(map[l] & 3u), prev = l ? (int)(map[l - 1] & 3u) : 0;
        bool exact;
        (void)tsbk_next_state(prev, c[l], &exact);
        inexact[l] = l < kTsbkCodeWords && !exact;
        hi_b[l] = l < 48 && (state & 2);
        lo_b[l] = l < 48 && (state & 1);
        if (l < 48) crc ^= tsbk_crc_term(l, state);
    }
    const uint64_t hi = ballot(hi_b), lo = ballot(lo_b);
    *crc_bad = crc != 0xffffu;
    const int jn = tsbk_frame_pos(tsbk_block_dibit(b, 98));
    const int next_bit = jn < fd ? ring_dibit(R, s + jn) >> 1 : 0;
    rec[0] = tsbk_word0(b, *crc_bad, next_bit, slice_popcount64(ballot(inexact)), dist, nid0);
    rec[1] = (uint32_t)(uint64_t)k0;
    for (int q = 0; q < 3; ++q) rec[2 + q] = slice_word_mem(slice_word_be(hi, lo, 2, q));
    rec[5] = slice_word_mem(nid0); rec[6] = slice_word_mem(nid1); rec[7] = (uint32_t)fd;
}

// one launch (tsbk_kernel, one wave)
void launch(const Rings &R, State &st, int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k, std::vector<uint32_t> &out)
{
    int64_t i = st.next_hit, k_last = st.k_last;
    const int64_t hit_cap = (int64_t)R.hit_mask + 1, word_cap = (int64_t)R.word_mask + 1;
    if (i < n_hits - hit_cap) { st.n_lost += n_hits - hit_cap - i; i = n_hits - hit_cap; }
    const int bound = n_k + kTsbkDecideDibits + 32;
    const int trips = 2 * (bound / kTsbkSyncDibits + 1) + bound / 64 + 2;
    for (int t = 0; t < trips && i < n_hits; ++t) {
        bool valid[64], accb[64];
        uint32_t item[64];
        int64_t k[64];
        for (int l = 0; l < 64; ++l) {
            valid[l] = i + l < n_hits;
            item[l] = valid[l] ? R.hit(i + l) : 0u;
            k[l] = tsbk_widen_k(item[l], n_sym);
            accb[l] = valid[l] && tsbk_accept(k[l], k_last);
        }
        const uint64_t acc = ballot(accb);
        if (!acc) { i += n_hits - i < 64 ? n_hits - i : 64; continue; }
        const int a = __builtin_ctzll(acc);
        if (a > 32) { i += a; continue; }
        const int64_t k0 = k[a], s = k0 - (kTsbkSyncDibits - 1);
        const uint32_t dist = item[a] >> 26;
        i += a;
        if (16 * n_words < s + kTsbkDecideDibits) break;
        bool nb_[64];
        for (int l = 0; l < 64; ++l) nb_[l] = valid[l] && l > a && tsbk_accept(k[l], k0);
        const uint64_t nxt = ballot(nb_);
        int fd = kTsbkFrameDibits;
        if (nxt) {
            const int64_t gap = k[__builtin_ctzll(nxt)] - k0;
            if (gap < fd) fd = (int)gap;
        }
        ++i; k_last = k0; ++st.n_frames;
        if ((s >> 4) < n_words - word_cap) { ++st.n_lost; continue; }
        bool hb[64], lb[64];
        for (int l = 0; l < 64; ++l) {
            const int dn = l < 32 ? ring_dibit(R, s + tsbk_frame_pos(24 + l)) : 0;
            hb[l] = dn & 2; lb[l] = dn & 1;
        }
        const uint64_t nhi = ballot(hb), nlo = ballot(lb);
        const uint32_t nid0 = slice_word_be(nhi, nlo, 2, 0), nid1 = slice_word_be(nhi, nlo, 2, 1);
        const int nb = tsbk_duid(nid0) == 7 ? tsbk_blocks_in(fd) : 0;
        if (nb == 0) {
            const uint32_t rec[8] = {tsbk_word0(3, false, 0, 0, dist, nid0), (uint32_t)(uint64_t)k0, 0, 0, 0, slice_word_mem(nid0), slice_word_mem(nid1), (uint32_t)fd};
            out.insert(out.end(), rec, rec + 8);
            ++st.n_records;
            continue;
        }
        for (int b = 0; b < nb; ++b) {
            uint32_t rec[8];
            bool bad;
            decode_block(R, s, fd, b, dist, nid0, nid1, k0, rec, &bad);
            out.insert(out.end(), rec, rec + 8);
            ++st.n_records; ++st.n_blocks;
            st.n_crc_bad += bad ? 1 : 0;
        }
    }
    st.next_hit = i; st.k_last = k_last;
}

std::vector<uint32_t> read_u32(const char *path)
{
    std::vector<uint32_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint32_t buf[4096];
    for (size_t n; (n = fread(buf, sizeof(uint32_t), 4096, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int mode_stream(int argc, char **argv)
{
    if (argc < 7 || (argc - 7) % 4) return 2;
    Rings R{read_u32(argv[2]), read_u32(argv[3]), (uint32_t)atoll(argv[5]) - 1u, (uint32_t)atoll(argv[6]) - 1u};
    State st;
    st.next_hit = atoll(argv[4]);
    std::vector<uint32_t> out;
    for (int i = 7; i + 3 < argc; i += 4) {
        const int64_t n_words = atoll(argv[i]), n_hits = atoll(argv[i + 1]), n_sym = atoll(argv[i + 2]);
        if (n_words > (int64_t)R.words.size() || n_hits > (int64_t)R.hits.size()) return 2;
        launch(R, st, n_words, n_hits, n_sym, atoi(argv[i + 3]), out);
    }
    printf("records %" PRId64 " frames %" PRId64 " blocks %" PRId64 " crc_bad %" PRId64 " lost %" PRId64 "\n", st.n_records, st.n_frames,
           st.n_blocks, st.n_crc_bad, st.n_lost);
    for (size_t r = 0; r + 8 <= out.size(); r += 8) {
        for (int q = 0; q < 8; ++q) printf("%08x%s", out[r + q], q == 7 ? "\n" : " ");
    }
    return st.n_records * 8 == (int64_t)out.size() ? 0 : 1;
}

int mode_scan(int argc, char **argv)
{
    if (argc < 4) return 2;
    uint64_t x = strtoull(argv[2], nullptr, 10) * 2 + 1;
    const int n = atoi(argv[3]);
    for (int trial = 0; trial < n; ++trial) {
        uint32_t c[64], map[64];
        for (int l = 0; l < 64; ++l) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            c[l] = (uint32_t)(x >> 60);
            map[l] = l < kTsbkCodeWords ? tsbk_map(c[l]) : kTsbkIdentity;
        }
        scan64(map);
        int state = 0;
        for (int l = 0; l < 64; ++l) {
            bool e;
            if (l < kTsbkCodeWords) state = tsbk_next_state(state, c[l], &e);
            if ((int)(map[l] & 3u) != state) { printf("trial %d lane %d: scan %u walk %d\n", trial, l, map[l] & 3u, state); return 1; }
        }
    }
    printf("ok %d\n", n);
    return 0;
}

int mode_pairs()
{
    for (int s = 0; s < 4; ++s)
        for (uint32_t c = 0; c < 16; ++c) {
            bool e;
            const int d = tsbk_next_state(s, c, &e);
            if (((tsbk_map(c) >> (2 * s)) & 3u) != (uint32_t)d) return 1;
            printf("%d %u %d %d\n", s, c, d, (int)e);
        }
    // the CRC terms against the register walked bit by bit, and the index map's range
    for (int p = 0; p < 96; ++p) {
        uint32_t reg = 0;
        for (int q = 0; q < 96; ++q) {
            reg = (reg << 1) | (q == p ? 1u : 0u);
            if (reg & 0x10000u) reg = (reg & 0xffffu) ^ 0x1021u;
        }
        if (reg != kTsbkCrcTerms.t[p]) return 1;
    }
    bool seen[98] = {false};
    for (int t = 0; t < kTsbkCodeWords; ++t) {
        const int at = tsbk_deinterleave(t);
        if (at < 0 || at > 96 || seen[at] || seen[at + 1]) return 1;
        seen[at] = seen[at + 1] = true;
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "stream")) return mode_stream(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "scan")) return mode_scan(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "pairs")) return mode_pairs();
    if (argc >= 4 && !strcmp(argv[1], "widen")) {
        printf("%" PRId64 "\n", tsbk_widen_k((uint32_t)strtoul(argv[2], nullptr, 16), atoll(argv[3])));
        return 0;
    }
    fprintf(stderr, "usage: %s stream|scan|pairs|widen ...\n", argv[0]);
    return 2;
}
