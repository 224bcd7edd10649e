// tsbk_core_check.cpp -- radiocapture-rf_amd/csrc/tsbk_core.hpp compiled for the host: a stand-alone walk of the P25
// trunking stage over the slicer's two streams, launch by launch as tsbk_kernel (tsbk.hip) walks them: wave_host.hpp's frame
// walk and tsbk_decode_host.hpp's frame, without the stage's options.
//   tsbk_core_check stream <words.u32> <hits.u32> <first_hit> <word_cap> <hit_cap> <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; prints the five counters, then every record as 8 hex words
//   tsbk_core_check scan <seed> <n>       n random blocks of 49 code words: the six-step scan against the 49-step walk
//   tsbk_core_check pairs                 all 64 (state, code word) pairs: next state and whether a candidate is exact
//   tsbk_core_check widen <item hex> <n_symbols>
// tests/test_tsbk_cpu.py holds the output to the numpy restatement's (tests/tsbk_ref.py).
#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "tsbk_decode_host.hpp"

namespace {

int mode_stream(int argc, char **argv)
{
    if (argc < 7 || (argc - 7) % 4) return 2;
    Rings R{read_file<uint32_t>(argv[2]), read_file<uint32_t>(argv[3]), (uint32_t)atoll(argv[5]) - 1u, (uint32_t)atoll(argv[6]) - 1u};
    State st;
    NidCount nc;
    TrellisCount tc;
    st.next_hit = atoll(argv[4]);
    std::vector<uint32_t> out;
    if (!for_launches(R, argc, argv, 7, [&](int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k) {
            walk<TsbkWalk>(R, st, n_words, n_hits, n_sym, n_k,
                           [&](int64_t s, int fd, int64_t k0, uint32_t dist) { tsbk_frame(R, st, false, false, nc, tc, s, fd, k0, dist, out); });
        }))
        return 2;
    printf("records %" PRId64 " frames %" PRId64 " blocks %" PRId64 " crc_bad %" PRId64 " lost %" PRId64 "\n", st.n_records, st.n_frames, st.n_a, st.n_b,
           st.n_lost);
    print_records(out);
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
        printf("%" PRId64 "\n", slice_widen_k((uint32_t)strtoul(argv[2], nullptr, 16), atoll(argv[3])));
        return 0;
    }
    fprintf(stderr, "usage: %s stream|scan|pairs|widen ...\n", argv[0]);
    return 2;
}
