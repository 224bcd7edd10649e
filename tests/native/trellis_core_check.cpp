// trellis_core_check.cpp -- the trellis option of the P25 trunking stage (RCF_TRELLIS_VITERBI; radiocapture-rf_amd/csrc/
// tsbk_core.hpp) compiled for the host: the wave form of tsbk.hip walked stand-alone (tsbk_decode_host.hpp) -- with the
// min-plus matrices, their composition, the forward map, the branch distance and the record bits coming from the header's
// own functions -- held to a sequential form written out here (backward costs, forward walk).  The frame walk is
// wave_host.hpp's.
//   trellis_core_check assoc <seed> <n>          n random triples of matrices: (A x B) x C == A x (B x C)
//   trellis_core_check blocks <n_words> <c.u8>   rows of n_words + 1 code words (a byte each; n_words 48 is a TSBK block,
//                                               the last word the flushing one): per row the wave form's states as digits,
//                                               cost, n_inexact; exit 1 where the sequential form differs
//   trellis_core_check random <seed> <n>         n random blocks of 49 code words, half of them valid blocks with few flips:
//                                               wave form against sequential form
//   trellis_core_check stream <words.u32> <hits.u32> <nid> <trellis> <first_hit> <word_cap> <hit_cap> <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; prints the stage's five counters, the NID's four and the trellis decoder's four, then
//       every record as 8 hex words
// tests/test_trellis_cpu.py holds the output to the restatement's (tests/trellis_ref.py).
#include <algorithm>

#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "tsbk_decode_host.hpp"

namespace {

// the rule's sequential form, with nothing of the header but the table
Decoded sequential_form(const uint32_t (&c)[64], int last)
{
    const auto dist = [](int s, int d, uint32_t w) { return __builtin_popcount(((tsbk_trellis_row(s) >> (4 * d)) & 15u) ^ (w & 15u)); };
    int beta[65][4] = {{0}};
    for (int s = 0; s < 4; ++s) beta[last][s] = dist(s, 0, c[last]);
    for (int t = last - 1; t >= 0; --t)
        for (int s = 0; s < 4; ++s) {
            int least = 1 << 20;
            for (int d = 0; d < 4; ++d) least = std::min(least, dist(s, d, c[t]) + beta[t + 1][d]);
            beta[t][s] = least;
        }
    Decoded r{};
    int s = 0;
    for (int t = 0; t <= last; ++t) {
        int best = 0, least = 1 << 20;
        for (int d = 0; d < (t < last ? 4 : 1); ++d) {
            const int sum = dist(s, d, c[t]) + (t < last ? beta[t + 1][d] : 0);
            if (sum < least) { least = sum; best = d; }
        }
        const int away = dist(s, best, c[t]);
        r.cost += away; r.n_inexact += away != 0;
        r.state[t] = best;
        s = best;
    }
    return r;
}

bool same(const Decoded &a, const Decoded &b, int last)
{
    for (int t = 0; t <= last; ++t)
        if (a.state[t] != b.state[t]) return false;
    return a.cost == b.cost && a.n_inexact == b.n_inexact;
}

uint64_t lcg(uint64_t &x) { x = x * 6364136223846793005ull + 1442695040888963407ull; return x >> 33; }

int mode_assoc(int argc, char **argv)
{
    if (argc < 4) return 2;
    uint64_t x = strtoull(argv[2], nullptr, 10) * 2 + 1;
    const int n = atoi(argv[3]);
    for (int trial = 0; trial < n; ++trial) {
        TsbkMat m[3];
        for (int i = 0; i < 3; ++i) {
            const uint64_t v = lcg(x);
            m[i] = v % 11 == 0 ? tsbk_mat_identity() : tsbk_mat((uint32_t)(v >> 4) & 15u, v % 7 == 0);
            for (uint64_t k = lcg(x) % 20; k; --k) m[i] = tsbk_mat_compose(m[i], tsbk_mat((uint32_t)lcg(x) & 15u, false));   // products of up to 20 words as well
        }
        const TsbkMat left = tsbk_mat_compose(tsbk_mat_compose(m[0], m[1]), m[2]), right = tsbk_mat_compose(m[0], tsbk_mat_compose(m[1], m[2]));
        const TsbkMat id = tsbk_mat_identity(), li = tsbk_mat_compose(id, m[0]), ri = tsbk_mat_compose(m[0], id);
        for (int s = 0; s < 4; ++s)
            if (left.row[s] != right.row[s] || li.row[s] != m[0].row[s] || ri.row[s] != m[0].row[s]) { printf("trial %d row %d\n", trial, s); return 1; }
    }
    printf("ok %d\n", n);
    return 0;
}

int mode_blocks(int argc, char **argv)
{
    if (argc < 4) return 2;
    const int last = atoi(argv[2]);
    if (last < 1 || last > 62) return 2;
    const std::vector<uint8_t> all = read_file<uint8_t>(argv[3]);
    for (size_t at = 0; at + (size_t)last + 1 <= all.size(); at += (size_t)last + 1) {
        uint32_t c[64] = {0};
        for (int l = 0; l <= last; ++l) c[l] = all[at + (size_t)l] & 15u;
        const Decoded w = wave_form(c, last, true), q = sequential_form(c, last);
        if (!same(w, q, last)) { printf("row %zu: the wave form is not the sequential form\n", at / ((size_t)last + 1)); return 1; }
        for (int l = 0; l <= last; ++l) putchar('0' + w.state[l]);
        printf(" %d %d\n", w.cost, w.n_inexact);
    }
    return 0;
}

int mode_random(int argc, char **argv)
{
    if (argc < 4) return 2;
    uint64_t x = strtoull(argv[2], nullptr, 10) * 2 + 1;
    const int n = atoi(argv[3]);
    int64_t cost = 0;
    for (int trial = 0; trial < n; ++trial) {
        uint32_t c[64] = {0};
        if (trial & 1) {                             // a valid block with 0 .. 8 wrong bits
            int s = 0;
            for (int t = 0; t < kTsbkCodeWords; ++t) {
                const int d = t < 48 ? (int)(lcg(x) & 3u) : 0;
                c[t] = (tsbk_trellis_row(s) >> (4 * d)) & 15u;
                s = d;
            }
            for (uint64_t k = lcg(x) % 9; k; --k) c[lcg(x) % kTsbkCodeWords] ^= 1u << (lcg(x) & 3u);
        } else {
            for (int t = 0; t < kTsbkCodeWords; ++t) c[t] = (uint32_t)lcg(x) & 15u;
        }
        const Decoded w = wave_form(c, kTsbkCodeWords - 1, true), q = sequential_form(c, kTsbkCodeWords - 1);
        if (!same(w, q, kTsbkCodeWords - 1)) { printf("trial %d: the wave form is not the sequential form\n", trial); return 1; }
        if (w.state[kTsbkCodeWords - 1] != 0) return 1;
        cost += w.cost;
    }
    printf("ok %d cost %" PRId64 "\n", n, cost);
    return 0;
}

int mode_stream(int argc, char **argv)
{
    if (argc < 9 || (argc - 9) % 4) return 2;
    Rings R{read_file<uint32_t>(argv[2]), read_file<uint32_t>(argv[3]), (uint32_t)atoll(argv[7]) - 1u, (uint32_t)atoll(argv[8]) - 1u};
    const bool nid = atoi(argv[4]) != 0, viterbi = atoi(argv[5]) != 0;
    State st;
    NidCount nc;
    TrellisCount tc;
    st.next_hit = atoll(argv[6]);
    std::vector<uint32_t> out;
    if (!for_launches(R, argc, argv, 9, [&](int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k) {
            walk<TsbkWalk>(R, st, n_words, n_hits, n_sym, n_k,
                           [&](int64_t s, int fd, int64_t k0, uint32_t dist) { tsbk_frame(R, st, nid, viterbi, nc, tc, s, fd, k0, dist, out); });
        }))
        return 2;
    printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " nid %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " trellis %" PRId64 " %" PRId64
           " %" PRId64 " %" PRId64 "\n", st.n_records, st.n_frames, st.n_a, st.n_b, st.n_lost, nc.decoded, nc.fixed, nc.bits, nc.bad, tc.decoded, tc.clean, tc.bits, tc.words);
    print_records(out);
    return st.n_records * 8 == (int64_t)out.size() ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "assoc")) return mode_assoc(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "blocks")) return mode_blocks(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "random")) return mode_random(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "stream")) return mode_stream(argc, argv);
    fprintf(stderr, "usage: %s assoc|blocks|random|stream ...\n", argv[0]);
    return 2;
}
