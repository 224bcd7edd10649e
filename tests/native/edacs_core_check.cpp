// edacs_core_check.cpp -- radiocapture-rf_amd/csrc/edacs_core.hpp compiled for the host: a stand-alone walk of the EDACS
// control-frame stage over the slicer's two streams, launch by launch as edacs_kernel (edacs.hip) walks them -- the 64 lanes
// of a wave as a loop, a ballot as the mask that loop builds, an xor-reduction as the xor over the lanes' array -- with every
// index, syndrome term, class, Chien trial, status, election and record word coming from the header's own functions.
//   edacs_core_check stream <words.u32> <hits.u32> <first_hit> <word_cap> <hit_cap> <flags> <base_words> <base_hits>
//                    <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; the files hold the streams from word base_words / hit base_hits on; prints the five
//       counters, then every record as 8 hex words
//   edacs_core_check syn                  all 2^12 syndrome pairs: class, status, positions, flip mask
//   edacs_core_check errors               every single and double error position 0 .. 62 on the zero word
//   edacs_core_check hits                 the slicer's hit rule for every dist 0 .. 48, max_errors 0 .. 47, sync_both 0 / 1 / 2
//   edacs_core_check widen <item hex> <n_symbols>
// tests/test_edacs_cpu.py holds the output to the numpy restatement's (tests/edacs_ref.py).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "../../radiocapture-rf_amd/csrc/edacs_core.hpp"

using namespace rcfx;

namespace {

constexpr uint32_t kFlagBoth = 1u, kFlagEsk = 2u;       // EdacsLaunch::flags (rcf_internal.h)

struct State { int64_t n_records = 0, n_frames = 0, n_msgs = 0, n_msgs_none = 0, n_lost = 0, next_hit = 0, k_last = kEdacsNoFrame; };
struct Rings {
    std::vector<uint32_t> words, hits;          // the streams from base_words / base_hits on
    uint32_t word_mask, hit_mask;
    int64_t base_words, base_hits;
    uint32_t word(int64_t i) const { return words.at((size_t)(i - base_words)); }    // (.at: a read outside what the slicer has written aborts)
    uint32_t hit(int64_t i) const { return hits.at((size_t)(i - base_hits)); }
};

uint64_t ballot(const bool (&b)[64])
{
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)b[l] << l;
    return m;
}

// a syndrome pair -> class, positions (the Chien trials as the lanes run them), status, flip
int solve(uint32_t syn, uint64_t *pos, uint64_t *flip, int *cls_out)
{
    int p, e1, e2;
    const int cls = edacs_classify(syn, &p, &e1, &e2);
    *pos = 0;
    if (cls == 1) *pos = (uint64_t)1 << p;
    else if (cls == 2) {
        bool root[64];
        for (int l = 0; l < 64; ++l) root[l] = l < 63 && edacs_chien_trial(e1, e2, l ? l : 63);
        *pos = ballot(root);
    }
    if (cls_out) *cls_out = cls;
    return edacs_copy_status(cls, *pos, flip);
}

// one frame -> its record
void decode_frame(const Rings &R, int64_t s, int64_t k0, uint32_t raw, uint32_t flags, uint32_t (&rec)[8], bool *has1, bool *has2)
{
    const bool inverted = edacs_inverted(raw, flags & kFlagBoth);
    uint64_t val[kEdacsCopies];
    uint32_t syn[kEdacsCopies / 2] = {0, 0, 0};
    for (int c = 0; c < kEdacsCopies; ++c) {
        bool bits[64];
        for (int l = 0; l < 64; ++l) {
            int bit = 0;
            if (l < kEdacsCopyBits) {
                const int64_t p = s + edacs_coef_bit(c, l);
                bit = edacs_word_bit(R.word(p >> 5), (int)(p & 31)) ^ (inverted != edacs_copy_inverted(c) ? 1 : 0);
            }
            bits[l] = bit != 0;
            if (bit) syn[c >> 1] ^= (l < kEdacsCopyBits ? edacs_syn_term(l) : 0u) << (12 * (c & 1));
        }
        val[c] = ballot(bits);
    }
    int status[kEdacsCopies];
    uint32_t statuses = 0;
    for (int c = 0; c < kEdacsCopies; ++c) {
        uint64_t pos, flip;
        status[c] = solve((syn[c >> 1] >> (12 * (c & 1))) & 0xfffu, &pos, &flip, nullptr);
        val[c] ^= flip;
        statuses |= (uint32_t)status[c] << (2 * c);
    }
    uint64_t m1, m2;
    *has1 = edacs_elect(status[0], status[1], status[2], val[0], val[1], val[2], &m1);
    *has2 = edacs_elect(status[3], status[4], status[5], val[3], val[4], val[5], &m2);
    if (*has1) m1 = edacs_esk(m1, flags & kFlagEsk);
    if (*has2) m2 = edacs_esk(m2, flags & kFlagEsk);
    rec[0] = edacs_word0(inverted, *has1, *has2, edacs_hit_dist(raw, inverted), statuses);
    rec[1] = (uint32_t)(uint64_t)k0;
    rec[2] = edacs_msg_word(m1, 0); rec[3] = edacs_msg_word(m1, 1);
    rec[4] = edacs_msg_word(m2, 0); rec[5] = edacs_msg_word(m2, 1);
    rec[6] = rec[7] = 0;
}

// one launch (edacs_kernel, one wave)
void launch(const Rings &R, State &st, uint32_t flags, int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k, std::vector<uint32_t> &out)
{
    int64_t i = st.next_hit, k_last = st.k_last;
    const int64_t hit_cap = (int64_t)R.hit_mask + 1, word_cap = (int64_t)R.word_mask + 1;
    if (i < n_hits - hit_cap) { st.n_lost += n_hits - hit_cap - i; i = n_hits - hit_cap; }
    const int bound = n_k + kEdacsFrameBits + 32;
    const int trips = bound / kEdacsFrameBits + 1 + bound / 64 + 2;
    for (int t = 0; t < trips && i < n_hits; ++t) {
        bool valid[64], accb[64];
        uint32_t item[64];
        int64_t k[64];
        for (int l = 0; l < 64; ++l) {
            valid[l] = i + l < n_hits;
            item[l] = valid[l] ? R.hit(i + l) : 0u;
            k[l] = edacs_widen_k(item[l], n_sym);
            accb[l] = valid[l] && edacs_accept(k[l], k_last);
        }
        const uint64_t acc = ballot(accb);
        if (!acc) { i += n_hits - i < 64 ? n_hits - i : 64; continue; }
        const int a = __builtin_ctzll(acc);
        const int64_t k0 = k[a], s = k0 - (kEdacsSyncBits - 1);
        const uint32_t raw = item[a] >> 26;
        i += a;
        if (32 * n_words < s + kEdacsFrameBits) break;
        ++i; k_last = k0; ++st.n_frames;
        if ((s >> 5) < n_words - word_cap) { ++st.n_lost; continue; }
        uint32_t rec[8];
        bool has1, has2;
        decode_frame(R, s, k0, raw, flags, rec, &has1, &has2);
        out.insert(out.end(), rec, rec + 8);
        ++st.n_records;
        st.n_msgs += (has1 ? 1 : 0) + (has2 ? 1 : 0);
        st.n_msgs_none += (has1 ? 0 : 1) + (has2 ? 0 : 1);
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
    if (argc < 10 || (argc - 10) % 4) return 2;
    Rings R{read_u32(argv[2]), read_u32(argv[3]), (uint32_t)atoll(argv[5]) - 1u, (uint32_t)atoll(argv[6]) - 1u, atoll(argv[8]), atoll(argv[9])};
    const uint32_t flags = (uint32_t)atoi(argv[7]);
    State st;
    st.next_hit = atoll(argv[4]);
    std::vector<uint32_t> out;
    for (int i = 10; i + 3 < argc; i += 4) {
        const int64_t n_words = atoll(argv[i]), n_hits = atoll(argv[i + 1]), n_sym = atoll(argv[i + 2]);
        if (n_words - R.base_words > (int64_t)R.words.size() || n_hits - R.base_hits > (int64_t)R.hits.size()) return 2;
        launch(R, st, flags, n_words, n_hits, n_sym, atoi(argv[i + 3]), out);
    }
    printf("records %" PRId64 " frames %" PRId64 " msgs %" PRId64 " msgs_none %" PRId64 " lost %" PRId64 "\n", st.n_records, st.n_frames,
           st.n_msgs, st.n_msgs_none, st.n_lost);
    for (size_t r = 0; r + 8 <= out.size(); r += 8)
        for (int q = 0; q < 8; ++q) printf("%08x%s", out[r + q], q == 7 ? "\n" : " ");
    return 0;
}

int mode_syn()
{
    for (uint32_t syn = 0; syn < 4096; ++syn) {
        uint64_t pos, flip;
        int cls;
        const int status = solve(syn, &pos, &flip, &cls);
        printf("%u %u %d %d %" PRIx64 " %" PRIx64 "\n", syn & 63u, syn >> 6, cls, status, pos, flip);
    }
    return 0;
}

int mode_errors()
{
    for (int p = 0; p < 63; ++p)
        for (int q = p; q < 63; ++q) {
            const uint32_t syn = edacs_syn_term(p) ^ (q != p ? edacs_syn_term(q) : 0u);
            uint64_t pos, flip;
            const int status = solve(syn, &pos, &flip, nullptr);
            printf("%d %d %d %" PRIx64 " %" PRIx64 "\n", p, q, status, pos, flip);
        }
    return 0;
}

int mode_hits()
{
    for (int both = 0; both < 3; ++both)
        for (int me = 0; me < 48; ++me) {
            printf("%d %d %d", both, me, (int)slice_sync_both_ok(48, me, both));
            for (int dist = 0; dist <= 48; ++dist) printf(" %d", (int)slice_is_hit(dist, 48, me, both));
            printf("\n");
        }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "stream")) return mode_stream(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "syn")) return mode_syn();
    if (argc >= 2 && !strcmp(argv[1], "errors")) return mode_errors();
    if (argc >= 2 && !strcmp(argv[1], "hits")) return mode_hits();
    if (argc == 4 && !strcmp(argv[1], "widen")) {
        printf("%" PRId64 "\n", edacs_widen_k((uint32_t)strtoul(argv[2], nullptr, 16), atoll(argv[3])));
        return 0;
    }
    fprintf(stderr, "usage: edacs_core_check stream|syn|errors|hits|widen ...\n");
    return 2;
}
