// edacs_core_check.cpp -- radiocapture-rf_amd/csrc/edacs_core.hpp compiled for the host: a stand-alone walk of the EDACS
// control-frame stage over the slicer's two streams, launch by launch as edacs_kernel (edacs.hip) walks them -- wave_host.hpp's
// wave and frame walk, an xor-reduction as the xor over the lanes' array -- with every index, syndrome term, class, Chien
// trial, status, election and record word coming from the header's own functions.
//   edacs_core_check stream <words.u32> <hits.u32> <first_hit> <word_cap> <hit_cap> <flags> <base_words> <base_hits>
//                    <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; the files hold the streams from word base_words / hit base_hits on; prints the five
//       counters, then every record as 8 hex words
//   edacs_core_check syn                  all 2^12 syndrome pairs: class, status, positions, flip mask
//   edacs_core_check errors               every single and double error position 0 .. 62 on the zero word
//   edacs_core_check hits                 the slicer's hit rule for every dist 0 .. 48, max_errors 0 .. 47, sync_both 0 / 1 / 2
//   edacs_core_check widen <item hex> <n_symbols>
// tests/test_edacs_cpu.py holds the output to the numpy restatement's (tests/edacs_ref.py).
#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "../../radiocapture-rf_amd/csrc/edacs_core.hpp"
#include "wave_host.hpp"

namespace {

static_assert(State{}.k_last == kEdacsNoFrame, "a fresh stage has accepted no hit");
constexpr uint32_t kFlagBoth = 1u, kFlagEsk = 2u;       // EdacsLaunch::flags (rcf_internal.h)

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

int mode_stream(int argc, char **argv)
{
    if (argc < 10 || (argc - 10) % 4) return 2;
    Rings R{read_file<uint32_t>(argv[2]), read_file<uint32_t>(argv[3]), (uint32_t)atoll(argv[5]) - 1u, (uint32_t)atoll(argv[6]) - 1u, atoll(argv[8]), atoll(argv[9])};
    const uint32_t flags = (uint32_t)atoi(argv[7]);
    State st;                                           // (n_a: msgs, n_b: msgs_none)
    st.next_hit = atoll(argv[4]);
    std::vector<uint32_t> out;
    if (!for_launches(R, argc, argv, 10, [&](int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k) {
            walk<EdacsWalk>(R, st, n_words, n_hits, n_sym, n_k, [&](int64_t s, int, int64_t k0, uint32_t raw) {
                uint32_t rec[8];
                bool has1, has2;
                decode_frame(R, s, k0, raw, flags, rec, &has1, &has2);
                out.insert(out.end(), rec, rec + 8);
                ++st.n_records;
                st.n_a += (has1 ? 1 : 0) + (has2 ? 1 : 0);
                st.n_b += (has1 ? 0 : 1) + (has2 ? 0 : 1);
            });
        }))
        return 2;
    printf("records %" PRId64 " frames %" PRId64 " msgs %" PRId64 " msgs_none %" PRId64 " lost %" PRId64 "\n", st.n_records, st.n_frames, st.n_a, st.n_b,
           st.n_lost);
    print_records(out);
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
        printf("%" PRId64 "\n", slice_widen_k((uint32_t)strtoul(argv[2], nullptr, 16), atoll(argv[3])));
        return 0;
    }
    fprintf(stderr, "usage: edacs_core_check stream|syn|errors|hits|widen ...\n");
    return 2;
}
