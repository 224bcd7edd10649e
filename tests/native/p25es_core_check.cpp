// p25es_core_check.cpp -- radiocapture-rf_amd/csrc/p25lc_core.hpp compiled for the host, with the options of
// rcf_chan_p25lc_opt: p25lc_core_check.cpp's stand-alone walk of the P25 voice-channel stage, following p25lc_kernel
// (p25lc.hip) where the options take it (voice_decode_host.hpp).
//   p25es_core_check stream <words.u32> <hits.u32> <correct> <options> <first_hit> <word_cap> <hit_cap> <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; prints the five counters, then every record as 8 hex words
//   p25es_core_check rs <n> <t> <symbols.u8> <0|1>    per word n symbols and n bytes of erased mask: rs_bad, n_rs, the n symbols after
//       decoding -- 1: rs_decode<true> with the mask, 0: rs_decode<false>, the mask ignored
//   p25es_core_check golay <words.u32>            per (24,12) word with its 24th bit taking part: data and status
// tests/test_p25es_cpu.py holds the output to the restatement's (tests/p25es_ref.py) and to the reference's answers.
#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "voice_decode_host.hpp"

namespace {

int mode_stream(int argc, char **argv)
{
    if (argc < 9 || (argc - 9) % 4) return 2;
    Rings R{read_file<uint32_t>(argv[2]), read_file<uint32_t>(argv[3]), (uint32_t)atoll(argv[7]) - 1u, (uint32_t)atoll(argv[8]) - 1u};
    const uint32_t flags = (atoi(argv[4]) ? kP25lcFlagCorrect : 0u) | (uint32_t)atoi(argv[5]) << 1;
    State st;
    NidCount nc;
    st.next_hit = atoll(argv[6]);
    std::vector<uint32_t> out;
    if (!voice_launches(R, st, flags, nc, argc, argv, 9, out)) return 2;
    printf("records %" PRId64 " frames %" PRId64 " decoded %" PRId64 " rs_bad %" PRId64 " lost %" PRId64 "\n", st.n_records, st.n_frames, st.n_a, st.n_b,
           st.n_lost);
    print_records(out);
    return st.n_records * 8 == (int64_t)out.size() ? 0 : 1;
}

int mode_rs(int argc, char **argv)
{
    if (argc < 6) return 2;
    const int n = atoi(argv[2]), t = atoi(argv[3]);
    const bool erasures = atoi(argv[5]) != 0;
    if (n < 2 * t + 1 || n > kP25lcMaxSyms || t > kP25lcMaxT) return 2;
    const std::vector<uint8_t> all = read_file<uint8_t>(argv[4]);
    for (size_t at = 0; at + 2 * n <= all.size(); at += 2 * n) {
        Lanes sym = {0};
        uint64_t E = 0;
        for (int l = 0; l < n; ++l) {
            sym[l] = all[at + l] & 63u;
            E |= (uint64_t)(all[at + n + l] & 1u) << l;
        }
        bool bad;
        int n_rs;
        if (erasures) rs_decode<true>(sym, E, n, t, &bad, &n_rs); else rs_decode<false>(sym, 0, n, t, &bad, &n_rs);
        printf("%d %d", (int)bad, n_rs);
        for (int l = 0; l < n; ++l) printf(" %u", sym[l]);
        printf("\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "stream")) return mode_stream(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "rs")) return mode_rs(argc, argv);
    if (argc >= 3 && !strcmp(argv[1], "golay")) {
        for (uint32_t w : read_file<uint32_t>(argv[2])) {
            int status;
            const uint32_t d = p25lc_golay24_detect(w, &status);
            printf("%u %d\n", d, status);
        }
        return 0;
    }
    fprintf(stderr, "usage: %s stream|golay|rs ...\n", argv[0]);
    return 2;
}
