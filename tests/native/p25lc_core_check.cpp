// p25lc_core_check.cpp -- radiocapture-rf_amd/csrc/p25lc_core.hpp compiled for the host: a stand-alone walk of the P25
// voice-channel stage over the slicer's two streams, launch by launch as p25lc_kernel (p25lc.hip) walks them: wave_host.hpp's
// frame walk and voice_decode_host.hpp's frame, without the stage's options.
//   p25lc_core_check stream <words.u32> <hits.u32> <correct> <first_hit> <word_cap> <hit_cap> <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; prints the five counters, then every record as 8 hex words
//   p25lc_core_check hamming              all 1024 words: data and status
//   p25lc_core_check golay <24|18> <words.u32>    per word: data and status
//   p25lc_core_check rs <n> <t> <symbols.u8>      per word of n symbols: rs_bad, n_rs, the n symbols after decoding
//   p25lc_core_check field                the tables and the shift / xor product against each other
// tests/test_p25lc_cpu.py holds the output to the numpy restatement's (tests/p25lc_ref.py) and to the reference's answers.
#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "voice_decode_host.hpp"

namespace {

int mode_stream(int argc, char **argv)
{
    if (argc < 8 || (argc - 8) % 4) return 2;
    Rings R{read_file<uint32_t>(argv[2]), read_file<uint32_t>(argv[3]), (uint32_t)atoll(argv[6]) - 1u, (uint32_t)atoll(argv[7]) - 1u};
    State st;
    NidCount nc;
    st.next_hit = atoll(argv[5]);
    std::vector<uint32_t> out;
    if (!voice_launches(R, st, atoi(argv[4]) ? kP25lcFlagCorrect : 0u, nc, argc, argv, 8, out)) return 2;
    printf("records %" PRId64 " frames %" PRId64 " decoded %" PRId64 " rs_bad %" PRId64 " lost %" PRId64 "\n", st.n_records, st.n_frames, st.n_a, st.n_b,
           st.n_lost);
    print_records(out);
    return st.n_records * 8 == (int64_t)out.size() ? 0 : 1;
}

int mode_rs(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int n = atoi(argv[2]), t = atoi(argv[3]);
    if (n < 2 * t + 1 || n > kP25lcMaxSyms || t > kP25lcMaxT) return 2;
    const std::vector<uint8_t> all = read_file<uint8_t>(argv[4]);
    for (size_t at = 0; at + n <= all.size(); at += n) {
        Lanes sym = {0};
        for (int l = 0; l < n; ++l) sym[l] = all[at + l] & 63u;
        bool bad;
        int n_rs;
        rs_decode<false>(sym, 0, n, t, &bad, &n_rs);
        printf("%d %d", (int)bad, n_rs);
        for (int l = 0; l < n; ++l) printf(" %u", sym[l]);
        printf("\n");
    }
    return 0;
}

int mode_field()
{
    for (uint32_t a = 0; a < 64; ++a)
        for (uint32_t b = 0; b < 64; ++b) {
            const uint32_t want = a && b ? kP25lcGf.exp[(kP25lcGf.log[a] + kP25lcGf.log[b]) % 63] : 0u;
            if (p25lc_gf_mul(a, b) != want) return 1;
        }
    for (uint32_t a = 1; a < 64; ++a)
        if (p25lc_gf_mul(a, p25lc_gf_inv(a)) != 1u) return 1;
    int filled = 0;
    for (int s = 0; s < 2048; ++s) {
        const uint32_t e = kP25lcGolay.e[s];
        if (p25lc_golay_syndrome(e) != (uint32_t)s || slice_popcount64(e) > 3) return 1;
        filled += e != 0;
    }
    printf("ok %d\n", filled);
    return filled == 2047 ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "stream")) return mode_stream(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "rs")) return mode_rs(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "field")) return mode_field();
    if (argc >= 2 && !strcmp(argv[1], "hamming")) {
        for (uint32_t w = 0; w < 1024; ++w) {
            int status;
            const uint32_t d = p25lc_hamming(w, &status);
            printf("%u %d\n", d, status);
        }
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "golay")) {
        const bool shortened = atoi(argv[2]) == 18;
        for (uint32_t w : read_file<uint32_t>(argv[3])) {
            int status;
            const uint32_t d = shortened ? p25lc_golay18(w, &status) : p25lc_golay24(w, &status);
            printf("%u %d\n", d, status);
        }
        return 0;
    }
    fprintf(stderr, "usage: %s stream|hamming|golay|rs|field ...\n", argv[0]);
    return 2;
}
