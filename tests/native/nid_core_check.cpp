// nid_core_check.cpp -- radiocapture-rf_amd/csrc/nid_core.hpp compiled for the host: the wave form of the NID's BCH(63,16,23)
// decoder (nid_wave.hpp) walked stand-alone (nid_decode_host.hpp) and the two stages' stream programs with the option in
// them (wave_host.hpp's frame walk; tsbk_decode_host.hpp's and voice_decode_host.hpp's frames).
//   nid_core_check words <words.u64>     per 63-bit word (code bit 0 highest): nid_fix and the word after decoding
//   nid_core_check stream tsbk|voice <words.u32> <hits.u32> <correct> <options> <nid> <first_hit> <word_cap> <hit_cap> <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; prints the stage's five counters and the NID's four, then every record as 8 hex words
// tests/test_nid_cpu.py holds the output to the restatement's (tests/nid_ref.py) and to the reference's answers.
#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "tsbk_decode_host.hpp"
#include "voice_decode_host.hpp"

namespace {

int mode_stream(int argc, char **argv)
{
    if (argc < 11 || (argc - 11) % 4) return 2;
    const bool voice = !strcmp(argv[2], "voice");
    Rings R{read_file<uint32_t>(argv[3]), read_file<uint32_t>(argv[4]), (uint32_t)atoll(argv[9]) - 1u, (uint32_t)atoll(argv[10]) - 1u};
    const bool nid = atoi(argv[7]) != 0;
    const uint32_t flags = (atoi(argv[5]) ? kP25lcFlagCorrect : 0u) | (uint32_t)atoi(argv[6]) << 1 | (nid ? kNidFlagBch : 0u);
    State st;
    NidCount nc;
    TrellisCount tc;
    st.next_hit = atoll(argv[8]);
    std::vector<uint32_t> out;
    if (!(voice ? voice_launches(R, st, flags, nc, argc, argv, 11, out)
                : for_launches(R, argc, argv, 11, [&](int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k) {
                      walk<TsbkWalk>(R, st, n_words, n_hits, n_sym, n_k,
                                     [&](int64_t s, int fd, int64_t k0, uint32_t dist) { tsbk_frame(R, st, nid, false, nc, tc, s, fd, k0, dist, out); });
                  })))
        return 2;
    printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " nid %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", st.n_records, st.n_frames,
           st.n_a, st.n_b, st.n_lost, nc.decoded, nc.fixed, nc.bits, nc.bad);
    print_records(out);
    return st.n_records * 8 == (int64_t)out.size() ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "words")) {
        for (uint64_t w : read_file<uint64_t>(argv[2])) {
            int fix;
            const uint64_t c = nid_decode_wave(w & 0x7fffffffffffffffull, &fix);
            if (nid_encode((uint32_t)(c >> 47)) != c && fix != kNidFixBad) return 1;     // (a decoded word is a code word)
            printf("%d %" PRIu64 "\n", fix, c);
        }
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "stream")) return mode_stream(argc, argv);
    fprintf(stderr, "usage: %s words|stream ...\n", argv[0]);
    return 2;
}
