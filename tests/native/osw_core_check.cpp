// osw_core_check.cpp -- radiocapture-rf_amd/csrc/osw_core.hpp compiled for the host: a stand-alone walk of the SmartNet OSW
// stage over the slicer's two streams, launch by launch as osw_kernel (osw.hip) walks them -- the 64 lanes of a wave as a
// loop, a ballot as the mask that loop builds -- with every hit start, framing decision, lock step, packet index, mask and
// record word coming from the header's own functions.
//   osw_core_check stream <words.u32> <hits.u32> <first_hit> <pos0> <word_cap> <hit_cap> <base_words> <base_hits>
//                  <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; the files hold the streams from word base_words / hit base_hits on; prints the counters,
//       then every record as 8 hex words.  A read of a ring item that the ring no longer (or not yet) holds aborts.
//   osw_core_check masks <n_random>       psyn patterns -- all single bits, all pairs, n_random random ones -- with their flip mask
//   osw_core_check start <item hex> <n_symbols>
// tests/test_osw_cpu.py holds the output to the numpy restatement's (tests/osw_ref.py).
#define RCF_DEVFN static inline
#include "../../radiocapture-rf_amd/csrc/osw_core.hpp"
#include "wave_host.hpp"

namespace {

struct OswState {
    int64_t n_records = 0, n_frames = 0, n_bad = 0, n_rejects = 0, n_lost = 0;
    int32_t locked = 0, is_locked = 0;
    int64_t next_hit = 0, pos = 0;
};
struct OswRings : Rings {                       // ... with a launch's bounds: a read of an item the ring does not hold aborts
    int64_t n_words = 0, n_hits = 0;            // of the launch under way
    uint32_t word(int64_t i) const
    {
        if (i >= n_words || i < n_words - ((int64_t)word_mask + 1)) { fprintf(stderr, "word %" PRId64 " is not in the ring\n", i); abort(); }
        return Rings::word(i);
    }
    uint32_t hit(int64_t i) const
    {
        if (i >= n_hits || i < n_hits - ((int64_t)hit_mask + 1)) { fprintf(stderr, "hit %" PRId64 " is not in the ring\n", i); abort(); }
        return Rings::hit(i);
    }
};

// one launch (osw_kernel, one wave)
void launch(OswRings &R, OswState &st, int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k, std::vector<uint32_t> &out)
{
    R.n_words = n_words; R.n_hits = n_hits;
    const int64_t W = 32 * n_words;
    int64_t i = st.next_hit, pos = st.pos;
    int32_t locked = st.locked, is_locked = st.is_locked;
    const int64_t hit_cap = (int64_t)R.hit_mask + 1, word_cap = (int64_t)R.word_mask + 1;
    bool resync = false;
    if (i < n_hits - hit_cap) { st.n_lost += n_hits - hit_cap - i; i = n_hits - hit_cap; resync = true; }
    const int trips = osw_trips(n_k);
    int t = 0;
    for (; t < trips; ++t) {
        bool valid[64], geb[64];
        int64_t h[64];
        for (int l = 0; l < 64; ++l) {
            valid[l] = i + l < n_hits;
            h[l] = osw_hit_start(valid[l] ? R.hit(i + l) : 0u, n_sym);
            geb[l] = valid[l] && h[l] >= pos;
        }
        const uint64_t ge = ballot(geb);
        const bool have0 = ge != 0;
        int64_t h0 = 0;
        if (!have0) {
            const int64_t adv = n_hits - i < 64 ? (n_hits - i > 0 ? n_hits - i : 0) : 64;
            i += adv;
            if (adv == 64) continue;
        } else {
            const int a = __builtin_ctzll(ge);
            i += a;
            if (a > 64 - kOswSyncBits - 1) continue;
            h0 = h[a];
        }
        if (resync) { resync = false; if (have0) pos = h0; }
        if (!osw_ready(locked, have0, h0, pos, W)) break;
        bool ge1b[64];
        for (int l = 0; l < 64; ++l) ge1b[l] = have0 && valid[l] && h[l] >= h0 + kOswSyncBits;
        const uint64_t ge1 = ballot(ge1b);
        const bool have1 = ge1 != 0;
        const int64_t h1 = have1 ? h[__builtin_ctzll(ge1)] : 0;
        bool rel_nz;
        uint32_t rel;
        if (osw_decide(locked, have0, h0, have1, h1, pos, &rel_nz, &rel) == kOswReject) { pos = h0 + kOswSyncBits; ++st.n_rejects; continue; }
        const int32_t l1 = osw_lock_step(locked, rel_nz);
        const int64_t s = osw_sync_pos(l1, pos, h0);
        if ((s >> 5) < n_words - word_cap) { ++st.n_lost; pos = 32 * (n_words - word_cap); resync = true; continue; }
        locked = l1; is_locked = osw_is_locked(l1) ? 1 : 0; ++st.n_frames;
        bool db[64], pb[64];
        for (int l = 0; l < 64; ++l) {
            db[l] = pb[l] = false;
            if (l < kOswDataBits) {
                const int64_t pd = s + kOswSyncBits + osw_data_bit(l), pp = s + kOswSyncBits + osw_parity_bit(l);
                db[l] = osw_word_bit(R.word(pd >> 5), (int)(pd & 31)) != 0;
                pb[l] = osw_word_bit(R.word(pp >> 5), (int)(pp & 31)) != 0;
            }
        }
        uint64_t data = ballot(db);
        const uint64_t psyn = osw_psyn(data, ballot(pb)), flips = psyn ? osw_flip_mask(psyn) : 0;
        data ^= flips;
        if (psyn) ++st.n_bad;
        locked = osw_lock_clean(locked, rel_nz, psyn);
        const uint32_t word0 = osw_word0(rel_nz, psyn, is_locked != 0, data, flips, rel);
        for (int l = 0; l < kOswRecWords; ++l) out.push_back(osw_rec_word(l, word0, s, data, psyn, locked));
        ++st.n_records;
        pos = s + kOswFrameBits;
    }
    if (t >= trips) { fprintf(stderr, "the launch used up its %d trips (n_k %d)\n", trips, n_k); abort(); }   // the bound must leave the break
    st.locked = locked; st.is_locked = is_locked; st.next_hit = i; st.pos = pos;
}

int mode_stream(int argc, char **argv)
{
    if (argc < 10 || (argc - 10) % 4) return 2;
    OswRings R{{read_file<uint32_t>(argv[2]), read_file<uint32_t>(argv[3]), (uint32_t)atoll(argv[6]) - 1u, (uint32_t)atoll(argv[7]) - 1u, atoll(argv[8]), atoll(argv[9])}};
    OswState st;
    st.next_hit = atoll(argv[4]);
    st.pos = atoll(argv[5]);
    std::vector<uint32_t> out;
    if (!for_launches(R, argc, argv, 10, [&](int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k) { launch(R, st, n_words, n_hits, n_sym, n_k, out); })) return 2;
    printf("records %" PRId64 " frames %" PRId64 " bad %" PRId64 " rejects %" PRId64 " lost %" PRId64 " locked %d is_locked %d\n", st.n_records,
           st.n_frames, st.n_bad, st.n_rejects, st.n_lost, st.locked, st.is_locked);
    print_records(out);
    return 0;
}

int mode_masks(int n_random)
{
    const uint64_t all = ((uint64_t)1 << kOswDataBits) - 1;
    for (int a = 0; a < kOswDataBits; ++a)
        for (int b = a; b < kOswDataBits; ++b) {
            const uint64_t p = ((uint64_t)1 << a) | ((uint64_t)1 << b);
            printf("%" PRIx64 " %" PRIx64 "\n", p, osw_flip_mask(p));
        }
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (int n = 0; n < n_random; ++n) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint64_t p = x & all;
        printf("%" PRIx64 " %" PRIx64 "\n", p, osw_flip_mask(p));
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "stream")) return mode_stream(argc, argv);
    if (argc == 3 && !strcmp(argv[1], "masks")) return mode_masks(atoi(argv[2]));
    if (argc == 4 && !strcmp(argv[1], "start")) {
        printf("%" PRId64 "\n", osw_hit_start((uint32_t)strtoul(argv[2], nullptr, 16), atoll(argv[3])));
        return 0;
    }
    fprintf(stderr, "usage: osw_core_check stream|masks|start ...\n");
    return 2;
}
