// p25lc_core_check.cpp -- radiocapture-rf_amd/csrc/p25lc_core.hpp compiled for the host: a stand-alone walk of the P25
// voice-channel stage over the slicer's two streams, launch by launch as p25lc_kernel (p25lc.hip) walks them -- the 64 lanes
// of a wave as a loop, a ballot as the mask that loop builds, a lane read as an index into the lanes' array -- with every
// index map, inner decoder, field product and record word coming from the header's own functions.
//   p25lc_core_check stream <words.u32> <hits.u32> <correct> <first_hit> <word_cap> <hit_cap> <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; prints the five counters, then every record as 8 hex words
//   p25lc_core_check hamming              all 1024 words: data and status
//   p25lc_core_check golay <24|18> <words.u32>    per word: data and status
//   p25lc_core_check rs <n> <t> <symbols.u8>      per word of n symbols: rs_bad, n_rs, the n symbols after decoding
//   p25lc_core_check field                the tables and the shift / xor product against each other
// tests/test_p25lc_cpu.py holds the output to the numpy restatement's (tests/p25lc_ref.py) and to the reference's answers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "../../radiocapture-rf_amd/csrc/p25lc_core.hpp"

using namespace rcfx;

namespace {

struct State { int64_t n_records = 0, n_frames = 0, n_decoded = 0, n_rs_bad = 0, n_lost = 0, next_hit = 0, k_last = kTsbkNoFrame; };
struct Rings {
    std::vector<uint32_t> words, hits;          // the whole streams: ring index i & mask of a ring that has lost nothing yet
    uint32_t word_mask, hit_mask;
    uint32_t word(int64_t i) const { return words.at((size_t)i); }       // (.at: a read outside what the slicer has written aborts)
    uint32_t hit(int64_t i) const { return hits.at((size_t)i); }
};
typedef uint32_t Lanes[64];

int ring_dibit(const Rings &R, int64_t p) { return tsbk_word_dibit(R.word(p >> 4), (int)(p & 15)); }

uint64_t ballot(const bool (&b)[64])
{
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)b[l] << l;
    return m;
}
uint32_t wave_xor(const Lanes &v)
{
    uint32_t r = 0;
    for (int l = 0; l < 64; ++l) r ^= v[l];
    return r;
}

// rs_syndrome of p25lc.hip: lane m < 2 t runs Horner over the symbols
void rs_syndrome(const Lanes &sym, int n, int t, Lanes &S)
{
    for (int lane = 0; lane < 64; ++lane) {
        const uint32_t am = p25lc_gf_alpha(lane + 1);
        uint32_t s = 0;
        for (int i = 0; i < kP25lcMaxSyms; ++i)
            if (i < n) s = p25lc_gf_mul(s, am) ^ sym[i & 63];
        S[lane] = lane < 2 * t ? s : 0u;
    }
}

// rs_decode of p25lc.hip, step by step over the 64 lanes
void rs_decode(Lanes &sym, int n, int t, bool *rs_bad, int *n_rs)
{
    Lanes S, C, B;
    rs_syndrome(sym, n, t, S);
    for (int l = 0; l < 64; ++l) C[l] = B[l] = l == 0 ? 1u : 0u;
    uint32_t b = 1;
    int Ln = 0, m = 1;
    for (int r = 0; r < 2 * kP25lcMaxT; ++r) {
        Lanes term, Bs;
        for (int l = 0; l < 64; ++l) {
            term[l] = l <= r ? p25lc_gf_mul(C[l], S[(r - l) & 63]) : 0u;
            Bs[l] = B[(l - m) & 63];
        }
        const uint32_t d = wave_xor(term);
        if (r >= 2 * t) continue;
        if (d == 0) { ++m; continue; }
        Lanes Cn;
        for (int l = 0; l < 64; ++l) Cn[l] = C[l] ^ p25lc_gf_mul(p25lc_gf_mul(d, p25lc_gf_inv(b)), l >= m ? Bs[l] : 0u);
        if (2 * Ln <= r) { memcpy(B, C, sizeof(B)); Ln = r + 1 - Ln; b = d; m = 1; } else ++m;
        memcpy(C, Cn, sizeof(C));
    }
    Lanes xi, om, e, fixed, left;
    bool root[64], changed[64], nz[64];
    for (int l = 0; l < 64; ++l) {
        xi[l] = l < n ? p25lc_rs_xinv(n, l) : 0u;
        uint32_t v = 0;
        for (int j = kP25lcMaxT; j >= 0; --j) v = p25lc_gf_mul(v, xi[l]) ^ C[j];
        root[l] = l < n && v == 0;
        om[l] = 0;
        for (int i = 0; i <= kP25lcMaxT; ++i)
            if (i <= l) om[l] ^= p25lc_gf_mul(C[i], S[(l - i) & 63]);
    }
    const bool ok = Ln <= t && slice_popcount64(ballot(root)) == Ln;
    for (int l = 0; l < 64; ++l) {
        const uint32_t xi2 = p25lc_gf_mul(xi[l], xi[l]);
        uint32_t num = 0, den = 0;
        for (int j = kP25lcMaxT - 1; j >= 0; --j) num = p25lc_gf_mul(num, xi[l]) ^ om[j];
        for (int j = kP25lcMaxT - 1; j >= 1; j -= 2) den = p25lc_gf_mul(den, xi2) ^ C[j];
        e[l] = root[l] && den ? p25lc_gf_mul(num, p25lc_gf_inv(den)) : 0u;
        fixed[l] = sym[l] ^ e[l];
        changed[l] = e[l] != 0;
    }
    rs_syndrome(fixed, n, t, left);
    for (int l = 0; l < 64; ++l) nz[l] = left[l] != 0;
    *rs_bad = !ok || ballot(nz) != 0;
    *n_rs = *rs_bad ? 0 : slice_popcount64(ballot(changed));
    if (!*rs_bad) memcpy(sym, fixed, sizeof(fixed));
}

// one launch (p25lc_kernel, one wave)
void launch(const Rings &R, State &st, bool correct, int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k, std::vector<uint32_t> &out)
{
    int64_t i = st.next_hit, k_last = st.k_last;
    const int64_t hit_cap = (int64_t)R.hit_mask + 1, word_cap = (int64_t)R.word_mask + 1;
    if (i < n_hits - hit_cap) { st.n_lost += n_hits - hit_cap - i; i = n_hits - hit_cap; }
    const int bound = n_k + kP25lcDecideDibits + 32;
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
        if (16 * n_words < s + kP25lcDecideDibits) break;
        bool nb_[64];
        for (int l = 0; l < 64; ++l) nb_[l] = valid[l] && l > a && tsbk_accept(k[l], k0);
        const uint64_t nxt = ballot(nb_);
        int fd = kP25lcFrameDibits;
        if (nxt) {
            const int64_t gap = k[__builtin_ctzll(nxt)] - k0;
            if (gap < fd) fd = (int)gap;
        }
        ++i; k_last = k0; ++st.n_frames;
        if ((s >> 4) < n_words - word_cap) { ++st.n_lost; continue; }
        const auto dibit = [&R, s](int r) { return ring_dibit(R, s + r); };
        bool hb[64], lb[64];
        for (int l = 0; l < 64; ++l) {
            const int dn = l < 32 ? dibit(tsbk_frame_pos(24 + l)) : 0;
            hb[l] = dn & 2; lb[l] = dn & 1;
        }
        const uint32_t nid0 = slice_word_be(ballot(hb), ballot(lb), 2, 0);
        const int kind = p25lc_kind(tsbk_duid(nid0), fd);
        uint32_t rec[8] = {p25lc_word0(kind, false, 0, dist, nid0), (uint32_t)(uint64_t)k0, 0, 0, 0, 0, 0, p25lc_word7(fd, 0, 0)};
        ++st.n_records;
        if (kind == kP25lcFrame) { out.insert(out.end(), rec, rec + 8); continue; }
        Lanes data, two;
        bool fixedb[64], badb[64];
        for (int l = 0; l < 64; ++l) {
            const bool mine = l < p25lc_inner_words(kind);
            const uint32_t word = mine ? p25lc_gather(dibit, kind, l) : 0u;
            int status = 0;
            data[l] = mine ? (correct ? p25lc_inner(kind, word, &status) : p25lc_systematic(kind, word)) : 0u;
            fixedb[l] = mine && status == 1; badb[l] = mine && status == 2;
        }
        const int n = p25lc_rs_n(kind), kk = p25lc_rs_k(kind);
        if (kind == kP25lcTlc) {
            memcpy(two, data, sizeof(two));
            for (int l = 0; l < 64; ++l) data[l] = l < n ? (l & 1 ? two[l >> 1] & 63u : two[l >> 1] >> 6) : 0u;
        }
        bool rs_bad = false;
        int n_rs = 0;
        if (correct) rs_decode(data, n, p25lc_rs_t(kind), &rs_bad, &n_rs);
        for (int q = 0; q < 4; ++q) {
            uint64_t pay = 0;
            for (int j = 0; j < 7; ++j) {
                const int at = p25lc_pay_first(q) + j;
                pay = pay << 6 | (at < kk ? data[at & 63] : 0u);
            }
            rec[2 + q] = slice_word_mem(p25lc_pay_word(pay, q));
        }
        for (int l = 0; l < 64; ++l) {
            const int dl = kind == kP25lcLdu1 && l < 16 ? dibit(tsbk_frame_pos(kP25lcLsdDibit + l)) : 0;
            hb[l] = dl & 2; lb[l] = dl & 1;
        }
        rec[0] = p25lc_word0(kind, rs_bad, n_rs, dist, nid0);
        rec[6] = slice_word_mem(slice_word_be(ballot(hb), ballot(lb), 2, 0));
        rec[7] = p25lc_word7(fd, slice_popcount64(ballot(fixedb)), slice_popcount64(ballot(badb)));
        out.insert(out.end(), rec, rec + 8);
        ++st.n_decoded;
        st.n_rs_bad += rs_bad ? 1 : 0;
    }
    st.next_hit = i; st.k_last = k_last;
}

template <class T> std::vector<T> read_file(const char *path)
{
    std::vector<T> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    T buf[4096];
    for (size_t n; (n = fread(buf, sizeof(T), 4096, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int mode_stream(int argc, char **argv)
{
    if (argc < 8 || (argc - 8) % 4) return 2;
    Rings R{read_file<uint32_t>(argv[2]), read_file<uint32_t>(argv[3]), (uint32_t)atoll(argv[6]) - 1u, (uint32_t)atoll(argv[7]) - 1u};
    const bool correct = atoi(argv[4]) != 0;
    State st;
    st.next_hit = atoll(argv[5]);
    std::vector<uint32_t> out;
    for (int i = 8; i + 3 < argc; i += 4) {
        const int64_t n_words = atoll(argv[i]), n_hits = atoll(argv[i + 1]), n_sym = atoll(argv[i + 2]);
        if (n_words > (int64_t)R.words.size() || n_hits > (int64_t)R.hits.size()) return 2;
        launch(R, st, correct, n_words, n_hits, n_sym, atoi(argv[i + 3]), out);
    }
    printf("records %" PRId64 " frames %" PRId64 " decoded %" PRId64 " rs_bad %" PRId64 " lost %" PRId64 "\n", st.n_records, st.n_frames,
           st.n_decoded, st.n_rs_bad, st.n_lost);
    for (size_t r = 0; r + 8 <= out.size(); r += 8)
        for (int q = 0; q < 8; ++q) printf("%08x%s", out[r + q], q == 7 ? "\n" : " ");
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
        rs_decode(sym, n, t, &bad, &n_rs);
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
