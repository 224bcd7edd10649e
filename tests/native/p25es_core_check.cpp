// p25es_core_check.cpp -- radiocapture-rf_amd/csrc/p25lc_core.hpp compiled for the host, with the options of
// rcf_chan_p25lc_opt: p25lc_core_check.cpp's stand-alone walk of the P25 voice-channel stage -- the 64 lanes of a wave as a
// loop, a ballot as the mask that loop builds, a lane read as an index into the lanes' array -- following p25lc_kernel
// (p25lc.hip) where the options take it: the LDU2 as a unit of kind 4, the (24,12) word's 24th bit, the ballot of the words
// given up as the erased set, and rs_decode<true>: erasure locator, Berlekamp-Massey from round |E|, Chien, Forney and the
// products to degree d - 1.
//   p25es_core_check stream <words.u32> <hits.u32> <correct> <options> <first_hit> <word_cap> <hit_cap> <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; prints the five counters, then every record as 8 hex words
//   p25es_core_check rs <n> <t> <symbols.u8> <0|1>    per word n symbols and n bytes of erased mask: rs_bad, n_rs, the n symbols after
//       decoding -- 1: rs_decode<true> with the mask, 0: rs_decode<false>, the mask ignored
//   p25es_core_check golay <words.u32>            per (24,12) word with its 24th bit taking part: data and status
// tests/test_p25es_cpu.py holds the output to the restatement's (tests/p25es_ref.py) and to the reference's answers.
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

// rs_decode of p25lc.hip, step by step over the 64 lanes; E: the ballot of the erased symbols (kErasures) or 0
template <bool kErasures> void rs_decode(Lanes &sym, uint64_t E, int n, int t, bool *rs_bad, int *n_rs)
{
    constexpr int kDeg = kErasures ? kP25lcMaxD1 : kP25lcMaxT;
    const int ne = kErasures ? slice_popcount64(E) : 0;
    Lanes S, C, B;
    rs_syndrome(sym, n, t, S);
    for (int l = 0; l < 64; ++l) C[l] = l == 0 ? 1u : 0u;
    uint64_t rest = ne <= 2 * t ? E : 0ull;
    for (int r = 0; kErasures && r < kP25lcMaxD1; ++r) {
        Lanes up;
        for (int l = 0; l < 64; ++l) up[l] = C[(l - 1) & 63];
        if (!rest) continue;
        const uint32_t x = p25lc_rs_x(n, __builtin_ctzll(rest));
        for (int l = 0; l < 64; ++l) C[l] ^= p25lc_gf_mul(x, l ? up[l] : 0u);
        rest &= rest - 1;
    }
    memcpy(B, C, sizeof(B));
    uint32_t b = 1;
    int Ln = ne, m = 1;
    for (int r = 0; r < 2 * kP25lcMaxT; ++r) {
        Lanes term, Bs;
        for (int l = 0; l < 64; ++l) {
            term[l] = l <= r ? p25lc_gf_mul(C[l], S[(r - l) & 63]) : 0u;
            Bs[l] = B[(l - m) & 63];
        }
        const uint32_t d = wave_xor(term);
        if (r < ne || r >= 2 * t) continue;
        if (d == 0) { ++m; continue; }
        Lanes Cn;
        for (int l = 0; l < 64; ++l) Cn[l] = C[l] ^ p25lc_gf_mul(p25lc_gf_mul(d, p25lc_gf_inv(b)), l >= m ? Bs[l] : 0u);
        if (2 * Ln <= r + ne) { memcpy(B, C, sizeof(B)); Ln = r + 1 - Ln + ne; b = d; m = 1; } else ++m;
        memcpy(C, Cn, sizeof(C));
    }
    Lanes xi, om, e, fixed, left;
    bool root[64], changed[64], nz[64];
    for (int l = 0; l < 64; ++l) {
        xi[l] = l < n ? p25lc_rs_xinv(n, l) : 0u;
        uint32_t v = 0;
        for (int j = kDeg; j >= 0; --j) v = p25lc_gf_mul(v, xi[l]) ^ C[j];
        root[l] = l < n && v == 0;
        om[l] = 0;
        for (int i = 0; i <= kDeg; ++i)
            if (i <= l) om[l] ^= p25lc_gf_mul(C[i], S[(l - i) & 63]);
        if (kErasures && l >= 2 * t) om[l] = 0;
    }
    const uint64_t roots = ballot(root);
    const bool ok = 2 * Ln - ne <= 2 * t && slice_popcount64(roots) == Ln && (roots & E) == E;
    for (int l = 0; l < 64; ++l) {
        const uint32_t xi2 = p25lc_gf_mul(xi[l], xi[l]);
        uint32_t num = 0, den = 0;
        for (int j = kDeg - 1; j >= 0; --j) num = p25lc_gf_mul(num, xi[l]) ^ om[j];
        for (int j = kDeg - 1; j >= 1; j -= 2) den = p25lc_gf_mul(den, xi2) ^ C[j];
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
void launch(const Rings &R, State &st, uint32_t flags, int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k, std::vector<uint32_t> &out)
{
    const bool correct = flags & kP25lcFlagCorrect, erasures = flags & kP25lcFlagErasures;
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
        const int kind = p25lc_kind(tsbk_duid(nid0), fd, flags), wk = p25lc_words_kind(kind);
        uint32_t rec[8] = {p25lc_word0(kind, false, 0, dist, nid0), (uint32_t)(uint64_t)k0, 0, 0, 0, 0, 0, p25lc_word7(fd, 0, 0)};
        ++st.n_records;
        if (kind == kP25lcFrame) { out.insert(out.end(), rec, rec + 8); continue; }
        Lanes data, two;
        bool fixedb[64], badb[64];
        for (int l = 0; l < 64; ++l) {
            const bool mine = l < p25lc_inner_words(wk);
            const uint32_t word = mine ? p25lc_gather(dibit, wk, l) : 0u;
            int status = 0;
            data[l] = mine ? (correct ? p25lc_inner(kind, word, &status, erasures) : p25lc_systematic(wk, word)) : 0u;
            fixedb[l] = mine && status == 1; badb[l] = mine && status == 2;
        }
        const int n = p25lc_rs_n(wk), kk = p25lc_rs_k_es(kind);
        uint64_t bad = ballot(badb);
        if (kind == kP25lcTlc) {
            memcpy(two, data, sizeof(two));
            bool sb[64];
            for (int l = 0; l < 64; ++l) {
                data[l] = l < n ? (l & 1 ? two[l >> 1] & 63u : two[l >> 1] >> 6) : 0u;
                sb[l] = l < n && (bad >> (l >> 1) & 1);
            }
            bad = ballot(sb);
        }
        bool rs_bad = false;
        int n_rs = 0;
        if (correct && erasures) rs_decode<true>(data, bad, n, p25lc_rs_t_es(kind), &rs_bad, &n_rs);
        else if (correct) rs_decode<false>(data, 0, n, p25lc_rs_t_es(kind), &rs_bad, &n_rs);
        for (int q = 0; q < 4; ++q) {
            uint64_t pay = 0;
            for (int j = 0; j < 7; ++j) {
                const int at = p25lc_pay_first(q) + j;
                pay = pay << 6 | (at < kk ? data[at & 63] : 0u);
            }
            rec[2 + q] = slice_word_mem(p25lc_pay_word(pay, q));
        }
        for (int l = 0; l < 64; ++l) {
            const int dl = p25lc_has_lsd(kind) && l < 16 ? dibit(tsbk_frame_pos(kP25lcLsdDibit + l)) : 0;
            hb[l] = dl & 2; lb[l] = dl & 1;
        }
        rec[0] = p25lc_word0_wide(kind, rs_bad, n_rs, dist, nid0);
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
    if (argc < 9 || (argc - 9) % 4) return 2;
    Rings R{read_file<uint32_t>(argv[2]), read_file<uint32_t>(argv[3]), (uint32_t)atoll(argv[7]) - 1u, (uint32_t)atoll(argv[8]) - 1u};
    const uint32_t flags = (atoi(argv[4]) ? kP25lcFlagCorrect : 0u) | (uint32_t)atoi(argv[5]) << 1;
    State st;
    st.next_hit = atoll(argv[6]);
    std::vector<uint32_t> out;
    for (int i = 9; i + 3 < argc; i += 4) {
        const int64_t n_words = atoll(argv[i]), n_hits = atoll(argv[i + 1]), n_sym = atoll(argv[i + 2]);
        if (n_words > (int64_t)R.words.size() || n_hits > (int64_t)R.hits.size()) return 2;
        launch(R, st, flags, n_words, n_hits, n_sym, atoi(argv[i + 3]), out);
    }
    printf("records %" PRId64 " frames %" PRId64 " decoded %" PRId64 " rs_bad %" PRId64 " lost %" PRId64 "\n", st.n_records, st.n_frames,
           st.n_decoded, st.n_rs_bad, st.n_lost);
    for (size_t r = 0; r + 8 <= out.size(); r += 8)
        for (int q = 0; q < 8; ++q) printf("%08x%s", out[r + q], q == 7 ? "\n" : " ");
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
