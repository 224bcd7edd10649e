// nid_core_check.cpp -- radiocapture-rf_amd/csrc/nid_core.hpp compiled for the host: the wave form of the NID's BCH(63,16,23)
// decoder (nid_wave.hpp) walked stand-alone -- the 64 lanes of a wave as a loop, a ballot as the mask that loop builds, a lane
// read as an index into the lanes' array -- and the two stages' stream programs with the option in them.  The blocks of a
// TSDU and the words of a voice unit are decoded by the walks of tsbk_core_check.cpp and p25es_core_check.cpp, included here
// in namespaces of their own; what follows tsbk_kernel and p25lc_kernel anew is the frame walk and the place of the NID.
//   nid_core_check words <words.u64>     per 63-bit word (code bit 0 highest): nid_fix and the word after decoding
//   nid_core_check stream tsbk|voice <words.u32> <hits.u32> <correct> <options> <nid> <first_hit> <word_cap> <hit_cap> <n_words n_hits n_symbols n_k> ...
//       one launch per quadruple; prints the stage's five counters and the NID's four, then every record as 8 hex words
// tests/test_nid_cpu.py holds the output to the restatement's (tests/nid_ref.py) and to the reference's answers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "../../radiocapture-rf_amd/csrc/nid_core.hpp"

#define main tsbk_check_main
namespace tsbkc {
#include "tsbk_core_check.cpp"
}
#undef main
#define main p25es_check_main
namespace voicec {
#include "p25es_core_check.cpp"
}
#undef main

using namespace rcfx;

namespace {

typedef uint32_t Lanes[64];

uint32_t wave_xor(const Lanes &v)
{
    uint32_t r = 0;
    for (int l = 0; l < 64; ++l) r ^= v[l];
    return r;
}
uint64_t ballot(const bool (&b)[64])
{
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)b[l] << l;
    return m;
}

// nid_decode_wave of nid_wave.hpp, step by step over the 64 lanes
uint64_t nid_decode_wave(uint64_t r, int *fix)
{
    Lanes S, C, B;
    for (int l = 0; l < 64; ++l) { S[l] = nid_syndrome(r, l); C[l] = B[l] = l == 0 ? 1u : 0u; }
    uint32_t b = 1;
    int Ln = 0, m = 1;
    for (int rd = 0; rd < kNidRoots; ++rd) {
        Lanes term, Bs;
        for (int l = 0; l < 64; ++l) {
            term[l] = l <= rd ? p25lc_gf_mul(C[l], S[(rd - l) & 63]) : 0u;
            Bs[l] = B[(l - m) & 63];
        }
        const uint32_t d = wave_xor(term);
        if (d == 0) { ++m; continue; }
        Lanes Cn;
        for (int l = 0; l < 64; ++l) Cn[l] = C[l] ^ p25lc_gf_mul(p25lc_gf_mul(d, p25lc_gf_inv(b)), l >= m ? Bs[l] : 0u);
        if (2 * Ln <= rd) { memcpy(B, C, sizeof(B)); Ln = rd + 1 - Ln; b = d; m = 1; } else ++m;
        memcpy(C, Cn, sizeof(C));
    }
    bool root[64], nz[64];
    for (int l = 0; l < 64; ++l) {
        const uint32_t xi = l < kNidBits ? nid_xinv(l) : 0u;
        uint32_t v = 0;
        for (int j = kNidT; j >= 0; --j) v = p25lc_gf_mul(v, xi) ^ C[j];
        root[l] = l < kNidBits && v == 0;
    }
    const uint64_t roots = ballot(root);
    const bool ok = Ln <= kNidT && slice_popcount64(roots) == Ln;
    const uint64_t fixed = r ^ roots;
    for (int l = 0; l < 64; ++l) nz[l] = nid_syndrome(fixed, l) != 0;
    const bool bad = !ok || ballot(nz) != 0;
    *fix = bad ? kNidFixBad : Ln;
    return bad ? r : fixed;
}

struct NidCount { int64_t decoded = 0, fixed = 0, bits = 0, bad = 0; };
void count(NidCount &nc, int fix)
{
    ++nc.decoded;
    if (fix == kNidFixBad) ++nc.bad;
    else if (fix) { ++nc.fixed; nc.bits += fix; }
}

struct State { int64_t n_records = 0, n_frames = 0, n_a = 0, n_b = 0, n_lost = 0, next_hit = 0, k_last = kTsbkNoFrame; };
typedef voicec::Rings Rings;

// the frame walk the two kernels share; frame(s, fd, k0, dist) decodes one decided frame
template <class Frame>
void walk(const Rings &R, State &st, int decide, int longest, int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k, Frame &&frame)
{
    int64_t i = st.next_hit, k_last = st.k_last;
    const int64_t hit_cap = (int64_t)R.hit_mask + 1, word_cap = (int64_t)R.word_mask + 1;
    if (i < n_hits - hit_cap) { st.n_lost += n_hits - hit_cap - i; i = n_hits - hit_cap; }
    const int bound = n_k + decide + 32;
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
        if (16 * n_words < s + decide) break;
        bool nb_[64];
        for (int l = 0; l < 64; ++l) nb_[l] = valid[l] && l > a && tsbk_accept(k[l], k0);
        const uint64_t nxt = ballot(nb_);
        int fd = longest;
        if (nxt) {
            const int64_t gap = k[__builtin_ctzll(nxt)] - k0;
            if (gap < fd) fd = (int)gap;
        }
        ++i; k_last = k0; ++st.n_frames;
        if ((s >> 4) < n_words - word_cap) { ++st.n_lost; continue; }
        frame(s, fd, k0, dist);
    }
    st.next_hit = i; st.k_last = k_last;
}

// the NID of the frame at s: its two words as received, and with the option the decoded first word and nid_fix
void read_nid(const Rings &R, int64_t s, bool nid, NidCount &nc, uint32_t *nid0, uint32_t *nid1, uint32_t *nidc, int *fix)
{
    bool hb[64], lb[64];
    for (int l = 0; l < 64; ++l) {
        const int dn = l < 32 ? voicec::ring_dibit(R, s + tsbk_frame_pos(24 + l)) : 0;
        hb[l] = dn & 2; lb[l] = dn & 1;
    }
    const uint64_t nhi = ballot(hb), nlo = ballot(lb);
    *nid0 = *nidc = slice_word_be(nhi, nlo, 2, 0);
    *nid1 = slice_word_be(nhi, nlo, 2, 1);
    *fix = -1;
    if (nid) {
        *nidc = nid_word0_of(nid_decode_wave(nid_poly(*nid0, *nid1), fix));
        count(nc, *fix);
    }
}

void tsbk_frame(const Rings &R, State &st, bool nid, NidCount &nc, int64_t s, int fd, int64_t k0, uint32_t dist, std::vector<uint32_t> &out)
{
    uint32_t nid0, nid1, nidc;
    int fix;
    read_nid(R, s, nid, nc, &nid0, &nid1, &nidc, &fix);
    const uint32_t w7 = (uint32_t)fd | (nid ? nid_tsbk_word7(fix) : 0u);
    const int nb = tsbk_duid(nidc) == 7 ? tsbk_blocks_in(fd) : 0;
    if (nb == 0) {
        const uint32_t rec[8] = {tsbk_word0(3, false, 0, 0, dist, nidc), (uint32_t)(uint64_t)k0, 0, 0, 0, slice_word_mem(nid0), slice_word_mem(nid1), w7};
        out.insert(out.end(), rec, rec + 8);
        ++st.n_records;
        return;
    }
    const tsbkc::Rings TR{R.words, R.hits, R.word_mask, R.hit_mask};
    for (int b = 0; b < nb; ++b) {
        uint32_t rec[8];
        bool bad;
        tsbkc::decode_block(TR, s, fd, b, dist, nidc, nid1, k0, rec, &bad);
        rec[5] = slice_word_mem(nid0); rec[7] = w7;                  // (the NID as received; word 7 with the option's bits)
        out.insert(out.end(), rec, rec + 8);
        ++st.n_records; ++st.n_a;
        st.n_b += bad ? 1 : 0;
    }
}

// p25lc_kernel behind the NID (p25es_core_check.cpp's launch from there on)
void voice_frame(const Rings &R, State &st, uint32_t flags, NidCount &nc, int64_t s, int fd, int64_t k0, uint32_t dist, std::vector<uint32_t> &out)
{
    using voicec::rs_decode;
    const bool correct = flags & kP25lcFlagCorrect, erasures = flags & kP25lcFlagErasures, nid = flags & kNidFlagBch;
    uint32_t nid0, nid1, nidc;
    int fix;
    read_nid(R, s, nid, nc, &nid0, &nid1, &nidc, &fix);
    const uint32_t w0 = nid ? kNidP25lcWord0 : 0u, w7 = nid ? nid_p25lc_word7(fix) : 0u;
    const auto dibit = [&R, s](int r) { return voicec::ring_dibit(R, s + r); };
    const int kind = p25lc_kind(tsbk_duid(nidc), fd, flags), wk = p25lc_words_kind(kind);
    uint32_t rec[8] = {p25lc_word0(kind, false, 0, dist, nidc) | w0, (uint32_t)(uint64_t)k0, 0, 0, 0, 0, 0, p25lc_word7(fd, 0, 0) | w7};
    ++st.n_records;
    if (kind == kP25lcFrame) { out.insert(out.end(), rec, rec + 8); return; }
    Lanes data, two;
    bool fixedb[64], badb[64], hb[64], lb[64];
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
    rec[0] = p25lc_word0_wide(kind, rs_bad, n_rs, dist, nidc) | w0;
    rec[6] = slice_word_mem(slice_word_be(ballot(hb), ballot(lb), 2, 0));
    rec[7] = p25lc_word7(fd, slice_popcount64(ballot(fixedb)), slice_popcount64(ballot(badb))) | w7;
    out.insert(out.end(), rec, rec + 8);
    ++st.n_a;
    st.n_b += rs_bad ? 1 : 0;
}

int mode_stream(int argc, char **argv)
{
    if (argc < 11 || (argc - 11) % 4) return 2;
    const bool voice = !strcmp(argv[2], "voice");
    Rings R{voicec::read_file<uint32_t>(argv[3]), voicec::read_file<uint32_t>(argv[4]), (uint32_t)atoll(argv[9]) - 1u, (uint32_t)atoll(argv[10]) - 1u};
    const bool nid = atoi(argv[7]) != 0;
    const uint32_t flags = (atoi(argv[5]) ? kP25lcFlagCorrect : 0u) | (uint32_t)atoi(argv[6]) << 1 | (nid ? kNidFlagBch : 0u);
    State st;
    NidCount nc;
    st.next_hit = atoll(argv[8]);
    std::vector<uint32_t> out;
    for (int i = 11; i + 3 < argc; i += 4) {
        const int64_t n_words = atoll(argv[i]), n_hits = atoll(argv[i + 1]), n_sym = atoll(argv[i + 2]);
        if (n_words > (int64_t)R.words.size() || n_hits > (int64_t)R.hits.size()) return 2;
        if (voice)
            walk(R, st, kP25lcDecideDibits, kP25lcFrameDibits, n_words, n_hits, n_sym, atoi(argv[i + 3]),
                 [&](int64_t s, int fd, int64_t k0, uint32_t dist) { voice_frame(R, st, flags, nc, s, fd, k0, dist, out); });
        else
            walk(R, st, kTsbkDecideDibits, kTsbkFrameDibits, n_words, n_hits, n_sym, atoi(argv[i + 3]),
                 [&](int64_t s, int fd, int64_t k0, uint32_t dist) { tsbk_frame(R, st, nid, nc, s, fd, k0, dist, out); });
    }
    printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " nid %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", st.n_records, st.n_frames,
           st.n_a, st.n_b, st.n_lost, nc.decoded, nc.fixed, nc.bits, nc.bad);
    for (size_t r = 0; r + 8 <= out.size(); r += 8)
        for (int q = 0; q < 8; ++q) printf("%08x%s", out[r + q], q == 7 ? "\n" : " ");
    return st.n_records * 8 == (int64_t)out.size() ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "words")) {
        for (uint64_t w : voicec::read_file<uint64_t>(argv[2])) {
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
