// voice_decode_host.hpp -- p25lc_kernel's decided frame (radiocapture-rf_amd/csrc/p25lc.hip) on the host, for the check
// programs of the P25 voice stage and its options: the 64 lanes of a wave as a loop, a ballot as the mask that loop builds,
// a lane read as an index into the lanes' array, with every index map, inner decoder, field product and record word coming
// from p25lc_core.hpp's own functions.  With the options of rcf_chan_p25lc_opt: the LDU2 as a unit of kind 4, the (24,12)
// word's 24th bit, the ballot of the words given up as the erased set, and rs_decode<true>: erasure locator,
// Berlekamp-Massey from round |E|, Chien, Forney and the products to degree d - 1.
#pragma once
#include "nid_decode_host.hpp"

namespace {

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

// one decided frame -> its record (st.n_a: decoded, st.n_b: rs_bad); flags: P25lcLaunch's
void voice_frame(const Rings &R, State &st, uint32_t flags, NidCount &nc, int64_t s, int fd, int64_t k0, uint32_t dist, std::vector<uint32_t> &out)
{
    const bool correct = flags & kP25lcFlagCorrect, erasures = flags & kP25lcFlagErasures, nid = flags & kNidFlagBch;
    uint32_t nid0, nid1, nidc;
    int fix;
    read_nid(R, s, nid, nc, &nid0, &nid1, &nidc, &fix);
    const uint32_t w0 = nid ? kNidP25lcWord0 : 0u, w7 = nid ? nid_p25lc_word7(fix) : 0u;
    const auto dibit = [&R, s](int r) { return ring_dibit(R, s + r); };
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

// a voice stream program's launches, from argv[first] on (for_launches)
bool voice_launches(const Rings &R, State &st, uint32_t flags, NidCount &nc, int argc, char **argv, int first, std::vector<uint32_t> &out)
{
    return for_launches(R, argc, argv, first, [&](int64_t n_words, int64_t n_hits, int64_t n_sym, int n_k) {
        walk<P25lcWalk>(R, st, n_words, n_hits, n_sym, n_k,
                        [&](int64_t s, int fd, int64_t k0, uint32_t dist) { voice_frame(R, st, flags, nc, s, fd, k0, dist, out); });
    });
}

}  // namespace
