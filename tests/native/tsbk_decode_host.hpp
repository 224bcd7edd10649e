// tsbk_decode_host.hpp -- tsbk_kernel's decided frame (radiocapture-rf_amd/csrc/tsbk.hip) on the host, for the check programs
// of the P25 trunking stage and its two options: the 64 lanes of a wave as a loop, a shuffle as an index into the lanes'
// array, a ballot as the mask that loop builds, with every index map, transition map, composition, min-plus matrix, CRC term
// and record word coming from tsbk_core.hpp's own functions.
#pragma once
#include "nid_decode_host.hpp"

namespace {

// the inclusive scan of 64 maps under composition, six steps (tsbk_kernel's loop)
void scan64(uint32_t (&map)[64])
{
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t before[64];
        for (int l = 0; l < 64; ++l) before[l] = map[l >= d ? l - d : l];
        for (int l = 0; l < 64; ++l)
            if (l >= d) map[l] = tsbk_compose(before[l], map[l]);
    }
}

// viterbi_map_wave of tsbk.hip over the 64 lanes; last: the lane of the flushing word (48 for a TSBK block)
void viterbi_maps(const uint32_t (&c)[64], int last, uint32_t (&map)[64], uint32_t *beta0)
{
    TsbkMat own[64], suffix[64];
    for (int l = 0; l < 64; ++l) suffix[l] = own[l] = l <= last ? tsbk_mat(c[l], l == last) : tsbk_mat_identity();
    for (int d = 1; d < 64; d <<= 1) {
        TsbkMat after[64];
        for (int l = 0; l < 64; ++l) after[l] = suffix[l + d < 64 ? l + d : l];
        for (int l = 0; l < 64; ++l)
            if (l + d < 64) suffix[l] = tsbk_mat_compose(suffix[l], after[l]);
    }
    for (int l = 0; l < 64; ++l) {
        const uint32_t beta_next = tsbk_mat_beta(suffix[l + 1 < 64 ? l + 1 : l]);
        map[l] = l > last ? kTsbkIdentity : tsbk_viterbi_map(own[l], l == last ? 0u : beta_next);
    }
    *beta0 = tsbk_mat_beta(suffix[0]) & 255u;        // the least cost from state 0
}

struct Decoded { int state[64]; int cost, n_inexact; };

// the block's lanes as tsbk_kernel goes through them: maps, the inclusive scan, the states, distance ballot and cost
Decoded wave_form(const uint32_t (&c)[64], int last, bool viterbi)
{
    uint32_t map[64], beta0 = 0;
    for (int l = 0; l < 64; ++l) map[l] = l <= last ? tsbk_map(c[l]) : kTsbkIdentity;
    if (viterbi) viterbi_maps(c, last, map, &beta0);
    scan64(map);
    Decoded r{};
    bool off[64];
    for (int l = 0; l < 64; ++l) {
        const int state = (int)(map[l] & 3u), prev = l ? (int)(map[l - 1] & 3u) : 0;
        r.state[l] = state;
        bool exact;
        (void)tsbk_next_state(prev, c[l], &exact);
        const int away = l <= last ? tsbk_branch_dist(prev, state, c[l]) : 0;
        off[l] = viterbi ? away != 0 : l <= last && !exact;
        r.cost += away;
    }
    r.n_inexact = slice_popcount64(ballot(off));
    if (viterbi && (int)beta0 != r.cost) { fprintf(stderr, "beta_0[0] %u is not the path's cost %d\n", beta0, r.cost); exit(1); }
    return r;
}

struct TrellisCount { int64_t decoded = 0, clean = 0, bits = 0, words = 0; };

// one decided frame -> its records (st.n_a: blocks, st.n_b: crc_bad)
void tsbk_frame(const Rings &R, State &st, bool nid, bool viterbi, NidCount &nc, TrellisCount &tc, int64_t s, int fd, int64_t k0, uint32_t dist,
                std::vector<uint32_t> &out)
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
    for (int b = 0; b < nb; ++b) {
        uint32_t c[64] = {0};
        for (int l = 0; l < kTsbkCodeWords; ++l) {
            const int j = tsbk_block_dibit(b, tsbk_deinterleave(l));
            c[l] = (uint32_t)(ring_dibit(R, s + tsbk_frame_pos(j)) << 2 | ring_dibit(R, s + tsbk_frame_pos(j + 1)));
        }
        const Decoded w = wave_form(c, kTsbkCodeWords - 1, viterbi);
        bool hi_b[64], lo_b[64];
        uint32_t crc = 0;
        for (int l = 0; l < 64; ++l) {
            hi_b[l] = l < 48 && (w.state[l] & 2);
            lo_b[l] = l < 48 && (w.state[l] & 1);
            if (l < 48) crc ^= tsbk_crc_term(l, w.state[l]);
        }
        const uint64_t hi = ballot(hi_b), lo = ballot(lo_b);
        const bool bad = crc != 0xffffu;
        const int jn = tsbk_frame_pos(tsbk_block_dibit(b, 98));
        const int next_bit = jn < fd ? ring_dibit(R, s + jn) >> 1 : 0;
        uint32_t rec[8] = {tsbk_word0(b, bad, next_bit, w.n_inexact, dist, nidc), (uint32_t)(uint64_t)k0, 0, 0, 0, slice_word_mem(nid0), slice_word_mem(nid1), w7};
        for (int q = 0; q < 3; ++q) rec[2 + q] = slice_word_mem(slice_word_be(hi, lo, 2, q));
        if (viterbi) {
            rec[7] |= tsbk_viterbi_word7(w.cost);
            ++tc.decoded; tc.clean += w.cost == 0 ? 1 : 0; tc.bits += w.cost; tc.words += w.n_inexact;
        }
        out.insert(out.end(), rec, rec + 8);
        ++st.n_records; ++st.n_a;
        st.n_b += bad ? 1 : 0;
    }
}

}  // namespace
