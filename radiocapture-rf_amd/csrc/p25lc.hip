// p25lc.hip -- P25 voice data units behind a channel's slicer (gfx950): what the reference's voice-channel consumer does per
// frame in Python (logging_receiver.p25_sensor: p25_general.procHDU / procLDU1 / procTLC with the codecs of hamming.py,
// golay.py and rs64.py) -- strip the status symbols, read the NID, and for a header, an LDU1 or a terminator with link
// control decode the inner Golay / Hamming words and the outer Reed-Solomon word --, every such stage of a block (or of a
// group's block) in one launch behind slice_kernel's.  include/rcf.h at rcf_chan_p25lc DEFINES the stage, tests/p25lc_ref.py
// restates it; the arithmetic is p25lc_core.hpp, which the CPU suite compiles for the host as it stands.
//
// The slicer's layout: a WAVE is a channel, four channels per workgroup.  The walk over the hit ring, the accept rule and
// the frame's length are item_wave.hpp's frame_walk with P25lcWalk: tsbk.hip's, with 864 + 24 dibits to wait for.  Per decided
// frame the lanes 0 .. 31 gather the NID (nid_wave.hpp).  Then lane w is inner word w (36, 24 or 12 lanes): it gathers its
// 9, 5 or 12 dibits through the status-symbol map, takes the syndrome with masks and popcount parity (Hamming) or twelve
// shift / xor rounds and the syndrome table (Golay; see p25lc_core.hpp for why a table) and corrects.  The Reed-Solomon word has a symbol per lane:
//   syndromes       lane m runs Horner over the symbols, read uniformly, for S[m] = r(alpha^(m + 1))
//   Berlekamp-      a fixed 2 t rounds, coefficient i of the locator and of the shadow polynomial in lane i; a round is
//   Massey          one lane-reversed read of S, a product, an xor-reduction over the wave (the discrepancy, then in every
//                   lane) and one shifted read of the shadow polynomial
//   Chien           lane i evaluates the locator at 1 / X_i; the ballot of the zeros is the error set, which must have as
//                   many members as the locator's degree (a root outside the n positions is missing there)
//   Forney          lane m forms coefficient m of S(x) Lambda(x), the error lanes evaluate it and the derivative
//   re-check        the syndromes of the corrected word, again one per lane
// instead of lane 0 walking dependent chains over 36 symbols with 63 lanes idle.  The options of rcf_chan_p25lc_opt: an LDU2 is
// a fourth unit on the LDU1's lanes with RS(24,16,9); with erasures the ballot of the BAD lanes is the erased set and rs_decode
// runs as rs_decode<true>, chosen by a wave-uniform branch on the flag, so a stage without the option walks the loops of t.  The lanes 0 .. 3 cut the payload words out
// of the data symbols, the lanes 0 .. 7 store a record's eight words.
// The decoders' trip counts are compile-time constants.  Every ring index is masked.  Plain vector stores only; nothing is
// shared between waves; no LDS.  Every cross-lane read stands in wave-uniform control flow.
// The option RCF_NID_BCH (kNidFlagBch): the NID's 63 bits go through nid_wave.hpp's decoder before the DUID names the unit's
// kind, behind a wave-uniform branch like the other options.
#include "item_wave.hpp"
#include "p25lc_core.hpp"
#include "nid_wave.hpp"

namespace rcfx {

namespace {

constexpr int kP25lcWaves = kItemWaves;

// lane m < 2 t: S[m] = the word's value at alpha^(m + 1); the other lanes 0
__device__ __forceinline__ uint32_t rs_syndrome(uint32_t sym, int n, int t, int lane)
{
    const uint32_t am = p25lc_gf_alpha(lane + 1);
    uint32_t S = 0;
    for (int i = 0; i < kP25lcMaxSyms; ++i) {
        const uint32_t r = lane_read(sym, i);
        if (i < n) S = p25lc_gf_mul(S, am) ^ r;
    }
    return lane < 2 * t ? S : 0u;
}
// the symbols of RS(n, n - 2 t) (lane i: symbol i; the lanes >= n hold 0) -> the corrected symbols, or the symbols as they
// are with *rs_bad; *n_rs: the symbols changed.  kErasures: E, the ballot of the erased symbols, enters -- the locator starts
// as the erasure locator prod (1 + X_j x) over E (coefficient i in lane i, a member of E per uniform round), Berlekamp-Massey
// from round |E| on, and Chien, Forney and the products run to degree d - 1 and no longer t: the joint locator of |E|
// erasures and v errors with 2 v + |E| <= d - 1.  Without it E is 0 and every bound the errors-only decoder's
template <bool kErasures>
__device__ __forceinline__ uint32_t rs_decode(uint32_t sym, uint64_t E, int n, int t, int lane, bool *rs_bad, int *n_rs)
{
    constexpr int kDeg = kErasures ? kP25lcMaxD1 : kP25lcMaxT;       // the locator's highest degree
    const int ne = kErasures ? __popcll(E) : 0;
    const uint32_t S = rs_syndrome(sym, n, t, lane);
    uint32_t C = lane == 0 ? 1u : 0u;
    if (kErasures) {
        uint64_t rest = ne <= 2 * t ? E : 0ull;      // (more than d - 1: given up below)
        for (int r = 0; r < kP25lcMaxD1; ++r) {
            const uint32_t up = lane_read(C, lane - 1);
            if (!rest) continue;                     // (uniform)
            C ^= p25lc_gf_mul(p25lc_rs_x(n, __builtin_ctzll(rest)), lane ? up : 0u);
            rest &= rest - 1;
        }
    }
    uint32_t B = C, b = 1;
    int Ln = ne, m = 1;
    for (int r = 0; r < 2 * kP25lcMaxT; ++r) {
        const uint32_t Sr = lane_read(S, r - lane);
        const uint32_t d = wave_xor(lane <= r ? p25lc_gf_mul(C, Sr) : 0u);
        const uint32_t Bs = lane_read(B, lane - m);
        if (r < ne || r >= 2 * t) continue;          // (uniform)
        if (d == 0) { ++m; continue; }
        const uint32_t Cn = C ^ p25lc_gf_mul(p25lc_gf_mul(d, p25lc_gf_inv(b)), lane >= m ? Bs : 0u);
        if (2 * Ln <= r + ne) { B = C; Ln = r + 1 - Ln + ne; b = d; m = 1; } else ++m;
        C = Cn;
    }
    const uint32_t xi = lane < n ? p25lc_rs_xinv(n, lane) : 0u, xi2 = p25lc_gf_mul(xi, xi);
    uint32_t v = 0, om = 0;
    for (int j = kDeg; j >= 0; --j) v = p25lc_gf_mul(v, xi) ^ lane_read(C, j);
    const bool root = lane < n && v == 0;
    const uint64_t roots = __ballot(root);
    const bool ok = 2 * Ln - ne <= 2 * t && __popcll(roots) == Ln && (roots & E) == E;
    for (int i = 0; i <= kDeg; ++i) {                // coefficient `lane` of S(x) Lambda(x)
        const uint32_t ci = lane_read(C, i), si = lane_read(S, lane - i);
        if (i <= lane) om ^= p25lc_gf_mul(ci, si);
    }
    if (kErasures && lane >= 2 * t) om = 0;          // ... modulo x^(2 t): its degree is below the locator's, which t no longer bounds
    uint32_t num = 0, den = 0;
    for (int j = kDeg - 1; j >= 0; --j) num = p25lc_gf_mul(num, xi) ^ lane_read(om, j);
    for (int j = kDeg - 1; j >= 1; j -= 2) den = p25lc_gf_mul(den, xi2) ^ lane_read(C, j);
    const uint32_t e = root && den ? p25lc_gf_mul(num, p25lc_gf_inv(den)) : 0u;
    const uint32_t fixed = sym ^ e;
    const bool left = __ballot(rs_syndrome(fixed, n, t, lane) != 0) != 0;
    *rs_bad = !ok || left;
    *n_rs = *rs_bad ? 0 : __popcll(__ballot(e != 0));
    return *rs_bad ? sym : fixed;
}

__global__ __launch_bounds__(64 * kP25lcWaves) void p25lc_kernel(const P25lcLaunch *__restrict__ items, int n_items)
{
    int lane;
    const int w = item_of_wave(n_items, &lane);
    if (w < 0) return;
    const P25lcLaunch L = items[w];
    P25lcState *st = L.st;
    const bool correct = L.flags & kP25lcFlagCorrect, erasures = L.flags & kP25lcFlagErasures, nid = L.flags & kNidFlagBch;
    NidCount nc;
    int64_t n_records = st->n_records, n_decoded = st->n_decoded, n_rs_bad = st->n_rs_bad;
    FrameWalk walk(st);
    frame_walk<P25lcWalk>(L, lane, walk, [&](int64_t s, int fd, int64_t k0, uint32_t dist) __attribute__((always_inline)) {
        const auto dibit = [&L, s](int r) { return ring_dibit(L, s + r); };
        const Nid id = read_nid(L, s, lane, nid, nc);
        const uint32_t nid0 = id.word0;              // (decoded with the option)
        const uint32_t w0 = nid ? kNidP25lcWord0 : 0u, w7 = nid ? nid_p25lc_word7(id.fix) : 0u;      // what the option adds to the words 0 and 7
        const int kind = __builtin_amdgcn_readfirstlane(p25lc_kind(tsbk_duid(nid0), fd, L.flags));
        uint32_t *rec = L.rec_ring + ((uint64_t)n_records & L.rec_mask) * kP25lcRecWords;
        ++n_records;
        if (kind == kP25lcFrame) {
            const uint32_t v = lane == 0 ? p25lc_word0(kind, false, 0, dist, nid0) | w0 : lane == 1 ? (uint32_t)(uint64_t)k0 : lane == 7 ? p25lc_word7(fd, 0, 0) | w7 : 0u;
            if (lane < kP25lcRecWords) rec[lane] = v;
            return;
        }
        // ---- inner word `lane`
        const int wk = p25lc_words_kind(kind);       // (an LDU2's words are an LDU1's)
        const bool mine = lane < p25lc_inner_words(wk);
        const uint32_t word = mine ? p25lc_gather(dibit, wk, lane) : 0u;
        int status = 0;
        uint32_t data = mine ? (correct ? p25lc_inner(kind, word, &status, erasures) : p25lc_systematic(wk, word)) : 0u;
        uint64_t bad = __ballot(mine && status == 2);
        const int n_fixed = __popcll(__ballot(mine && status == 1)), n_bad = __popcll(bad);
        const int n = p25lc_rs_n(wk), kk = p25lc_rs_k_es(kind);
        if (kind == kP25lcTlc) {                     // a Golay word is two symbols
            const uint32_t two = lane_read(data, lane >> 1);
            data = lane < n ? (lane & 1 ? two & 63u : two >> 6) : 0u;
            bad = __ballot(lane < n && (bad >> (lane >> 1) & 1));
        }
        bool rs_bad = false;
        int n_rs = 0;
        if (correct && erasures) data = rs_decode<true>(data, bad, n, p25lc_rs_t_es(kind), lane, &rs_bad, &n_rs);          // (uniform, both)
        else if (correct) data = rs_decode<false>(data, 0, n, p25lc_rs_t_es(kind), lane, &rs_bad, &n_rs);
        // ---- the payload: the data symbols' bits, the lanes 0 .. 3 a word each
        uint64_t pay = 0;
        for (int j = 0; j < 7; ++j) {
            const int at = p25lc_pay_first(lane & 3) + j;
            const uint32_t v = lane_read(data, at);
            pay = pay << 6 | (at < kk ? v : 0u);
        }
        const uint32_t pw = lane_read(slice_word_mem(p25lc_pay_word(pay, lane & 3)), lane - 2);
        const int dl = p25lc_has_lsd(kind) && lane < 16 ? dibit(tsbk_frame_pos(kP25lcLsdDibit + lane)) : 0;
        const uint64_t lhi = __ballot(dl & 2), llo = __ballot(dl & 1);
        const uint32_t v = lane == 0 ? p25lc_word0_wide(kind, rs_bad, n_rs, dist, nid0) | w0 : lane == 1 ? (uint32_t)(uint64_t)k0 : lane < 6 ? pw :
                           lane == 6 ? slice_word_mem(slice_word_be(lhi, llo, 2, 0)) : p25lc_word7(fd, n_fixed, n_bad) | w7;
        if (lane < kP25lcRecWords) rec[lane] = v;
        ++n_decoded;
        n_rs_bad += rs_bad ? 1 : 0;
    });
    if (lane == 0) {
        st->n_records = n_records; st->n_decoded = n_decoded; st->n_rs_bad = n_rs_bad;
        walk.store(st);
        if (nid) nc.store(st);
    }
}

}  // namespace

// ring_mask: unused -- every record carries the masks of its three rings
void launch_p25lc(const P25lcLaunch *d_items, int n_items, int max_n_k, uint64_t, hipStream_t s)
{
    launch_item_waves(p25lc_kernel, d_items, n_items, max_n_k, s);
}

}  // namespace rcfx
