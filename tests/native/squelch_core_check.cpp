// squelch_core_check.cpp -- radiocapture-rf_amd/csrc/squelch_core.hpp compiled for the host: a stand-alone walk of the carrier
// detector over one stream of samples, block by block, in both forms the kernels (squelch.hip) evaluate it in -- every power,
// step, comparison, carry and entry level coming from the header's own functions.
//   squelch_core_check seq <samples.cf32> <threshold_db> <alpha> <first_index> <n0 n1 ...>
//       squelch_kernel's walk: one block per count (0 allowed), the state carried from block to block
//   squelch_core_check seg <samples.cf32> <threshold_db> <alpha> <first_index> <segment> <n0 n1 ...>
//       the bank's two passes per block: the zero-state response of every whole segment but the block's last, then per segment
//       the entry level from the z before it and the walk from there; counts and last-open indices summed over the segments
//   both print, per block, "level(hex) n_seen n_open first_open last_open unmuted" as of the block's end
//   squelch_core_check thr <db> ...      prints squelch_threshold(db) for every argument, as hexadecimal doubles
// threshold_db and alpha are parsed with strtod: hexadecimal floats give the test's doubles exactly.
// tests/test_squelch_cpu.py holds the output to the numpy restatement's (tests/squelch_ref.py).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RCF_DEVFN static inline
#include "../../radiocapture-rf_amd/csrc/squelch_core.hpp"

using namespace rcfx;

namespace {

std::vector<float> load(const char *path)
{
    std::vector<float> v;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    float buf[1024];
    size_t n;
    while ((n = fread(buf, sizeof(float), 1024, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    if (v.size() % 2) { fprintf(stderr, "%s holds half a sample\n", path); exit(2); }
    return v;
}

void print(const SquelchWalk &w, int64_t n_seen)
{
    printf("%a %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d\n", w.level, n_seen, w.n_open, w.first_open, w.last_open, (int)w.unmuted);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "thr")) {
        for (int i = 2; i < argc; ++i) printf("%a\n", squelch_threshold(strtod(argv[i], nullptr)));
        return 0;
    }
    const bool seg = argc >= 2 && !strcmp(argv[1], "seg");
    if (argc < (seg ? 7 : 6) || (!seg && strcmp(argv[1], "seq"))) { fprintf(stderr, "usage: see the head of the source\n"); return 2; }
    const std::vector<float> x = load(argv[2]);
    const size_t n_total = x.size() / 2;
    const double thr = squelch_threshold(strtod(argv[3], nullptr)), alpha = strtod(argv[4], nullptr), one_minus_alpha = 1.0 - alpha;
    const int64_t first_index = strtoll(argv[5], nullptr, 10);
    const int S = seg ? atoi(argv[6]) : 0;
    if (seg && S < 1) { fprintf(stderr, "segment %d\n", S); return 2; }
    const double a_pow_s = seg ? squelch_a_pow_s(alpha, S) : 0.0;
    SquelchWalk w{0.0, 0, -1, -1, 0};
    int64_t n_seen = 0;
    size_t at = 0;
    for (int a = seg ? 7 : 6; a < argc; ++a) {
        const size_t n = (size_t)strtoull(argv[a], nullptr, 10);
        if (at + n > n_total) { fprintf(stderr, "block of %zu samples runs past the file's %zu\n", n, n_total); return 2; }
        const auto re = [&](size_t i) { return x.at(2 * (at + i)); };
        const auto im = [&](size_t i) { return x.at(2 * (at + i) + 1); };
        if (!seg) {
            for (size_t i = 0; i < n; ++i) squelch_walk_step(w, alpha, one_minus_alpha, thr, re(i), im(i), first_index + (int64_t)(at + i));
        } else if (n > 0) {
            const size_t segs = (n + (size_t)S - 1) / (size_t)S;
            // pass 1 (pfb_squelch_z_kernel): whole segments, all but the block's last
            std::vector<double> z(segs - 1, 0.0);
            for (size_t s = 0; s + 1 < segs; ++s)
                for (size_t i = s * S; i < (s + 1) * S; ++i) z.at(s) = squelch_step(z.at(s), alpha, one_minus_alpha, squelch_power(re(i), im(i)));
            // pass 2 (pfb_squelch_walk_kernel): every segment on its own, from the level before the block
            const double level_in = w.level;
            for (size_t s = 0; s < segs; ++s) {
                double level = level_in;
                for (size_t j = 0; j < s; ++j) level = squelch_enter(z.at(j), level, a_pow_s, one_minus_alpha);
                SquelchWalk ws{level, 0, -1, -1, 0};
                const size_t hi = s * S + S < n ? s * S + S : n;
                for (size_t i = s * S; i < hi; ++i) squelch_walk_step(ws, alpha, one_minus_alpha, thr, re(i), im(i), first_index + (int64_t)(at + i));
                w.n_open += ws.n_open;                                  // (the atomic add and max of the kernel)
                if (ws.n_open > 0) {
                    if (w.first_open < 0 || ws.first_open < w.first_open) w.first_open = ws.first_open;
                    if (ws.last_open > w.last_open) w.last_open = ws.last_open;
                }
                if (s + 1 == segs) { w.level = ws.level; w.unmuted = ws.unmuted; }
            }
        }
        at += n;
        n_seen += (int64_t)n;
        print(w, n_seen);
    }
    return 0;
}
