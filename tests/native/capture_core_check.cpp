// capture_core_check.cpp -- radiocapture-rf_amd/csrc/capture_core.hpp compiled for the host: a stand-alone walk of the
// carrier-operated capture over streams of samples, piece by piece, the way capture_kernel (capture.hip) walks a block: the
// detector at index j, the writer at j - pre re-reading the stream there -- every power, step, decision, record and
// accumulator coming from the header's own functions.
//   capture_core_check <samples.cf32> <cases.txt>
// cases.txt, one case per line:  offset count threshold_db alpha a pre hang n0 n1 ...
//   the case's stream is samples [offset, offset + count) of the file, its first sample the channel's output a (the attach
//   point); one piece per n (0 allowed), the state carried from piece to piece.  threshold_db and alpha are parsed with
//   strtod: hexadecimal floats give the test's doubles exactly.
// Output per case: "CASE", then per piece its events in order --
//   "R kind n_open sample pos peak(hex)" and "K sample re(bits) im(bits)" for every kept sample --
// and "S level(hex) n_seen n_decided n_kept n_records n_windows last_open in_window unmuted" as of the piece's end.
// tests/test_capture_cpu.py holds the output to the numpy restatement's (tests/capture_ref.py).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#define RCF_DEVFN static inline
#include "../../radiocapture-rf_amd/csrc/capture_core.hpp"

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

uint32_t bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, sizeof(u));
    return u;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: see the head of the source\n"); return 2; }
    const std::vector<float> x = load(argv[1]);
    FILE *cf = fopen(argv[2], "r");
    if (!cf) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    std::string text;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), cf)) > 0) text.append(buf, got);
    fclose(cf);
    std::istringstream lines(text);
    std::string line;
    while (std::getline(lines, line)) {
        std::istringstream in(line);
        std::string s_off, s_cnt, s_thr, s_alpha, s_a, s_pre, s_hang;
        if (!(in >> s_off >> s_cnt >> s_thr >> s_alpha >> s_a >> s_pre >> s_hang)) continue;
        const size_t off = (size_t)strtoull(s_off.c_str(), nullptr, 10), count = (size_t)strtoull(s_cnt.c_str(), nullptr, 10);
        if (off + count > x.size() / 2) { fprintf(stderr, "case runs past the file\n"); return 2; }
        const double thr = squelch_threshold(strtod(s_thr.c_str(), nullptr)), alpha = strtod(s_alpha.c_str(), nullptr);
        const double one_minus_alpha = 1.0 - alpha;
        const int64_t a = strtoll(s_a.c_str(), nullptr, 10), pre = strtoll(s_pre.c_str(), nullptr, 10), hang = strtoll(s_hang.c_str(), nullptr, 10);
        if (pre < 0 || hang < 0) { fprintf(stderr, "negative pre or hang\n"); return 2; }
        printf("CASE\n");
        CaptureWalk w{0.0, -1, 0, 0, 0, 0, 0.0, 0, 0};
        int64_t n_seen = 0, n_decided = 0;
        size_t at = 0;                                       // samples of the case walked so far
        std::string s_n;
        while (in >> s_n) {
            const size_t n = (size_t)strtoull(s_n.c_str(), nullptr, 10);
            if (at + n > count) { fprintf(stderr, "piece of %zu samples runs past the case's %zu\n", n, count); return 2; }
            for (size_t i = 0; i < n; ++i) {
                const int64_t j = a + (int64_t)(at + i), s = j - pre;
                capture_detect(w, alpha, one_minus_alpha, thr, squelch_power(x.at(2 * (off + at + i)), x.at(2 * (off + at + i) + 1)), j);
                if (s < a) continue;                         // the lead-in is clipped at the attach point
                CaptureRec ev;
                const bool keep = capture_write(w, hang, s, &ev);
                ++n_decided;
                if (ev.kind) printf("R %u %u %" PRId64 " %" PRId64 " %a\n", ev.kind, ev.n_open, ev.sample, ev.pos, (double)ev.peak);
                if (keep) {
                    const size_t k = off + (size_t)(s - a);  // the writer re-reads the stream pre samples back
                    printf("K %" PRId64 " %u %u\n", s, bits(x.at(2 * k)), bits(x.at(2 * k + 1)));
                }
            }
            at += n;
            n_seen += (int64_t)n;
            printf("S %a %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d\n", w.level, n_seen, n_decided, w.n_kept,
                   w.n_records, w.n_windows, w.last_open, (int)w.in_window, (int)w.unmuted);
        }
    }
    return 0;
}
