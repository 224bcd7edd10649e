// hard_bound_check -- g++ only.  Prints what rcf_streams.h (radiocapture-rf_amd/csrc) answers for the pump's slots of the
// streams behind the slicer, as JSON (tests/test_hard_delivery_host.py holds it against a restatement of its own):
//   "bound":  [what, bps, n_k, hard_bound] for every `what` in 0 .. 60 that read_kind knows -- -1 for a stream that is not a
//             hard one --, bps 1 and 2, n_k in {0, 1, 37, 500, 1200}
//   "slot":   [what, out_cap, item_bytes, slot_items] for out_cap in {16, 32, 64, 4096}
//   "ring":   per hard `what` and out_cap a host ring walked the way the pump's reader walks it: R = slot_items items of
//             item_bytes in a buffer of out_cap x 8 bytes, item i written at (i & (R - 1)) x item_bytes, then runs of odd lengths
//             copied out in the two pieces the wrap leaves.  [what, out_cap, items checked, mismatches].  Built with
//             -fsanitize=address,undefined this is where a ring that does not fit its slot shows.
#include <cstdio>
#include <cstring>
#include <vector>

#include "rcf_streams.h"

using namespace rcfx;

static long long ring_walk(int kind, long long out_cap, long long *checked)
{
    const size_t elem = read_row(kind).item_w * 4u, R = (size_t)slot_items(kind, out_cap);
    std::vector<unsigned char> slot((size_t)out_cap * 8), out;
    long long bad = 0, written = 0, cursor = 0;
    *checked = 0;
    for (int round = 0; round < 40; ++round) {
        const long long n_new = (round * 7 + 3) % (long long)R + 1;          // a gather of 1 .. R items
        for (long long i = written; i < written + n_new; ++i)
            for (size_t b = 0; b < elem; ++b) slot[(size_t)((unsigned long long)i & (R - 1)) * elem + b] = (unsigned char)(i * 131 + (long long)b * 7);
        written += n_new;
        if (cursor < written - (long long)R) cursor = written - (long long)R;
        const size_t n = (size_t)(written - cursor), pos = (size_t)((unsigned long long)cursor & (R - 1)), first = n < R - pos ? n : R - pos;
        out.assign(n * elem, 0);
        std::memcpy(out.data(), slot.data() + pos * elem, first * elem);
        if (n > first) std::memcpy(out.data() + first * elem, slot.data(), (n - first) * elem);
        for (size_t j = 0; j < n; ++j)
            for (size_t b = 0; b < elem; ++b) {
                bad += out[j * elem + b] != (unsigned char)((cursor + (long long)j) * 131 + (long long)b * 7);
                ++*checked;
            }
        if (round % 3) cursor = written;                                      // (every third round the reader sleeps)
    }
    return bad;
}

int main()
{
    const long long n_ks[] = {0, 1, 37, 500, 1200}, caps[] = {16, 32, 64, 4096};
    printf("{\"bound\": [");
    bool first = true;
    for (int what = 0; what <= 60; ++what) {
        const int k = read_kind(what);
        if (k < 0) continue;
        for (int bps = 1; bps <= 2; ++bps)
            for (long long n : n_ks) { printf("%s[%d, %d, %lld, %lld]", first ? "" : ", ", what, bps, n, (long long)hard_bound(k, n, bps)); first = false; }
    }
    printf("],\n \"slot\": [");
    first = true;
    for (int what = 0; what <= 60; ++what) {
        const int k = read_kind(what);
        if (k < 0) continue;
        for (long long c : caps) { printf("%s[%d, %lld, %u, %lld]", first ? "" : ", ", what, c, read_row(k).item_w * 4u, (long long)slot_items(k, c)); first = false; }
    }
    printf("],\n \"ring\": [");
    first = true;
    for (int what = 0; what <= 60; ++what) {
        const int k = read_kind(what);
        if (k < 0 || hard_bound(k, 0, 1) < 0) continue;
        for (long long c : caps) {
            if (slot_items(k, c) < 16) continue;                              // RCF_ECAP
            long long checked = 0;
            const long long bad = ring_walk(k, c, &checked);
            printf("%s[%d, %lld, %lld, %lld]", first ? "" : ", ", what, c, checked, bad);
            first = false;
        }
    }
    printf("]}\n");
    return 0;
}
