// stream_table_check -- g++ only.  Prints what the stream table (radiocapture-rf_amd/csrc/rcf_streams.h) answers for every
// `what` in 0 .. 40 -- the row, or null for a refusal -- and the readers' integer rules over a small grid, as JSON
// (tests/test_stream_table.py holds both against values written out there and against tests/delivery_ref.py).
#include <cstdio>
#include <initializer_list>

#include "rcf_streams.h"

using namespace rcfx;

int main()
{
    printf("{\"rows\": [");
    for (int what = 0; what <= 40; ++what) {
        const int k = stream_kind(what);
        if (k < 0) { printf("%snull", what ? ", " : ""); continue; }
        const StreamKind &r = kStreams[k];
        printf("%s\n {\"what\": %d, \"kind\": %d, \"item_bytes\": %u, \"u32\": %d, \"counted\": %d, \"pumped\": %d, \"refusal\": \"%s\"}",
               what ? "," : "", r.what, k, r.item_w * 4u, (int)r.u32, (int)r.counted, (int)r.pumped, r.refusal);
    }
    const long long counters[] = {0, 1, 24, 25, 26, 999, 12345}, n_ks[] = {0, 1, 37, 500, 1200};
    const unsigned rs[][2] = {{1, 1}, {8, 25}, {48, 25}, {441, 1000}};
    printf("],\n \"count_end\": [");             // [counter, interp, decim, end]
    bool first = true;
    for (long long c : counters)
        for (auto &r : rs) { printf("%s[%lld, %u, %u, %lld]", first ? "" : ", ", c, r[0], r[1], (long long)count_end(c, r[0], r[1])); first = false; }
    printf("],\n \"steady_bound\": [");          // [n_k, interp, decim, bound]
    first = true;
    for (long long n : n_ks)
        for (auto &r : rs) { printf("%s[%lld, %u, %u, %lld]", first ? "" : ", ", n, r[0], r[1], (long long)steady_bound(n, r[0], r[1])); first = false; }
    // a reader at `cursor` of a stream that ends at `end` in a ring of `cap`, asked for at most `max`: [cap, cursor, end, max,
    // cursor after the clamp, items]; then what a host ring of `room` keeps of them: [cursor after, items]
    printf("],\n \"lag_clamp\": [");
    first = true;
    const long long caps[] = {16, 256}, maxes[] = {0, 7, 1000000}, rooms[] = {8, 64, 4096};
    for (long long cap : caps)
        for (long long end : counters)
            for (long long cursor : {0LL, 1LL, end - cap - 1, end - cap, end - cap + 1, end - 1, end, end + 3})
                for (long long max : maxes)
                    for (long long room : rooms) {
                        if (cursor < 0) continue;
                        int64_t cur = cursor;
                        const int64_t n = lag_clamp(cap, &cur, end, end, max);
                        int64_t cur2 = cur;
                        const int64_t n2 = ring_room(&cur2, n, room);
                        printf("%s[%lld, %lld, %lld, %lld, %lld, %lld, %lld, %lld, %lld]", first ? "" : ", ", cap, cursor, end, max,
                               (long long)cur, (long long)n, room, (long long)cur2, (long long)n2);
                        first = false;
                    }
    printf("]}\n");
    return 0;
}
