// pfb_shape_check -- g++ only.  Prints what the filterbank shape table (radiocapture-rf_amd/csrc/pfb_shape.h) answers over
// the grid of tests/golden/pfb_shapes.json, one JSON row per (bins, decimation, prototype length), and holds
// pfb_zero_history to the predicate written out for every supported shape of the grid (tests/test_pfb_shape_table.py).
#include <cstdio>

#include "pfb_shape.h"

using namespace rcfx;

int main()
{
    const int NBs[] = {25, 32, 64, 128, 160, 192, 200, 228, 256, 400, 480, 512, 640, 800, 960, 1024, 1280, 1600, 2048, 3200, 6400};
    const int divs[] = {1, 2, 3, 4, 8};
    long long zh_checked = 0, zh_bad = 0;
    printf("{\"rows\": [\n");
    bool first = true;
    for (int NB : NBs)
        for (int dv : divs) {
            if (NB % dv) continue;
            const int D = NB / dv;
            for (int Pq = 1; Pq <= 17; ++Pq)
                for (int form = 0; form < 2; ++form) {
                    const int ntaps = form == 0 ? Pq * NB : (Pq - 1) * NB + 1;
                    const PfbShape s = pfb_shape(NB, D, (ntaps + NB - 1) / NB);
                    printf("%s[%d, %d, %d, %d, %d, %d, %d, %d, %d, %zu, %d, %d, %d, %d]", first ? "" : ",\n", NB, D, ntaps,
                           s.family ? 1 : 0, s.family, s.Ppad, s.chunk_frames, (int)s.frame_major, (int)s.fused, s.fused_history,
                           (int)s.takes_rider, (int)s.carries_s2, (int)s.grouped, (int)s.grouped_fused);
                    first = false;
                    if (!s.family) {
                        if (s.NB || s.D || s.OS || s.P) ++zh_bad;             // (no kernel: every field zero)
                        continue;
                    }
                    if (s.NB != NB || s.D != D || s.OS != dv || s.P != (ntaps + NB - 1) / NB) ++zh_bad;
                    // three start samples: 0, one that is no multiple of D, one a few frames in and a multiple of D
                    const long long starts[3] = {0, (long long)D + D / 3 + 1, 5LL * D};
                    const int halos[2] = {0, s.chunk_frames};
                    for (long long start : starts)
                        for (int halo : halos)
                            for (long long n_lo = -2; n_lo <= 40; ++n_lo) {
                                const long long first_sample = (n_lo - halo - (long long)dv * (s.Ppad - 1)) * D - (NB - 1);
                                ++zh_checked;
                                if (pfb_zero_history(s, n_lo, start, halo) != (first_sample < start)) ++zh_bad;
                            }
                }
        }
    printf("\n],\n \"zero_history_checked\": %lld, \"zero_history_mismatches\": %lld}\n", zh_checked, zh_bad);
    return zh_bad ? 1 : 0;
}
