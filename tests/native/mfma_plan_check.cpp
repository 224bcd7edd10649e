// mfma_plan_check -- g++ only.  Prints what the matrix-core planner of radiocapture-rf_amd/csrc/rcf_internal.h answers for the
// triples "n_chans n_k T" on stdin, one line each:  n_chans n_k T bank2_steps nt parts applicable
// (applicable: mfma2_applicable at D = 1 with the handle's default history and block capacities).
// tests/test_fir_census_cpu.py holds the Python restatement in tests/fir_census_ref.py to it.
#include <cstdio>

#include "rcf_internal.h"

using namespace rcfx;

int main()
{
    int n_chans, n_k, T;
    long long lines = 0;
    while (scanf("%d %d %d", &n_chans, &n_k, &T) == 3) {
        if (n_chans < 1 || n_k < 1 || T < 1) { fprintf(stderr, "bad triple %d %d %d\n", n_chans, n_k, T); return 2; }
        const MfmaPlan p = mfma_plan(n_chans, n_k, T);
        const size_t hist = size_t(1) << 16, block = size_t(1) << 22;
        printf("%d %d %d %d %d %d %d\n", n_chans, n_k, T, bank2_steps(T), p.nt, p.parts,
               (int)mfma2_applicable(1, T, hist, hist + block));
        ++lines;
    }
    fprintf(stderr, "%lld triples\n", lines);
    return 0;
}
