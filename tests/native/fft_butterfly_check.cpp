// The register butterflies of radiocapture-rf_amd/csrc/fft_core.hpp compiled for the host (RCF_FFT_CORE_HOST) and held
// against a double-precision naive DFT: the radix-3 and radix-32 butterflies and the prime-factor composites the
// mixed-radix filterbank (pfbm.hip) is built on, next to the ones the other banks already use.
// Prints "R <radix> relerr <max relative rms error over the trials>" per radix; tests/test_pfbm_host.py reads it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
struct float2 { float x, y; };
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
#define __device__
#define __host__
#define __forceinline__ inline
#define RCF_FFT_CORE_HOST 1
#define RCF_EXPLICIT_FMA 1
#include "fft_core.hpp"

using namespace rcfx;

template <int R, int SIGN>
static double check()
{
    double worst = 0.0;
    for (int trial = 0; trial < R + 8; ++trial) {
        cf v[R];
        double xr[R], xi[R];
        for (int n = 0; n < R; ++n) {
            // trial < R: unit impulses (every input position on its own); then noise
            float a = trial < R ? (n == trial ? 1.f : 0.f) : (float)(rand() / (double)RAND_MAX - 0.5);
            float b = trial < R ? 0.f : (float)(rand() / (double)RAND_MAX - 0.5);
            v[n] = make_float2(a, b);
            xr[n] = a; xi[n] = b;
        }
        Dft<R, SIGN>::run(v);
        double num = 0.0, den = 0.0;
        for (int f = 0; f < R; ++f) {
            double sr = 0.0, si = 0.0;
            for (int n = 0; n < R; ++n) {
                const double ang = SIGN * 2.0 * M_PI * (double)((f * n) % R) / R;
                sr += xr[n] * std::cos(ang) - xi[n] * std::sin(ang);
                si += xr[n] * std::sin(ang) + xi[n] * std::cos(ang);
            }
            const cf g = v[Dft<R, SIGN>::reg_of(f)];
            num += (g.x - sr) * (g.x - sr) + (g.y - si) * (g.y - si);
            den += sr * sr + si * si;
        }
        const double e = std::sqrt(num / den);
        if (e > worst) worst = e;
    }
    std::printf("R %d sign %d relerr %.3e\n", R, SIGN, worst);
    return worst;
}

int main()
{
    srand(12345);
    check<3, +1>();  check<3, -1>();
    check<5, +1>();
    check<8, +1>();
    check<10, +1>(); check<10, -1>();
    check<12, +1>(); check<12, -1>();
    check<16, +1>();
    check<20, +1>();
    check<24, +1>(); check<24, -1>();
    check<32, +1>(); check<32, -1>();
    check<40, +1>(); check<40, -1>();
    return 0;
}
