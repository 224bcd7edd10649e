// agc.hip -- GNU Radio's feedforward_agc_cc on channel IQ rings (gfx950): the AGC of the P25 CQPSK front half
// (p25_control_demod.py:149, logging_receiver.py:281), every AGC stage of a block (or of a group's block) in one launch.
//
//   env(z)  = float(|re| > |im| ? (double)|re| + 0.4 (double)|im| : (double)|im| + 0.4 (double)|re|)
//   M[n]    = max(1e-4f, max_{m = n-N+1 .. n} env(x[m]))
//   out[n]  = (R / M[n]) * x[n - N + 1]                      (x[m] = 0 before the stage's first input)
//
// One workgroup per (item, tile of up to kTile outputs).  It stages env() of the tile's inputs and their N - 1 look-back
// samples in LDS (coalesced 8-byte reads of the ring) and takes the window maximum from a doubling table: after pass j,
// S[i] = max env[i .. i + 2^j), and with 2^k <= N < 2^(k+1) the window maximum is max(S_k[i], S_k[i + N - 2^k]) -- at most
// 12 LDS passes instead of N compares per output.  A maximum is exact in any order and every rounding below is spelled
// out (no contraction), so the outputs are the bits of GNU Radio's naive loop restated in float.
#include "rcf_internal.h"

namespace rcfx {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;   // outputs per workgroup

__device__ __forceinline__ float agc_envelope(float2 z)
{
#pragma clang fp contract(off)
    const double r = fabs((double)z.x), i = fabs((double)z.y);
    return (float)(r > i ? __dadd_rn(r, __dmul_rn(0.4, i)) : __dadd_rn(i, __dmul_rn(0.4, r)));
}

// dynamic LDS: two tables of (tile + N_max - 1) floats (ping-pong between the doubling passes)
__global__ __launch_bounds__(kThreads) void agc_kernel(const AgcLaunch *__restrict__ items, int span, uint64_t ring_mask)
{
    extern __shared__ float lds[];
    const AgcLaunch it = items[blockIdx.x];
    const int j0 = (int)blockIdx.y * kTile;
    if (j0 >= it.n_k) return;
    const int cnt = min(kTile, it.n_k - j0);
    const int N = it.nsamples;
    const int L = cnt + N - 1;                      // staged inputs: x[m0 .. m0 + L)
    const int64_t m0 = it.n_lo + j0 - (N - 1);
    float *s = lds, *d = lds + span;
    for (int t = threadIdx.x; t < L; t += kThreads) {
        const int64_t m = m0 + t;
        s[t] = m >= it.n_first ? agc_envelope(it.iq_ring[(uint64_t)m & ring_mask]) : 0.f;
    }
    __syncthreads();
    int k = 0;
    while ((2 << k) <= N) ++k;                      // 2^k <= N < 2^(k+1)
    for (int j = 0; j < k; ++j) {
        const int w = 1 << j;
        const int valid = L - 2 * w + 1;            // S_{j+1}[i], i < valid, needs S_j up to i + w
        for (int t = threadIdx.x; t < valid; t += kThreads) d[t] = fmaxf(s[t], s[t + w]);
        __syncthreads();
        float *tmp = s; s = d; d = tmp;
    }
    const int off = N - (1 << k);
    for (int t = threadIdx.x; t < cnt; t += kThreads) {
        const float M = fmaxf(1e-4f, fmaxf(s[t], s[t + off]));
        const float g = __fdiv_rn(it.reference, M);
        const int64_t m = m0 + t;
        const float2 x = m >= it.n_first ? it.iq_ring[(uint64_t)m & ring_mask] : make_float2(0.f, 0.f);
        it.agc_ring[(uint64_t)(m + N - 1) & ring_mask] = make_float2(__fmul_rn(x.x, g), __fmul_rn(x.y, g));
    }
}

}  // namespace

void launch_agc(const AgcLaunch *d_items, int n_items, int max_n_k, int max_nsamples, uint64_t ring_mask, hipStream_t s)
{
    if (n_items <= 0 || max_n_k <= 0 || max_nsamples < 1) return;
    const int span = (max_n_k < kTile ? max_n_k : kTile) + max_nsamples - 1;
    hipLaunchKernelGGL(agc_kernel, dim3(n_items, (max_n_k + kTile - 1) / kTile), dim3(kThreads),
                       2 * sizeof(float) * (size_t)span, s, d_items, span, ring_mask);
}

}  // namespace rcfx
