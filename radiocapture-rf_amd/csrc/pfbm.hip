// pfbm.hip -- mixed-radix polyphase filterbank for the bin counts the reference's own source rates give on the 12.5 kHz
// raster: NB = R1 * R2 in {160, 192, 480, 640, 960, 1280} (2, 2.4, 6, 8, 12, 16 Msps), D = NB / 2, up to 2 taps per branch.
//
// Bin k IS the reference's channel at offset k fs / NB (rc_frontend/channel.py:31-33: D = int(fs / cr) / 2,
// T = odd(int(fs / 6875)) ~ 1.82 NB), exactly as in pfb5.hip, whose frame-major contract (PfbLaunch) this kernel honours:
//
//   out_k[n] = e^{-j 2 pi k n D / NB} * sum_{rho<NB} e^{+j 2 pi k rho / NB} * u_rho[n]        (bin phase = (-1)^{k n})
//   u_rho[n] = sum_{q<P} h[NB q + rho] * x[n D - rho - NB q]
//
// Mapping: workgroup = F R2 threads, one chunk of F frames (16 for 160 / 192 bins, 8 for 480 / 640, 4 for 960 / 1280:
// 3 to 5.4 K complex of LDS, three workgroups and more per CU); four workgroup barriers per chunk.
//   NB-point inverse-sign DFT = R1 x R2 Stockham (Ns = 1, R1) with both butterflies in registers (fft_core.hpp):
//     160 = 10 x 16   192 = 12 x 16   480 = 20 x 24   640 = 20 x 32   960 = 24 x 40   1280 = 32 x 40
//     (10 = 5 x 2, 12 = 3 x 4, 20 = 5 x 4, 24 = 3 x 8, 40 = 5 x 8 as Good-Thomas prime-factor butterflies: no twiddles inside)
//   * the chunk's input window ((F + 3) D samples: every sample is used by OS P = 4 (frame, branch) pairs of different
//     threads) is staged in the LDS the frame rows take later, coalesced loads through a buffer descriptor (anything
//     outside the wideband buffer reads as zero); the zero-history instantiation zeroes what lies before start_sample here
//     and nowhere else, so both instantiations run the same arithmetic on the same window.
//   * phase A, thread = (frame, j < R2): the branch FIR for the R1 inputs rho = j + R2 t of first-pass butterfly j out of
//     the window (consecutive lanes = consecutive samples), the radix-R1 butterfly, results to LDS at R1 j + f -- rows
//     padded by one complex per R1: the stride-R1 writes of consecutive lanes fall in distinct banks (R1 + 1 is odd).
//   * phase B, thread = (frame, k < R1): second-pass butterfly k reads positions k + R1 t, twiddles W_NB^{k t} (one exact
//     table entry, the other powers by binary powering), and yields bins k + R1 f -- the SAME positions.  With two passes
//     the second one is in place thread by thread: no hazard, no ordering to arrange.
//   * taps first, copy-out last, both as in pfb5.hip: slots from tap_first on into the launch's tap matrix, then whole
//     frames as contiguous rows of bins_ring[(n & mask) NB + k], streamed (non-temporal) -- every NB here is a multiple
//     of 16, a row is whole 128-byte lines.
// Bound: HBM by its bytes (8 + 16 per input sample).  Measured on 2^22-sample blocks, input resident
// (profiles/pfbm_banks.json): 0.36 (960 bins) to 0.62 (192 bins) of 8 TB/s beside 0.48 for pfb5.hip's 400-bin bank in the
// same run; 16 to 47 times faster than the NB - 1 direct channels that give the same outputs.  These rates need real-time
// factors in the thousands at most, and nothing was spent on the last of it (no direct-to-LDS window DMA, prototype rows
// from L2).
// No rider and no fused discriminator (PfbShape::takes_rider and ::fused are false for this family).
// Build: pfb5.hip's flags -- no SLP vectoriser, no implicit contraction, the FMAs spelled out (RCF_EXPLICIT_FMA): the
// single, grouped and zero-history instantiations round alike.
#define RCF_EXPLICIT_FMA 1
#include "fft_core.hpp"
#include <hip/hip_ext.h>
#include "rcf_internal.h"

namespace rcfx {

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kStoreAuxM = 2;          // non-temporal
constexpr int kP = kPfbmP;              // taps per branch the kernel reads (PfbShape::Ppad): what the channel rule gives at OS = 2
// (frames per chunk: pfbm_frames, pfb_shape.h)
// padded extent of one frame in LDS (one spare complex after every R1): odd, so the copy-out's and the taps' column walks
// (stride = one row) spread over the banks as well
constexpr int pfbm_row_stride(int R1, int R2) { return R1 * R2 + R2 - 1; }
constexpr int pfbm_win(int NB, int F) { return (F - 1 + 2 * (kP - 1)) * (NB / 2) + NB; }
constexpr int pfbm_buf(int R1, int R2)
{
    const int NB = R1 * R2, F = pfbm_frames(NB);
    const int rows = F * pfbm_row_stride(R1, R2), win = pfbm_win(NB, F);
    return rows > win ? rows : win;
}

// one chunk of one front-end's bank (shared by the single-front-end kernel and the grouped one: same instructions, same bits)
template <int R1, int R2, bool ZH>
__device__ __forceinline__ void pfbm_chunk(const PfbLaunch &p, const int wg, const int tid, cf *buf)
{
    constexpr int NB = R1 * R2, OS = 2, D = NB / OS;
    constexpr int F = pfbm_frames(NB);
    constexpr int TPB = F * R2;
    constexpr int RS = pfbm_row_stride(R1, R2);
    constexpr int WIN = pfbm_win(NB, F);
    static_assert(R2 >= R1 && R1 % 2 == 0, "phase B fits the workgroup; R1 + 1 odd");
    static_assert((size_t)pfbm_buf(R1, R2) * sizeof(cf) <= 42 * 1280, "three workgroups per CU need <= 42 LDS granules each");
    const int fb0 = wg * F;
    if (fb0 >= p.n_frames) return;
    const int nf = min(F, p.n_frames - fb0);
    const int64_t n0 = p.n_lo + fb0;

    // ---- the window: x[m_lo + i], i < WIN
    {
        const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<cf *>(p.src.base), 0, (int)(p.src_len * (int64_t)sizeof(cf)), 0x00020000);
        const int64_t m_lo = (n0 - OS * (kP - 1)) * D - (NB - 1);
        constexpr int NLD = (WIN + TPB - 1) / TPB;
        // (a sample before the buffer's base gives a negative offset = an unsigned one beyond the descriptor's range: zero)
        const int vo0 = (int)((m_lo + tid - p.src.origin) * (int64_t)sizeof(cf));
        cf xs[NLD];
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(in_rsrc, vo0 + r * TPB * (int)sizeof(cf), 0, 0);
            xs[r] = make_float2(__uint_as_float(w.x), __uint_as_float(w.y));
        }
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int idx = tid + r * TPB;
            if (ZH && m_lo + idx < p.start_sample) xs[r] = make_float2(0.f, 0.f);
            if (NLD * TPB == WIN || idx < WIN) buf[idx] = xs[r];
        }
    }
    // ---- phase A: branch FIR + first radix-R1 pass.  u[t] = sum_q h[NB q + rho_t] x[(n - OS q) D - rho_t],
    // rho_t = j + R2 t; X[f] -> buf[R1 j + f] (padded)
    {
        const int frame = tid / R2, j = tid % R2;
        float h[kP][R1];
#pragma unroll
        for (int q = 0; q < kP; ++q)
#pragma unroll
            for (int t = 0; t < R1; ++t) h[q][t] = p.ptaps[q * NB + j + R2 * t];
        __syncthreads();
        cf vv[R1];
#pragma unroll
        for (int t = 0; t < R1; ++t) vv[t] = make_float2(0.f, 0.f);
        // x[(n - OS q) D - j - R2 t] = window[(frame + OS (kP - 1 - q)) D + NB - 1 - j - R2 t]
        const cf *sb = buf + frame * D + R2 - 1 - j;                       // q = kP - 1, t = R1 - 1
#pragma unroll
        for (int q = 0; q < kP; ++q) {
            cf x[R1];
#pragma unroll
            for (int t = 0; t < R1; ++t) x[t] = sb[OS * (kP - 1 - q) * D + R2 * (R1 - 1 - t)];
#pragma unroll
            for (int t = 0; t < R1; ++t) {
                vv[t].x = fmaf(h[q][t], x[t].x, vv[t].x);
                vv[t].y = fmaf(h[q][t], x[t].y, vv[t].y);
            }
        }
        __syncthreads();                                 // every thread has read the window before it is overwritten
        Dft<R1, +1>::run(vv);
        cf *o = buf + frame * RS + j * (R1 + 1);         // padded (R1 j + f) = (R1 + 1) j + f for f < R1
#pragma unroll
        for (int f = 0; f < R1; ++f) o[f] = vv[Dft<R1, +1>::reg_of(f)];
    }
    __syncthreads();
    // ---- phase B: second pass (Ns = R1), in place: butterfly k reads positions k + R1 t and leaves bin k + R1 f at
    // position k + R1 f, with the bin phase factor (-1)^{bin n} (R1 is even: the bin's parity is k's)
    if (tid < F * R1) {
        const int frame = tid / R1, k = tid % R1;
        cf *pos = buf + frame * RS + k;                  // padded (k + R1 t) = k + (R1 + 1) t for k < R1
        cf vv[R2];
#pragma unroll
        for (int t = 0; t < R2; ++t) vv[t] = pos[t * (R1 + 1)];
        {
            cf w[R2];
            twiddle_powers<R2>(p.tw[k], w);              // W_NB^{k t} from one table entry
#pragma unroll
            for (int t = 1; t < R2; ++t) vv[t] = cmul(vv[t], w[t]);
        }
        Dft<R2, +1>::run(vv);
        const bool neg = (((n0 + frame) & 1) != 0) && ((k & 1) != 0);
#pragma unroll
        for (int f = 0; f < R2; ++f) {
            const cf z = vv[Dft<R2, +1>::reg_of(f)];
            pos[f * (R1 + 1)] = neg ? make_float2(-z.x, -z.y) : z;
        }
    }
    __syncthreads();
    // ---- taps: bins that are open as channels go into the launch's compact tap matrix, tap_mat[(frame - n_lo) tap_pitch +
    // slot - tap_first] (lanes = consecutive slots); slots below tap_first are whole aligned runs of 16 bins, which
    // tap_finalize reads from the ring
    const int n_mat = p.n_taps - p.tap_first;
    if (n_mat > 0) {
        float2 *trow = p.tap_mat + (size_t)fb0 * p.tap_pitch;
        for (int sl = tid; sl < n_mat; sl += TPB) {
            const int bin = p.tap_bins[p.tap_first + sl];
            const cf *col = buf + bin + bin / R1;
#pragma unroll
            for (int f = 0; f < F; ++f)
                if (f < nf) trow[(size_t)f * p.tap_pitch + sl] = col[f * RS];
        }
    }
    // ---- copy-out: whole frames, bins consecutive across lanes -- every wavefront store is 512 contiguous bytes of
    // the frame-major ring bins_ring[(n & mask) NB + k]; one descriptor per frame row (the ring has no 2 GiB limit)
#pragma unroll
    for (int f = 0; f < F; ++f) {
        if (f >= nf) break;
        const int64_t slot = (int64_t)((uint64_t)(n0 + f - p.n_abs0) & p.ring_mask);
        const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            p.bins_ring + slot * NB, 0, NB * (int)sizeof(cf), 0x00020000);
        const cf *row = buf + f * RS;
#pragma unroll
        for (int bb = 0; bb < (NB + TPB - 1) / TPB; ++bb) {
            const int bin = tid + bb * TPB;
            if (NB % TPB != 0 && bin >= NB) break;
            const cf z = row[bin + bin / R1];
            u32x2 o;
            o.x = __float_as_uint(z.x);
            o.y = __float_as_uint(z.y);
            __builtin_amdgcn_raw_buffer_store_b64(o, out_rsrc, bin * (int)sizeof(cf), 0, kStoreAuxM);
        }
    }
}

template <int R1, int R2, bool ZH>
__global__ __launch_bounds__(pfbm_frames(R1 * R2) * R2) void pfbm_kernel(PfbLaunch p, int n_wg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf *buf = reinterpret_cast<cf *>(smem_raw);
    // neighbouring chunks (they share input rows) on one XCD
    const int b = blockIdx.x;
    const int wg = xcd_chunk_first(n_wg, b) + b / 8;
    pfbm_chunk<R1, R2, ZH>(p, wg, threadIdx.x, buf);
}

// The banks of G front-ends in ONE launch (rcf_group.cpp): steady state only.  Ten 2.4 Msps sources with 20 ms blocks are
// 32 chunks each -- one launch of 320 instead of ten that fill an eighth of the device
template <int R1, int R2>
__global__ __launch_bounds__(pfbm_frames(R1 * R2) * R2) void pfbm_group_kernel(const PfbLaunch *__restrict__ pls, GroupMap gm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf *buf = reinterpret_cast<cf *>(smem_raw);
    int fe, wg;
    group_resolve(gm, blockIdx.x, fe, wg);
    const PfbLaunch p = pls[fe];
    pfbm_chunk<R1, R2, false>(p, wg, threadIdx.x, buf);
}

template <int R1, int R2>
void launchm(const PfbLaunch &p, bool zh, hipStream_t s)
{
    constexpr int NB = R1 * R2, F = pfbm_frames(NB), TPB = F * R2;
    const int n_wg = (p.n_frames + F - 1) / F;
    const size_t lds = (size_t)pfbm_buf(R1, R2) * sizeof(cf);
    if (zh) RCF_PFB_LAUNCH(p, (pfbm_kernel<R1, R2, true>), dim3(n_wg), dim3(TPB), lds, s, p, n_wg);
    else    RCF_PFB_LAUNCH(p, (pfbm_kernel<R1, R2, false>), dim3(n_wg), dim3(TPB), lds, s, p, n_wg);
}

template <int R1, int R2>
void launchm_group(const PfbLaunch *d_pls, const GroupMap &gm, hipStream_t s)
{
    constexpr int NB = R1 * R2, F = pfbm_frames(NB), TPB = F * R2;
    const size_t lds = (size_t)pfbm_buf(R1, R2) * sizeof(cf);
    hipLaunchKernelGGL((pfbm_group_kernel<R1, R2>), dim3(gm.total_wg), dim3(TPB), lds, s, d_pls, gm);
}

}  // namespace

// sh: a family-3 shape (pfb_shape.h)
void pfbm_launch(const PfbShape &sh, const PfbLaunch &p, bool zh, hipStream_t s)
{
#define RCF_X(R1_, R2_) \
    if (sh.NB == R1_ * R2_) return launchm<R1_, R2_>(p, zh, s);
    RCF_PFBM_SHAPES(RCF_X)
#undef RCF_X
}

void pfbm_launch_group(const PfbShape &sh, const PfbLaunch *d_pls, const GroupMap &gm, hipStream_t s)
{
#define RCF_X(R1_, R2_) \
    if (sh.NB == R1_ * R2_) return launchm_group<R1_, R2_>(d_pls, gm, s);
    RCF_PFBM_SHAPES(RCF_X)
#undef RCF_X
}

}  // namespace rcfx
