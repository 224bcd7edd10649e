// pfb_shape.h -- the shape table of the polyphase filterbanks: the ONLY place a (bins, decimation, taps per branch) shape
// is named.  Plain C++17, no HIP: the planner reads it (rcf_bank.cpp, rcf_plan.cpp, rcf_launch.cpp, rcf_group.cpp), the
// kernel files expand the same lists to instantiate and dispatch (pfb.hip, pfb5.hip, pfbm.hip), and
// tests/native/pfb_shape_check.cpp compiles it alone.  A shape is supported exactly when a row below names it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rcfx {

// family 1 -- power-of-two bin counts (pfb.hip): X(NB).  D = NB or NB / 2; the prototype's taps per branch run the next
// instantiated row count (pfb1_round_p).  16 frames per chunk, tiled ring.
#define RCF_PFB1_SHAPES(X) X(64) X(128) X(256) X(512) X(1024)
// family 2 -- 400 2^k bins (pfb5.hip): X(R, R3, OS, P, grouped, fused).  NB = R R R3, D = NB / OS, P rows of the polyphase
// table (a shorter prototype runs the next larger P of its (NB, OS)), 16 / R3 frames per chunk, frame-major ring.
// grouped: has pfb5_group_kernel; fused: has the fused-discriminator kernels, single and grouped -- the shapes the
// reference's channel rule produces (OS = 2: 12.5 kHz raster, OS = 4: 6.25 kHz).
#define RCF_PFB5_SHAPES(X)                                                                                   \
    X(20, 4, 2, 2, 1, 1) X(20, 4, 2, 1, 0, 0) X(20, 4, 1, 4, 0, 0) X(20, 4, 4, 1, 0, 0) /* 1600 bins */      \
    X(20, 8, 4, 1, 1, 1) X(20, 8, 2, 2, 1, 0) X(20, 8, 2, 1, 0, 0) X(20, 8, 1, 4, 0, 0) /* 3200 bins */      \
    X(20, 2, 2, 2, 1, 1) X(20, 2, 2, 1, 0, 0) X(20, 2, 1, 4, 0, 0) X(20, 2, 4, 1, 0, 0) /* 800 bins */       \
    X(20, 1, 2, 2, 1, 1) X(20, 1, 2, 1, 0, 0) X(20, 1, 1, 4, 0, 0) X(20, 1, 4, 1, 0, 0) /* 400 bins */
// family 3 -- mixed radix (pfbm.hip): X(R1, R2).  NB = R1 R2 = 160, 192, 480, 640, 960, 1280 at D = NB / 2 -- the reference's
// 2 / 2.4 / 6 / 8 / 12 / 16 Msps sources on the 12.5 kHz raster.  ONE instantiation per bin count, two taps per branch (what
// the channel rule gives; a shorter prototype runs with a row of zeros); frame-major, grouped, no fused discriminator.
#define RCF_PFBM_SHAPES(X) X(10, 16) X(12, 16) X(20, 24) X(20, 32) X(24, 40) X(32, 40)

// family 1: taps per branch the kernels are instantiated for.  14 is what the reference's own low_pass_2 rule with a
// Blackman-Harris window gives a critically sampled bank of ANY size (transition 0.2 bin, 60 dB -> 13.6 taps
// per branch), so that case gets its exact row count instead of 16.
constexpr int pfb1_round_p(int P, int OS)
{
    return P <= 4 ? 4 : (OS == 1 && P > 8 && P <= 14) ? 14 : P <= 16 ? 16 : 0;
}
// family 1: the form of the kernel is a function of the shape (pfb.hip: launch_os)
constexpr bool pfb1_two_branch(int NB, int OS) { return OS == 1 && NB >= 512; }
constexpr bool pfb1_persistent(int NB, int OS) { return OS != 1 && NB >= 512; }
constexpr int kPfb1ChunkFrames = 16;
constexpr int kPfbS2Bins = 256;         // the bank whose workgroups have the stage-2 tile's thread count (fir_small.hpp: kSmallThreads)
// family 3: frames per chunk
constexpr int pfbm_frames(int NB) { return NB <= 192 ? 16 : (NB <= 640 ? 8 : 4); }
constexpr int kPfbmP = 2;

struct PfbShape {
    int family = 0;              // 0: no kernel (every other field zero / false), 1 pfb.hip, 2 pfb5.hip, 3 pfbm.hip
    int NB = 0, D = 0, OS = 0;
    int P = 0, Ppad = 0;         // taps per branch of the prototype; rows of the polyphase table the kernel reads (zero padded)
    int chunk_frames = 0;        // frames per chunk (= per workgroup)
    bool frame_major = false;    // ring layout (PfbLaunch::frame_major); false: tiled
    bool grouped = false;        // has a grouped kernel (rcf_group.cpp) ...
    bool grouped_fused = false;  // ... and one with the discriminator fused in
    bool fused = false;          // has the fused-discriminator kernels (rcf_pfb_fm_enable)
    size_t fused_history = 0;    // fused: input samples the halo chunk of a launch's first workgroup reaches back over
    // takes the copy rider (PfbLaunch::rider_*): every tiled form but the persistent one -- its workgroups are ONE resident
    // round, and 64 of them starting late set the whole launch back by what the copy launch cost (cfg5: kernel +2.8 us,
    // step unchanged); the frame-major kernels measured +5.7 us on the 1600-bin launch for 4.7 saved
    bool takes_rider = false;
    bool carries_s2 = false;     // its steady-state kernel can carry a stage-2 rider (S2Rider): the 256-bin bank
};

inline PfbShape pfb_shape(int NB, int D, int P)
{
    PfbShape s{};
    if (NB < 1 || D < 1 || P < 1 || NB % D) return s;
    const int OS = NB / D;
    int family = 0, ppad = 0, chunk = 0;
    bool grouped = false, fused = false;
#define RCF_X(NB_)                                                                             \
    if (NB == NB_ && (OS == 1 || OS == 2) && pfb1_round_p(P, OS)) {                            \
        family = 1; ppad = pfb1_round_p(P, OS); chunk = kPfb1ChunkFrames;                      \
        grouped = !pfb1_persistent(NB_, OS);                                                   \
    }
    RCF_PFB1_SHAPES(RCF_X)
#undef RCF_X
#define RCF_X(R_, R3_, OS_, P_, G_, F_)                                                        \
    if (NB == R_ * R_ * R3_ && OS == OS_ && P <= P_ && (family != 2 || P_ < ppad)) {           \
        family = 2; ppad = P_; chunk = 16 / R3_; grouped = G_; fused = F_;                     \
    }
    RCF_PFB5_SHAPES(RCF_X)
#undef RCF_X
#define RCF_X(R1_, R2_)                                                                        \
    if (NB == R1_ * R2_ && OS == 2 && P <= kPfbmP) {                                           \
        family = 3; ppad = kPfbmP; chunk = pfbm_frames(R1_ * R2_); grouped = true;             \
    }
    RCF_PFBM_SHAPES(RCF_X)
#undef RCF_X
    if (!family) return s;
    s.family = family;
    s.NB = NB; s.D = D; s.OS = OS; s.P = P; s.Ppad = ppad;
    s.chunk_frames = chunk;
    s.frame_major = family != 1;
    s.grouped = grouped;
    s.grouped_fused = s.fused = fused;
    // chunk + OS (Ppad - 1) + 1 frames and the prototype's span
    if (fused) s.fused_history = (size_t)(chunk + OS * (ppad - 1) + 2) * (size_t)D + (size_t)NB;
    s.takes_rider = family == 1 && !pfb1_persistent(NB, OS);
    s.carries_s2 = family == 1 && NB == kPfbS2Bins;
    return s;
}

// Whether a launch whose first frame is n_lo still reaches samples before the bank's start: it then runs the masking
// (zero-history) instantiation, alone -- no grouped launch, no riders.  halo_frames: 0, or chunk_frames for the fused
// discriminator, whose first workgroups recompute the chunk BEFORE the launch's first frame.  The planner asks (plan_pfb),
// the launchers are told.
inline bool pfb_zero_history(const PfbShape &s, int64_t n_lo, int64_t start_sample, int halo_frames)
{
    return (n_lo - halo_frames - (int64_t)s.OS * (s.Ppad - 1)) * (int64_t)s.D - (s.NB - 1) < start_sample;
}

}  // namespace rcfx
