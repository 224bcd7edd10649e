// squelch_core.hpp -- the arithmetic of the carrier detector (squelch.hip; definition: include/rcf.h at rcf_chan_squelch):
// GNU Radio's simple_squelch_cc -- float |x|^2 into single_pole_iir<double,double,double>, open while level >= thr -- as one
// step, as a sequential walk with its counters, and cut in time: a segment's zero-state response and the carry that takes a
// level across a segment (the recurrence is linear, so the cut is exact up to rounding).  No HIP types in here, like
// slice_core.hpp: RCF_DEVFN is the function qualifier, so that the CPU suite compiles this very source with g++
// (tests/native/squelch_core_check.cpp).  Whoever includes it compiles without floating-point contraction
// (-ffp-contract=off): the unfused products and sums below are the definition.
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef RCF_DEVFN
#define RCF_DEVFN __device__ __forceinline__
#endif

namespace rcfx {

namespace {

constexpr int kSquelchSegment = 256;     // frames per segment of the bank's detector (rcf_pfb_squelch_segment)

// simple_squelch_cc::set_threshold, on the host (the attach calls: the kernels take thr as it is)
static inline double squelch_threshold(double threshold_db) { return pow(10.0, threshold_db / 10); }
// what takes a level across a whole segment of s samples: (1 - alpha)^s, one pow() of the host as well
static inline double squelch_a_pow_s(double alpha, int s) { return pow(1.0 - alpha, (double)s); }

// float products, float sum (complex_to_mag_squared), widened by the caller
RCF_DEVFN float squelch_power(float re, float im) { return re * re + im * im; }

// single_pole_iir::filter: alpha * input + (1 - alpha) * previous, in double
RCF_DEVFN double squelch_step(double level, double alpha, double one_minus_alpha, float p)
{
    return alpha * (double)p + one_minus_alpha * level;
}

// open while level >= thr: a NaN level is muted
RCF_DEVFN bool squelch_is_open(double level, double thr) { return level >= thr; }

// what a walk keeps beside the level; indices are the caller's (channel samples, bank frames)
struct SquelchWalk {
    double level;
    int64_t n_open, first_open, last_open;       // -1: none
    int32_t unmuted;
};

// one sample at index i
RCF_DEVFN void squelch_walk_step(SquelchWalk &w, double alpha, double one_minus_alpha, double thr, float re, float im, int64_t i)
{
    w.level = squelch_step(w.level, alpha, one_minus_alpha, squelch_power(re, im));
    const bool open = squelch_is_open(w.level, thr);
    w.unmuted = open ? 1 : 0;
    w.n_open += open ? 1 : 0;
    w.first_open = open && w.first_open < 0 ? i : w.first_open;
    w.last_open = open ? i : w.last_open;
}

// ---- the recurrence cut into segments of S samples.  With a = 1 - alpha, the level behind a segment that was entered at e is
// z + a^S e, z being the level the segment gives from 0 (its zero-state response).  a^S is one pow() of the host.
// An infinite level stays infinite in the sequential form while a > 0; a^S may have underflowed to 0 by then, and 0 x Inf
// would make it a NaN: the carry keeps the infinity (a == 0 -- alpha 1 -- makes the NaN in the sequential form as well)
RCF_DEVFN double squelch_carry(double entry, double a_pow_s, double one_minus_alpha)
{
    const bool inf = entry - entry != 0.0 && entry == entry;      // +-Inf (a NaN fails the second test)
    return inf && one_minus_alpha > 0.0 ? entry : a_pow_s * entry;
}

// the level a later segment is entered at: z of the segment before it plus the carry of that segment's own entry level
RCF_DEVFN double squelch_enter(double z_before, double entry_before, double a_pow_s, double one_minus_alpha)
{
    return z_before + squelch_carry(entry_before, a_pow_s, one_minus_alpha);
}

}  // namespace

}  // namespace rcfx
