// capture_core.hpp -- the per-sample step of the carrier-operated capture (capture.hip; definition: include/rcf.h at
// rcf_chan_capture): the carrier detector's step (squelch_core.hpp), the writer's decision `pre` samples behind it, the
// OPEN / CLOSE events and the two accumulators a CLOSE record reports.  No HIP types in here, like squelch_core.hpp:
// RCF_DEVFN is the function qualifier, so that the CPU suite compiles this very source with g++
// (tests/native/capture_core_check.cpp).  Whoever includes it compiles without floating-point contraction
// (-ffp-contract=off): the detector's unfused products and sums are the definition.
#pragma once
#include "squelch_core.hpp"

namespace rcfx {

namespace {

constexpr uint32_t kCaptureOpen = 1, kCaptureClose = 2;     // rcf_capture_rec_t::kind
constexpr int kCaptureRecWords = 8;                         // 4-byte words per record

// What the stage carries from sample to sample.  Indices count the channel's outputs; -1: none.
struct CaptureWalk {
    double level;            // the detector's filter output after the last sample seen
    int64_t last_open;       // L(n): the greatest open index the detector has seen
    int64_t n_kept;          // samples written to the captured stream
    int64_t n_records;       // records written
    int64_t n_windows;       // OPEN records among them
    int64_t acc_open;        // open samples the detector has seen since the last CLOSE
    double acc_peak;         // the largest level at one of them (0: none)
    int32_t in_window;       // the last decided sample was kept
    int32_t unmuted;         // the last sample seen was open
};

// The record of an event, as the ring holds it (rcf_capture_rec_t)
struct CaptureRec {
    uint32_t kind, n_open;
    int64_t sample, pos;
    float peak;
    uint32_t reserved_;
};

// The detector's step at index j on power p = squelch_power(re, im): simple_squelch_cc's, and what a CLOSE will report
RCF_DEVFN void capture_detect(CaptureWalk &w, double alpha, double one_minus_alpha, double thr, float p, int64_t j)
{
    w.level = squelch_step(w.level, alpha, one_minus_alpha, p);
    const bool open = squelch_is_open(w.level, thr);
    w.unmuted = open ? 1 : 0;
    w.last_open = open ? j : w.last_open;
    w.acc_open += open ? 1 : 0;
    w.acc_peak = open && w.level > w.acc_peak ? w.level : w.acc_peak;
}

// The writer's step at index s = j - pre >= a, behind capture_detect(j): keep(s) <=> L(s + pre) >= s - hang, and L(s + pre)
// is w.last_open.  Returns whether s is kept; *ev: 0, or the record of the event at s (the caller stores it at record
// n_records - 1 and, when s is kept, the sample at item n_kept - 1: both counters have advanced on return).
// The accumulators reset at a CLOSE, which is exact: keep(s) is false there, so no index in [s - hang, s + pre] is open --
// every open sample the detector has seen lies before s - hang, inside a window that has ended at s, and those of the
// windows before this one were taken out by their own CLOSE.
RCF_DEVFN bool capture_write(CaptureWalk &w, int64_t hang, int64_t s, CaptureRec *ev)
{
    const bool keep = w.last_open >= 0 && w.last_open >= s - hang;
    ev->kind = 0;
    if (keep && !w.in_window) {
        *ev = CaptureRec{kCaptureOpen, 0u, s, w.n_kept, 0.0f, 0u};
        w.n_windows += 1;
        w.n_records += 1;
    } else if (!keep && w.in_window) {
        const uint32_t n_open = w.acc_open > 0xffffffffll ? 0xffffffffu : (uint32_t)w.acc_open;      // (saturates)
        *ev = CaptureRec{kCaptureClose, n_open, s, w.n_kept, (float)w.acc_peak, 0u};
        w.acc_open = 0;
        w.acc_peak = 0.0;
        w.n_records += 1;
    }
    w.in_window = keep ? 1 : 0;
    w.n_kept += keep ? 1 : 0;
    return keep;
}

}  // namespace

}  // namespace rcfx
