// rcf_bank.cpp -- C ABI of the polyphase filterbank and the scanner (fft_vector.py + fft_peak_detection.py).
#include "rcf_plan.h"
#define RCF_DEVFN static inline
#include "squelch_core.hpp"    // (squelch_threshold, squelch_a_pow_s)

namespace rcfx {

void pfb_release(rcf_t *h)
{
    Pfb &p = h->pfb;
    for (void *q : {(void *)p.d_ptaps, (void *)p.d_tw, (void *)p.d_bins, (void *)p.d_fm, (void *)p.d_fm_inc, (void *)p.d_fm_edge,
                    (void *)p.d_fm_flag, (void *)p.d_fm_err, (void *)p.sq.d_state, (void *)p.sq.d_z})
        bury(h, q);
    p = Pfb();
}

// The rotator increment's angle a discriminator-only channel on bin k of the bank carries (Chan::dangle of a tap opened
// with rcf_pfb_tap_open(bin, gr_phase): rcf_chan.cpp) -- for every bin at once, uploaded and turned into float32 phasors
// on the device (launch_pfb5_fm_inc: tap_finalize's own expression)
int pfb_fm_upload_increments(rcf_t *h)
{
    Pfb &p = h->pfb;
    std::vector<double> dangle((size_t)p.NB, 0.0);
    // what rcf_source_shift adds to every bin-fed channel's NCO (upload_composite: a D = 1, T = 1 channel at the bin rate)
    double shift_angle = 0.0;
    if (h->shift_hz != 0.0) {
        const float one = 1.0f;
        std::vector<float> ct;
        float incr[2];
        design_composite(&one, 1, 1, h->shift_hz, h->fs / p.D, ct, incr);
        shift_angle = std::atan2((double)incr[1], (double)incr[0]);
    }
    for (int bin = 0; bin < p.NB; ++bin) {
        double d = shift_angle;
        if (p.fm_gr_phase) d += pfb_tap_gr_dangle(h, bin);
        dangle[(size_t)bin] = d;
    }
    double *d_dangle = nullptr;
    RCF_HIP(hipMalloc(&d_dangle, sizeof(double) * dangle.size()));
    if (!hip_ok(hipMemcpyAsync(d_dangle, dangle.data(), sizeof(double) * dangle.size(), hipMemcpyHostToDevice, h->stream), "hipMemcpy(fm increments)")) {
        (void)hipFree(d_dangle);
        return RCF_EHIP;
    }
    launch_pfb5_fm_inc(d_dangle, p.d_fm_inc, p.NB, h->stream);
    RCF_HIP(hipStreamSynchronize(h->stream));          // (dangle is a local vector; the stream also orders the table before the next block)
    (void)hipFree(d_dangle);
    return RCF_OK;
}

bool pfb_fm_stream(rcf_t *h, int bin, int64_t *cursor, bool pump, Stream *s)
{
    const Pfb &p = h->pfb;
    if (!p.open || !p.d_fm || bin < 0 || bin >= p.NB) return false;
    const int64_t end = p.fm_mode ? p.produced : p.fm_until;      // while the discriminator is off, readers stop where it was switched off
    *s = Stream{h, p.d_fm + bin, 1u, (uint32_t)p.NB, (uint32_t)h->out_cap, cursor, end, pump ? end : p.produced};
    if (pump && cursor) *cursor = std::max(*cursor, p.fm_from);   // (switched off and on again: the frames between were never demodulated)
    return true;
}

}  // namespace rcfx

using namespace rcfx;

// =================================================================== C ABI
extern "C" {

// ------------------------------------------------------------------ PFB
int rcf_pfb_open(rcf_t *h, int n_bins, int decim, const float *taps, int ntaps)
{
    if (!h || !taps || ntaps < 1 || n_bins < 1 || decim < 1) { set_error("bad PFB arguments"); return RCF_EINVAL; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    if (h->pfb.open) { set_error("PFB already open"); return RCF_ESTATE; }
    const int P = (ntaps + n_bins - 1) / n_bins;
    const PfbShape sh = pfb_shape(n_bins, decim, P);
    if (!sh.family) {
        set_error("unsupported PFB shape: bins=%d decim=%d taps/branch=%d", n_bins, decim, P);
        return RCF_EINVAL;
    }
    const bool fm = sh.frame_major;
    if (!fm && h->out_cap < (size_t(1) << kPfbTileLog2)) { set_error("output capacity %zu < one ring tile", h->out_cap); return RCF_ECAP; }
    const size_t ring_samples = fm ? (size_t)n_bins * h->out_cap : (size_t)(h->out_cap >> kPfbTileLog2) * (size_t)pfb_tile_pitch(n_bins);
    // 32-bit buffer offsets: the wideband buffer, and the tiled ring of the power-of-two banks (one descriptor for the
    // whole ring).  The frame-major banks address their ring through one descriptor per frame row: no limit there.
    if ((!fm && (uint64_t)ring_samples * sizeof(float2) >= (1ull << 31)) ||
        (uint64_t)(h->hist_cap + h->block_cap) * sizeof(float2) >= (1ull << 31)) {
        set_error("PFB rings / wideband buffer exceed the 2 GiB range of 32-bit buffer offsets");
        return RCF_ECAP;
    }
    if ((size_t)P * n_bins + (size_t)decim > h->hist_cap) { set_error("history capacity %zu < P*bins", h->hist_cap); return RCF_ECAP; }
    Pfb &p = h->pfb;
    p.shape = sh;
    p.NB = n_bins; p.D = decim; p.T = ntaps; p.P = P;
    p.proto.assign(taps, taps + ntaps);
    std::vector<float> pt((size_t)sh.Ppad * n_bins, 0.f);
    for (int i = 0; i < ntaps; ++i) pt[i] = taps[i];          // pt[p*NB + rho] = h[NB p + rho]
    std::vector<float> tw(2 * (size_t)n_bins);
    for (int i = 0; i < n_bins; ++i) {
        const double a = kTwoPi * i / n_bins;
        tw[2 * i] = (float)std::cos(a);
        tw[2 * i + 1] = (float)std::sin(a);
    }
    RCF_HIP(hipMalloc(&p.d_ptaps, sizeof(float) * pt.size()));
    RCF_HIP(hipMemcpy(p.d_ptaps, pt.data(), sizeof(float) * pt.size(), hipMemcpyHostToDevice));
    RCF_HIP(hipMalloc(&p.d_tw, sizeof(float2) * (size_t)n_bins));
    RCF_HIP(hipMemcpy(p.d_tw, tw.data(), sizeof(float2) * (size_t)n_bins, hipMemcpyHostToDevice));
    RCF_HIP(hipMalloc(&p.d_bins, sizeof(float2) * ring_samples));
    RCF_HIP(hipMemsetAsync(p.d_bins, 0, sizeof(float2) * ring_samples, h->stream));
    p.rd.assign(n_bins, 0);
    p.start_sample = h->total_in;
    p.n_abs0 = ceil_div(p.start_sample, decim);
    p.produced = p.produced_before = 0;
    p.open = true;
    return RCF_OK;
}

int rcf_pfb_close(rcf_t *h)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Pfb &p = h->pfb;
    if (!p.open) return RCF_OK;
    for (auto it = h->chans.begin(); it != h->chans.end();) {
        if (it->second->src >= RCF_SRC_PFB_BIN0) { free_channel(h, it->second.get()); it = h->chans.erase(it); }
        else ++it;
    }
    pfb_release(h);
    ++h->chans_epoch;
    return RCF_OK;
}

int rcf_pfb_tap_leakage(double samp_rate, int n_bins, const float *taps, int ntaps, int bin, double *leak_l2,
                        double *const_phase)
{
    if (!(samp_rate > 0) || n_bins < 1 || !taps || ntaps < 1 || bin < 0 || bin >= n_bins) {
        set_error("bad tap-leakage arguments");
        return RCF_EINVAL;
    }
    design_tap_leakage(samp_rate, n_bins, taps, ntaps, bin, leak_l2, const_phase);
    return RCF_OK;
}

int rcf_pfb_shape_supported(int n_bins, int decim, int ntaps)
{
    if (n_bins < 1 || ntaps < 1) return 0;
    return pfb_shape(n_bins, decim, (ntaps + n_bins - 1) / n_bins).family ? 1 : 0;
}

int rcf_pfb_shape_family(int n_bins, int decim, int ntaps)
{
    if (n_bins < 1 || ntaps < 1) return 0;
    return pfb_shape(n_bins, decim, (ntaps + n_bins - 1) / n_bins).family;
}

int64_t rcf_pfb_produced(rcf_t *h)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    return h->pfb.open ? h->pfb.produced : RCF_ESTATE;
}

int64_t rcf_pfb_read_bin(rcf_t *h, int bin, float *out, size_t max_samples)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Pfb &p = h->pfb;
    if (!p.open || bin < 0 || bin >= p.NB) { set_error("no such PFB bin %d", bin); return RCF_EINVAL; }
    if (p.fm_mode == 2) { set_error("the bank writes its discriminator ring only (rcf_pfb_fm_enable mode 2): no bins to read"); return RCF_ESTATE; }
    // one bin out of the bank's ring (tiled or frame-major -- not a strided ring: gather_view_kernel, not host_read) into the
    // handle's pinned staging
    const int64_t n = lag_clamp((int64_t)h->out_cap, &p.rd[bin], p.produced, p.produced, (int64_t)max_samples);
    if (n == 0) return 0;
    SrcRange sr{};
    if (!source_range(h, RCF_SRC_PFB_BIN0 + bin, 0, 0, &sr)) return RCF_ESTATE;
    const int rc = h->host_stage.ensure(sizeof(float2) * (size_t)n, h->stream);
    if (rc != RCF_OK) return rc;
    launch_gather_view(sr.view, p.rd[bin], reinterpret_cast<float2 *>(h->host_stage.d), (size_t)n, h->stream);
    RCF_HIP(hipStreamSynchronize(h->stream));
    free_graveyard_idle(h);
    std::memcpy(out, h->host_stage.h, sizeof(float2) * (size_t)n);
    p.rd[bin] += n;
    return n;
}

int rcf_pfb_fm_enable(rcf_t *h, int mode, int gr_phase)
{
    if (!h || mode < 0 || mode > 2) { set_error("bad fm mode"); return RCF_EINVAL; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Pfb &p = h->pfb;
    if (!p.open) { set_error("no filterbank open"); return RCF_ESTATE; }
    if (mode == 2) {
        // the bins ring is not written in mode 2: nothing may be left filtering it (taps are copied by the kernel itself)
        for (const auto &kv : h->chans)
            if (kv.second->src >= RCF_SRC_PFB_BIN0 && !kv.second->is_tap) {
                set_error("channel %d reads bin %d of the bins ring, which mode 2 stops writing: close it first", kv.first,
                          kv.second->src - RCF_SRC_PFB_BIN0);
                return RCF_ESTATE;
            }
        if (p.sq.on) { set_error("the carrier detector (rcf_pfb_squelch) reads the bins ring, which mode 2 stops writing: switch it off first"); return RCF_ESTATE; }
    }
    if (p.fm_mode == 2 && mode != 2)                      // the frames of mode 2 never reached the bins ring: its readers skip them
        for (auto &r : p.rd) r = std::max(r, p.produced);
    if (mode == 0) {
        if (p.fm_mode) p.fm_until = p.produced;          // frames from here on are not demodulated: readers stop here
        p.fm_mode = 0;
        return RCF_OK;
    }
    if (!p.shape.fused) {
        set_error("no fused-discriminator kernel for bins=%d decim=%d taps/branch=%d", p.NB, p.D, p.P);
        return RCF_EINVAL;
    }
    const size_t need = p.shape.fused_history;
    if (need > h->hist_cap) { set_error("history capacity %zu < %zu (the fused discriminator's halo chunk)", h->hist_cap, need); return RCF_ECAP; }
    if (!p.d_fm) {
        // The look-back form's hand-over rows (RCF_PFB5_FM_LOOKBACK=0: the span form, which needs none).  Chunk c of a launch
        // publishes its last frame in row c mod fm_slots and waits for row c - 1: with one slot per chunk of the largest
        // launch the handle accepts no two chunks of a launch share a row or a flag, however the workgroups are dispatched,
        // retired or interleaved.  A launch is one block: at most ceil(block_cap / D) frames, and at most out_cap (plan_pfb,
        // which also refuses a launch with more chunks than rows).  Rows of an earlier launch are never taken for this
        // one's: launches of one bank run in stream order and every launch has its own tag (plan_pfb).
        static const bool lookback = [] { const char *e = getenv("RCF_PFB5_FM_LOOKBACK"); return !e || atoi(e) != 0; }();
        const int64_t max_frames = std::min<int64_t>((int64_t)h->out_cap, ceil_div((int64_t)h->block_cap, p.D));
        const int64_t slots = lookback ? ceil_div(max_frames, p.shape.chunk_frames) : 0;
        if (slots > (int64_t(1) << 27)) { set_error("output capacity %zu: too many hand-over rows for the fused discriminator", h->out_cap); return RCF_ECAP; }
        p.rd_fm.assign((size_t)p.NB, p.produced);
        // all or nothing: every buffer goes into a local first, the bank takes them only once all of them exist
        const size_t ring = (size_t)p.NB * h->out_cap;
        float *d_fm = nullptr;
        float2 *d_fm_inc = nullptr;
        unsigned long long *d_fm_edge = nullptr, *d_fm_flag = nullptr;      // [slots + 9][NB] rows, [slots][8] flags (one per wave)
        int *d_fm_err = nullptr;
        bool ok = hip_ok(hipMalloc(&d_fm, sizeof(float) * ring), "hipMalloc(fm ring)") &&
                  hip_ok(hipMalloc(&d_fm_inc, sizeof(float2) * (size_t)p.NB), "hipMalloc(fm increments)") &&
                  hip_ok(hipMemsetAsync(d_fm, 0, sizeof(float) * ring, h->stream), "hipMemset(fm ring)");
        if (ok && slots)
            ok = hip_ok(hipMalloc(&d_fm_edge, sizeof(unsigned long long) * (size_t)(slots + 9) * (size_t)p.NB), "hipMalloc(fm edge rows)") &&
                 hip_ok(hipMalloc(&d_fm_flag, sizeof(unsigned long long) * (size_t)slots * 8), "hipMalloc(fm flags)") &&
                 hip_ok(hipMalloc(&d_fm_err, sizeof(int)), "hipMalloc(fm lost count)") &&
                 hip_ok(hipMemsetAsync(d_fm_flag, 0, sizeof(unsigned long long) * (size_t)slots * 8, h->stream), "hipMemset(fm flags)") &&
                 hip_ok(hipMemsetAsync(d_fm_err, 0, sizeof(int), h->stream), "hipMemset(fm lost count)");
        if (!ok) {
            (void)hipStreamSynchronize(h->stream);       // (a memset may be queued on what is freed)
            for (void *q : {(void *)d_fm, (void *)d_fm_inc, (void *)d_fm_edge, (void *)d_fm_flag, (void *)d_fm_err})
                if (q) (void)hipFree(q);
            return RCF_EHIP;
        }
        p.d_fm = d_fm;
        p.d_fm_inc = d_fm_inc;
        p.d_fm_edge = d_fm_edge;
        p.d_fm_flag = d_fm_flag;
        p.d_fm_err = d_fm_err;
        p.fm_slots = (int)slots;
        if (slots) p.fm_local = pfb5_xcd_map_ok(h->device, h->stream) ? 1 : 0;
        p.fm_from = p.produced;
    } else if (p.fm_mode == 0) {                       // switched on again: the frames in between were not demodulated
        p.fm_from = p.produced;
        for (auto &r : p.rd_fm) r = std::max(r, p.produced);
    }
    p.fm_gr_phase = gr_phase ? 1 : 0;
    const int rc = pfb_fm_upload_increments(h);
    if (rc != RCF_OK) return rc;
    p.fm_mode = mode;
    return RCF_OK;
}

int64_t rcf_pfb_read_fm(rcf_t *h, int bin, float gain, float *out, size_t max_samples)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Pfb &p = h->pfb;
    if (!p.open || !p.d_fm || bin < 0 || bin >= p.NB) { set_error("no discriminator ring / no such bin %d", bin); return RCF_EINVAL; }
    Stream s;
    (void)pfb_fm_stream(h, bin, &p.rd_fm[(size_t)bin], false, &s);
    return read_one(h, s, gain, out, max_samples);
}

int64_t rcf_pfb_fm_lost(rcf_t *h)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Pfb &p = h->pfb;
    if (!p.open || !p.d_fm) { set_error("no discriminator ring"); return RCF_ESTATE; }
    if (!p.d_fm_err) return 0;
    int v = 0;
    RCF_HIP(hipMemcpyAsync(&v, p.d_fm_err, sizeof v, hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipStreamSynchronize(h->stream));
    return v;
}

int rcf_pfb_fm_ring(rcf_t *h, void **fm_ring, size_t *capacity_frames, int64_t *first_frame)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    if (!h->pfb.open || !h->pfb.d_fm) return RCF_ESTATE;
    if (fm_ring) *fm_ring = h->pfb.d_fm;
    if (capacity_frames) *capacity_frames = h->out_cap;
    if (first_frame) *first_frame = h->pfb.fm_from;
    return RCF_OK;
}

// ---- carrier detect on every bin (squelch.hip)
int rcf_pfb_squelch_segment(void) { return pfb_squelch_segment(); }

int rcf_pfb_squelch(rcf_t *h, const double *threshold_db, int n, double alpha)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Pfb &p = h->pfb;
    if (!p.open) { set_error("no filterbank open"); return RCF_ESTATE; }
    Pfb::Squelch &q = p.sq;
    if (!threshold_db) {                                       // off: the state stays readable as the last block left it
        if (q.on) q.until = p.produced;
        q.on = false;
        return RCF_OK;
    }
    if ((n != 1 && n != p.NB) || !(alpha > 0.0 && alpha <= 1.0)) {
        set_error("carrier detect: %d thresholds for %d bins (1 or all of them), or alpha %g outside (0, 1]", n, p.NB, alpha);
        return RCF_EINVAL;
    }
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(threshold_db[k])) { set_error("carrier detect: threshold %d is not finite", k); return RCF_EINVAL; }
    if (p.fm_mode == 2) { set_error("the bank writes its discriminator ring only (rcf_pfb_fm_enable mode 2): no bins for the carrier detector to read"); return RCF_ESTATE; }
    // a fresh state on every call: level 0, no bin open, counters 0.  The old one goes once the stream has passed it
    Pfb::Squelch nq;
    nq.bins_pad = ((size_t)p.NB + 63) & ~size_t(63);
    std::vector<double> st0(nq.state_doubles(), 0.0);
    int64_t *last = reinterpret_cast<int64_t *>(st0.data() + 3 * nq.bins_pad);
    for (size_t k = 0; k < nq.bins_pad; ++k) {
        last[k] = -1;
        st0[4 * nq.bins_pad + k] = squelch_threshold(threshold_db[n == 1 ? 0 : std::min<size_t>(k, (size_t)p.NB - 1)]);
    }
    // the z scratch of the largest launch the handle accepts: a block is at most ceil(block_cap / D) frames, and at most out_cap
    const int64_t max_frames = std::min<int64_t>((int64_t)h->out_cap, ceil_div((int64_t)h->block_cap, p.D));
    const size_t z_rows = (size_t)ceil_div(max_frames, pfb_squelch_segment());
    Fresh<double> d_state, d_z;
    RCF_HIP(d_state.alloc(st0.size()));
    if (!q.d_z) RCF_HIP(d_z.alloc(z_rows * (size_t)p.NB));
    if (!hip_ok(hipMemcpy(d_state.p, st0.data(), sizeof(double) * st0.size(), hipMemcpyHostToDevice), "hipMemcpy(carrier detect state)")) return RCF_EHIP;
    nq.on = true;
    nq.alpha = alpha;
    nq.a_pow_s = squelch_a_pow_s(alpha, pfb_squelch_segment());
    nq.d_z = q.d_z ? q.d_z : d_z.take();
    nq.d_state = d_state.take();
    nq.from = p.produced;
    bury(h, q.d_state);
    q = nq;
    return RCF_OK;
}

int rcf_pfb_squelch_read(rcf_t *h, double *level, int64_t *n_open, int64_t *last_open, uint32_t *unmuted_mask, int n_bins,
                         int64_t *frames_seen)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Pfb &p = h->pfb;
    if (!p.open) { set_error("no filterbank open"); return RCF_ESTATE; }
    const Pfb::Squelch &q = p.sq;
    if (!q.d_state) { set_error("the bank carries no carrier detector (rcf_pfb_squelch)"); return RCF_ESTATE; }
    if (n_bins != p.NB) { set_error("carrier detect: %d bins asked for, the bank has %d", n_bins, p.NB); return RCF_EINVAL; }
    std::vector<double> st(q.state_doubles());
    RCF_HIP(hipMemcpyAsync(st.data(), q.d_state, sizeof(double) * st.size(), hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipStreamSynchronize(h->stream));
    free_graveyard_idle(h);
    const size_t nb = (size_t)p.NB;
    if (level) std::memcpy(level, st.data() + (size_t)q.cur * q.bins_pad, sizeof(double) * nb);
    if (n_open) std::memcpy(n_open, st.data() + 2 * q.bins_pad, sizeof(int64_t) * nb);
    if (last_open) std::memcpy(last_open, st.data() + 3 * q.bins_pad, sizeof(int64_t) * nb);
    if (unmuted_mask) std::memcpy(unmuted_mask, st.data() + 5 * q.bins_pad, sizeof(uint32_t) * ((nb + 31) / 32));
    // (off: the count stands where the detector was switched off)
    if (frames_seen) *frames_seen = (q.on ? p.produced : q.until) - q.from;
    return RCF_OK;
}

int rcf_pfb_rings(rcf_t *h, void **bins_ring, size_t *capacity, size_t *pitch)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;                  // (queues the deferred stage-2 launch: see rcf_chan_rings)
    if (!h->pfb.open) return RCF_ESTATE;
    if (h->pfb.fm_mode == 2) { set_error("the bank writes its discriminator ring only (rcf_pfb_fm_enable mode 2): no bins ring"); return RCF_ESTATE; }
    if (bins_ring) *bins_ring = h->pfb.d_bins;
    if (capacity) *capacity = h->out_cap;
    if (pitch) *pitch = h->pfb.shape.frame_major ? 0 : (size_t(1) << kPfbTileLog2);   // frames per tile (0: frame-major)
    return RCF_OK;
}

// ------------------------------------------------------------------ scan
int rcf_scan_start(rcf_t *h, int fft_len, int n_frames, int avg_len)
{
    if (!h || n_frames < 1 || avg_len < 1) { set_error("bad scan arguments"); return RCF_EINVAL; }
    if (!scan_supported(fft_len)) { set_error("unsupported scan FFT length %d", fft_len); return RCF_EINVAL; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    if ((size_t)fft_len > h->hist_cap) { set_error("history capacity %zu < fft_len %d", h->hist_cap, fft_len); return RCF_ECAP; }
    Scan &s = h->scan;
    // frames per launch: enough workgroups to fill 256 CUs (2^25 samples per launch), bounded so that
    // the log-magnitude ring ((avg_len + chunk) x N floats) and the four-step scratch stay modest
    int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(512, (int64_t(1) << 25) / fft_len));
    chunk = std::min(chunk, n_frames);
    if (s.d_vring && s.N == fft_len && s.L == avg_len && s.chunk == chunk) {
        // same geometry as the previous scan: keep every buffer (fresh device allocations cost tens of
        // milliseconds of first-touch page faults), just reset the running state
        s.n_frames = n_frames;
        s.frames_done = 0;
        s.done = false;
        s.start_sample = h->total_in;
        RCF_HIP(hipMemsetAsync(s.d_sum, 0, sizeof(float) * (size_t)fft_len, h->stream));
        RCF_HIP(hipMemsetAsync(s.d_out, 0, sizeof(float) * (size_t)fft_len, h->stream));
        s.armed = true;
        return RCF_OK;
    }
    bury(h, s.d_window); bury(h, s.d_vring); bury(h, s.d_sum); bury(h, s.d_out); bury(h, s.d_tw);
    bury(h, s.d_scratch); bury(h, s.d_peaks); bury(h, s.d_peak_ws);
    s = Scan();
    s.N = fft_len; s.n_frames = n_frames; s.L = avg_len;
    s.chunk = chunk;
    s.R = avg_len + s.chunk;
    std::vector<float> win(fft_len), tw(2 * (size_t)fft_len);
    design_window(RCF_WIN_BLACKMAN_HARRIS, fft_len, win.data());
    auto fill = [&](size_t at, int count, double step) {      // tw[at + i] = e^{-j step i}
        for (int i = 0; i < count; ++i) {
            tw[2 * (at + i)] = (float)std::cos(-step * i);
            tw[2 * (at + i) + 1] = (float)std::sin(-step * i);
        }
    };
    int n1 = 0, n2 = 0;
    if (fft_len > 16384 && scan4_split(fft_len, &n1, &n2)) {
        // four-step tables: [e^{-2 pi i n/N1} | e^{-2 pi i n/N2} | W_N^i, i<1024 | W_N^{1024 j}]
        fill(0, n1, kTwoPi / n1);
        fill((size_t)n1, n2, kTwoPi / n2);
        fill((size_t)n1 + n2, 1024, kTwoPi / fft_len);
        fill((size_t)n1 + n2 + 1024, fft_len / 1024, kTwoPi * 1024.0 / fft_len);
    } else {
        fill(0, fft_len, kTwoPi / fft_len);
    }
    RCF_HIP(hipMalloc(&s.d_window, sizeof(float) * (size_t)fft_len));
    RCF_HIP(hipMemcpy(s.d_window, win.data(), sizeof(float) * (size_t)fft_len, hipMemcpyHostToDevice));
    RCF_HIP(hipMalloc(&s.d_tw, sizeof(float2) * (size_t)fft_len));
    RCF_HIP(hipMemcpy(s.d_tw, tw.data(), sizeof(float2) * (size_t)fft_len, hipMemcpyHostToDevice));
    RCF_HIP(hipMalloc(&s.d_vring, sizeof(float) * (size_t)fft_len * s.R));
    RCF_HIP(hipMalloc(&s.d_sum, sizeof(float) * (size_t)fft_len));
    RCF_HIP(hipMalloc(&s.d_out, sizeof(float) * (size_t)fft_len));
    RCF_HIP(hipMemsetAsync(s.d_sum, 0, sizeof(float) * (size_t)fft_len, h->stream));
    RCF_HIP(hipMemsetAsync(s.d_out, 0, sizeof(float) * (size_t)fft_len, h->stream));
    if (fft_len > 16384) RCF_HIP(hipMalloc(&s.d_scratch, sizeof(float2) * (size_t)fft_len * s.chunk));
    s.start_sample = h->total_in;
    s.armed = true;
    return RCF_OK;
}

int rcf_scan_frames_done(rcf_t *h)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    return h->scan.armed ? h->scan.frames_done : RCF_ESTATE;
}

int rcf_scan_result(rcf_t *h, float *out)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Scan &s = h->scan;
    if (!s.armed) { set_error("scan not armed"); return RCF_ESTATE; }
    if (!s.done) return RCF_EAGAIN;
    RCF_HIP(hipMemcpyAsync(out, s.d_out, sizeof(float) * (size_t)s.N, hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipStreamSynchronize(h->stream));
    return RCF_OK;
}

int rcf_scan_result_device(rcf_t *h, void **dev_spectrum)
{
    if (!h || !dev_spectrum) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->scan.armed) return RCF_ESTATE;
    if (!h->scan.done) return RCF_EAGAIN;
    *dev_spectrum = h->scan.d_out;
    return RCF_OK;
}

int rcf_find_peaks(const float *spectrum, int64_t n, double min_w, double max_w, double prominence, int64_t *idx,
                   int64_t cap, int64_t *count, double *mean_out)
{
    if (!spectrum || n < 0 || cap < 0 || (cap > 0 && !idx)) { set_error("bad find_peaks arguments"); return RCF_EINVAL; }
    const int64_t c = find_peaks_host(spectrum, n, min_w, max_w, prominence, idx, cap, mean_out);
    if (count) *count = c;
    return RCF_OK;
}

int64_t rcf_peak_frequency(int64_t line, double samp_rate, int64_t fft_len, double center_freq)
{
    const double hz_per_bin = samp_rate / (double)fft_len;
    return (int64_t)(((double)line * hz_per_bin) - (samp_rate / 2) + center_freq);
}

int rcf_scan_find_peaks(rcf_t *h, double prominence, int64_t *idx, int64_t cap, int64_t *count, double *mean_out,
                        void **dev_idx)
{
    if (!h || cap < 1) { set_error("bad arguments"); return RCF_EINVAL; }
    if (cap > 4096) cap = 4096;                       // device sort capacity
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Scan &s = h->scan;
    if (!s.armed) return RCF_ESTATE;
    if (!s.done) return RCF_EAGAIN;
    const int N = s.N;
    const double hz_per_bin = h->fs / N;              // fft_peak_detection.py:46-52
    if (!s.d_peak_ws) RCF_HIP(hipMalloc(&s.d_peak_ws, peaks_workspace_bytes(N)));
    if (!s.d_peaks) RCF_HIP(hipMalloc(&s.d_peaks, sizeof(int64_t) * 4096));
    int *d_count = nullptr;
    double *d_mean = nullptr;
    launch_find_peaks(s.d_out, N, 3000 / hz_per_bin, 30000 / hz_per_bin, prominence, s.d_peak_ws, s.d_peaks,
                      (int)cap, &d_count, &d_mean, h->stream);
    int c = 0;
    double mean = 0.0;
    RCF_HIP(hipMemcpyAsync(&c, d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipMemcpyAsync(&mean, d_mean, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (idx) RCF_HIP(hipMemcpyAsync(idx, s.d_peaks, sizeof(int64_t) * (size_t)cap, hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipStreamSynchronize(h->stream));
    if (count) *count = c;
    if (mean_out) *mean_out = mean;
    if (dev_idx) *dev_idx = s.d_peaks;                // sorted ascending, -1 padded to `cap`
    return RCF_OK;
}

}  // extern "C"
