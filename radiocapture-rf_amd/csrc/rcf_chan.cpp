// rcf_chan.cpp -- channels: lifecycle (channel.channel / set_offset / destroy of /root/reference/rc_frontend/channel.py),
// taps of a filterbank, discriminator-only taps, source shift, info and produced queries.
#include "rcf_plan.h"


namespace rcfx {

bool source_range(rcf_t *h, int src, int64_t S0, int64_t S1, SrcRange *out)
{
    if (src < 0) {
        out->view.base = h->d_buf[h->cur];
        out->view.mask = ~0ull;
        out->view.origin = S0 - (int64_t)h->hist_cap;
        out->view.stride = 1;
        out->p0 = S0;
        out->p1 = S1;
        return true;
    }
    if (src >= RCF_SRC_PFB_BIN0) {
        if (!h->pfb.open) return false;
        const int bin = src - RCF_SRC_PFB_BIN0;
        if (h->pfb.shape.frame_major) {                           // bins_ring[i NB + bin]
            out->view.base = h->pfb.d_bins + bin;
            out->view.stride = h->pfb.NB;
            out->view.tshift = 0;
        } else {                                            // bins_ring[(i >> 4) tile_pitch + 16 bin + (i & 15)]
            out->view.base = h->pfb.d_bins + ((size_t)bin << kPfbTileLog2);
            out->view.stride = pfb_tile_pitch(h->pfb.NB);
            out->view.tshift = kPfbTileLog2;
        }
        out->view.mask = h->ring_mask;
        out->view.origin = 0;
        out->p0 = h->pfb.produced_before;
        out->p1 = h->pfb.produced;
        return true;
    }
    return false;   // channel-sourced: resolved by the caller (needs per-commit bookkeeping)
}

// What GNU Radio's freq_xlating_fir_filter_ccc(D, h, f_k, fs) on bin k's frequency would have done differently from the
// bank's exact phases, per output: its rotator advances by a = float32(-float32(2 pi f_k / fs) * D) instead of
// -2 pi k D / NB.  The difference, folded into (-pi, pi]: a tap's Chan::extra_dangle.
struct GrTap { int ks; float a; };          // the bin's signed index, GNU Radio's rotator advance per output
static GrTap gr_tap(const rcf_t *h, int bin)
{
    const Pfb &p = h->pfb;
    const int ks = bin < p.NB / 2 ? bin : bin - p.NB;
    const double f_k = (double)ks * h->fs / p.NB;
    const float fwT0 = (float)(kTwoPi * f_k / h->fs);
    return GrTap{ks, -fwT0 * (float)p.D};
}

double pfb_tap_gr_dangle(const rcf_t *h, int bin)
{
    const Pfb &p = h->pfb;
    const auto [ks, a] = gr_tap(h, bin);
    const long double exact = -2.0L * 3.14159265358979323846264338327950288L *
                              (long double)(((int64_t)ks * p.D) % p.NB) / (long double)p.NB;
    long double d = (long double)a - exact;
    d = remainderl(d, 2.0L * 3.14159265358979323846264338327950288L);
    return (double)d;
}

int upload_composite(rcf_t *h, Chan *c)
{
    std::vector<float> ct;
    float incr[2];
    // rcf_source_shift moves every signal of the source by -shift at baseband: the wideband channels' NCOs follow,
    // and so do the channels fed by filterbank bins (same Hz, at the bin rate)
    const bool shifted = c->src < 0 || c->src >= RCF_SRC_PFB_BIN0;
    design_composite(c->proto.data(), c->T, c->D, c->offset_hz + (shifted ? h->shift_hz : 0.0), c->src_rate,
                     ct, incr);
    const size_t slice = slice_round(sizeof(float2) * (size_t)c->T);
    float2 *fresh = static_cast<float2 *>(pool_get(h, slice));
    if (!fresh) return RCF_ENOMEM;
    if (!hip_ok(hipMemcpy(fresh, ct.data(), sizeof(float2) * (size_t)c->T, hipMemcpyHostToDevice), "hipMemcpy(taps)")) {
        h->pools[slice].free_.push_back(fresh);
        return RCF_EHIP;
    }
    bury(h, c->d_ctaps, slice);
    c->d_ctaps = fresh;
    c->taps_version = ++h->taps_clock;
    // GR iterates phase *= incr in float32; model it by the increment's actual angle and magnitude
    c->incr[0] = incr[0];
    c->incr[1] = incr[1];
    c->dangle = std::atan2((double)incr[1], (double)incr[0]) + c->extra_dangle;
    c->dlogmag = std::log(std::hypot((double)incr[0], (double)incr[1])) + c->extra_dlogmag;
    return RCF_OK;
}

int new_channel(rcf_t *h, int src, int D, const float *taps, int T, double offset_hz, int *chan_id, bool tap)
{
    if (D < 1 || T < 1 || !taps || !chan_id) { set_error("bad channel arguments"); return RCF_EINVAL; }
    if (src >= RCF_SRC_PFB_BIN0 && !tap && h->pfb.open && h->pfb.fm_mode == 2) {
        set_error("the bank writes its discriminator ring only (rcf_pfb_fm_enable mode 2): no bins ring to filter");
        return RCF_ESTATE;
    }
    std::unique_ptr<Chan> c(new Chan);
    c->src = src;
    c->D = D;
    c->T = T;
    c->offset_hz = offset_hz;
    c->proto.assign(taps, taps + T);
    if (src < 0) {
        c->src_rate = h->fs;
        c->start_sample = h->total_in;
        c->depth = 0;
        if ((size_t)(T - 1 + D) > h->hist_cap) { set_error("history capacity %zu < T-1+D", h->hist_cap); return RCF_ECAP; }
    } else if (src >= RCF_SRC_PFB_BIN0) {
        if (!h->pfb.open || src - RCF_SRC_PFB_BIN0 >= h->pfb.NB) { set_error("no such PFB bin"); return RCF_EINVAL; }
        c->src_rate = h->fs / h->pfb.D;
        c->start_sample = h->pfb.produced;
        c->depth = 1;
    } else {
        auto it = h->chans.find(src);
        if (it == h->chans.end()) { set_error("no such source channel %d", src); return RCF_ENOCHAN; }
        if (it->second->fm_only) { set_error("channel %d exposes its discriminator only: no IQ stream to chain on", src); return RCF_ESTATE; }
        c->src_rate = it->second->src_rate / it->second->D;
        c->start_sample = it->second->pos.produced;
        c->depth = it->second->depth + 1;
    }
    if (src >= 0 && (size_t)(T + D) * 2 > h->out_cap) { set_error("source ring too small for T=%d", T); return RCF_ECAP; }
    c->k_abs0 = ceil_div(c->start_sample, D);
    // iq ring + discriminator ring in one slice.  Not cleared: readers never go past `produced`, and every
    // kernel masks what lies before a channel's first output (GR zero history)
    const size_t ring_slice = slice_round(12 * h->out_cap);
    c->d_iq = static_cast<float2 *>(pool_get(h, ring_slice));
    if (!c->d_iq) return RCF_ENOMEM;
    c->d_fm = reinterpret_cast<float *>(c->d_iq + h->out_cap);
    if (h->exact_rot) {
        const size_t rot_slice = slice_round(sizeof(float2) * h->out_cap + 256);
        c->d_rot = static_cast<float2 *>(pool_get(h, rot_slice));
        if (!c->d_rot) { h->pools[ring_slice].free_.push_back(c->d_iq); return RCF_ENOMEM; }
        const float st0[4] = {1.0f, 0.0f, 0.0f, 0.0f};       // phase 1 + 0j, counter 0 (bit pattern of 0.0f)
        if (!hip_ok(hipMemcpy(c->d_rot + h->out_cap, st0, sizeof(st0), hipMemcpyHostToDevice), "hipMemcpy(rotator state)")) {
            h->pools[rot_slice].free_.push_back(c->d_rot);
            h->pools[ring_slice].free_.push_back(c->d_iq);
            return RCF_EHIP;
        }
    }
    int rc = upload_composite(h, c.get());
    if (rc != RCF_OK) {
        h->pools[ring_slice].free_.push_back(c->d_iq);      // never seen by the stream: straight back
        if (c->d_rot) h->pools[slice_round(sizeof(float2) * h->out_cap + 256)].free_.push_back(c->d_rot);
        return rc;
    }
    c->id = h->next_id++;
    *chan_id = c->id;
    h->chans[c->id] = std::move(c);
    ++h->chans_epoch;
    return RCF_OK;
}

void free_channel(rcf_t *h, Chan *c)
{
    bury(h, c->d_ctaps, slice_round(sizeof(float2) * (size_t)c->T));
    bury(h, c->d_iq, slice_round(12 * h->out_cap));       // d_fm lives in the same slice
    bury(h, c->d_rot, slice_round(sizeof(float2) * h->out_cap + 256));
    c->for_each_stage([h](auto &stage, size_t, bool) { drop_stage(h, stage); });
}

}  // namespace rcfx

using namespace rcfx;

// =================================================================== C ABI
extern "C" {

// ------------------------------------------------------------------ channels
int rcf_chan_open(rcf_t *h, int channel_rate, double offset_hz, int *chan_id)
{
    if (!h || !chan_id) { set_error("bad channel arguments"); return RCF_EINVAL; }
    int D = 0, T = 0;
    int rc = rcf_channel_params_ex(h->fs, channel_rate, h->decim_rule, &D, &T, nullptr);
    if (rc != RCF_OK) return rc;
    if (!(std::fabs(offset_hz) < h->fs / 2)) { set_error("offset %g Hz outside +-fs/2", offset_hz); return RCF_ERANGE; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    std::vector<float> &taps = h->proto_cache[channel_rate];
    if (taps.empty())
        taps = design_low_pass_2(1.0, h->fs, channel_rate / 2.0, channel_rate / 2.0, 20.0, RCF_WIN_HAMMING);
    return new_channel(h, -1, D, taps.data(), (int)taps.size(), offset_hz, chan_id);
}

int rcf_chan_open_taps(rcf_t *h, int src_chan, int decim, const float *taps, int ntaps, double offset_hz,
                       int *chan_id)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    return new_channel(h, src_chan < 0 ? -1 : src_chan, decim, taps, ntaps, offset_hz, chan_id);
}

int rcf_pfb_chan_open(rcf_t *h, int bin, int channel_rate, double delta_hz, int *chan_id)
{
    if (!h || !chan_id) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    if (!h->pfb.open || bin < 0 || bin >= h->pfb.NB) { set_error("no such PFB bin %d", bin); return RCF_EINVAL; }
    const double rate = h->fs / h->pfb.D;
    int D = 0, T = 0;
    int rc = rcf_channel_params_ex(rate, channel_rate, h->decim_rule, &D, &T, nullptr);
    if (rc != RCF_OK) return rc;
    std::vector<float> taps = design_low_pass_2(1.0, rate, channel_rate / 2.0, channel_rate / 2.0, 20.0,
                                                RCF_WIN_HAMMING);
    return new_channel(h, RCF_SRC_PFB_BIN0 + bin, D, taps.data(), (int)taps.size(), delta_hz, chan_id);
}

int rcf_pfb_tap_open(rcf_t *h, int bin, int gr_phase, int *chan_id)
{
    if (!h || !chan_id) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    Pfb &p = h->pfb;
    if (!p.open || bin < 0 || bin >= p.NB) { set_error("no such PFB bin %d", bin); return RCF_EINVAL; }
    const float one = 1.0f;
    int rc = new_channel(h, RCF_SRC_PFB_BIN0 + bin, 1, &one, 1, 0.0, chan_id, p.shape.frame_major);
    if (rc != RCF_OK) return rc;
    h->chans[*chan_id]->is_tap = p.shape.frame_major;     // power-of-two banks: an ordinary D = 1, T = 1 channel on the bin's ring
    ++h->chans_epoch;                                // (the planning summary counts taps and FIR channels differently)
    if (gr_phase) {
        // What GNU Radio's freq_xlating_fir_filter_ccc(D, h, f_k, fs) would have done differently from the bank's
        // exact phases: its rotator advances by a = float32(-float32(2 pi f_k / fs) * D) per output instead of
        // -2 pi k D / NB, and the float32 increment (cosf a, sinf a) is not exactly of unit length.  Both are
        // per-output factors: this channel's own rotator carries them.
        Chan *c = h->chans[*chan_id].get();
        const auto [ks, a] = gr_tap(h, bin);
        c->extra_dangle = pfb_tap_gr_dangle(h, bin);
        c->extra_dlogmag = std::log(std::hypot((double)std::cos(a), (double)std::sin(a)));
        // ... and GNU Radio's float32 tap phases float32(i * fwT0) differ from the bank's 2 pi k i / NB by a constant
        // (their filter-weighted mean, up to ~3e-4 rad) plus rounding noise (rcf_pfb_tap_leakage): the constant is a
        // rotation of the whole output and goes into the rotator's start phase
        double cphase = 0.0;
        design_tap_leakage(h->fs, p.NB, p.proto.data(), (int)p.proto.size(), bin, nullptr, &cphase);
        // ... and GNU Radio's rotator stands at 1 when the channel emits its FIRST output, whereas the bank's bin carries
        // e^{-j 2 pi k D n / NB} counted from the stream's first sample: a channel that starts at the bank's frame n0
        // is the bin times e^{+j 2 pi k D n0 / NB} (exact: integers mod NB; a sign for the 12.5 kHz grid's OS = 2 banks)
        const int64_t n0 = p.n_abs0 + c->k_abs0;
        const int64_t kd = (((int64_t)ks * p.D) % p.NB + p.NB) % p.NB;
        const int64_t turn = (kd * (n0 % p.NB)) % p.NB;
        c->pos.angle0 = (long double)cphase +
                    remainderl(2.0L * 3.14159265358979323846264338327950288L * (long double)turn / (long double)p.NB,
                               2.0L * 3.14159265358979323846264338327950288L);
        rc = upload_composite(h, c);
    }
    {
        // plan_channel never iterates the exact rotator for a frame-major bank's tap or a channel that carries GNU
        // Radio's phase corrections: give the phase ring (8 out_cap bytes, half a megabyte at 2^16) back -- a
        // receiver in 'pfb' mode opens hundreds of these.  Nothing has been queued on it yet.
        Chan *c = h->chans[*chan_id].get();
        if (c->d_rot && (c->is_tap || c->extra_dangle != 0.0 || c->extra_dlogmag != 0.0)) {
            h->pools[slice_round(sizeof(float2) * h->out_cap + 256)].free_.push_back(c->d_rot);
            c->d_rot = nullptr;
        }
    }
    return rc;
}

int rcf_chan_set_offset(rcf_t *h, int chan_id, double offset_hz)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    c->offset_hz = offset_hz;
    return upload_composite(h, c);
}

int rcf_chan_close(rcf_t *h, int chan_id)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    free_channel(h, c);
    h->chans.erase(chan_id);
    ++h->chans_epoch;
    return RCF_OK;
}

int rcf_chan_info(rcf_t *h, int chan_id, int *decim, int *ntaps, double *out_rate, double *offset_hz)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    FIND_CHAN(h, chan_id, c);
    if (decim) *decim = c->D;
    if (ntaps) *ntaps = c->T;
    if (out_rate) *out_rate = c->src_rate / c->D;
    if (offset_hz) *offset_hz = c->offset_hz;
    return RCF_OK;
}

int64_t rcf_chan_produced(rcf_t *h, int chan_id)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;                  // (the count includes the deferred stage-2 block: it is queued first)
    FIND_CHAN(h, chan_id, c);
    return c->pos.produced;
}

int64_t rcf_chan_start(rcf_t *h, int chan_id)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    FIND_CHAN(h, chan_id, c);
    return c->start_sample;
}

int rcf_chan_fm_level(rcf_t *h, int chan_id, float gain, int window, float *level)
{
    if (!h || !level || window < 1) { set_error("bad fm level arguments"); return RCF_EINVAL; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if ((size_t)window > h->out_cap) { set_error("window %d exceeds the ring", window); return RCF_ECAP; }
    if (!h->d_level) RCF_HIP(hipMalloc(&h->d_level, sizeof(float)));
    launch_fm_level(c->d_fm, c->pos.produced, window, gain, h->ring_mask, h->d_level, h->stream);
    RCF_HIP(hipMemcpyAsync(level, h->d_level, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipStreamSynchronize(h->stream));
    return RCF_OK;
}

int rcf_chan_set_fm_only(rcf_t *h, int chan_id, int on)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->is_tap) { set_error("channel %d is not a tap of a frame-major filterbank", chan_id); return RCF_EINVAL; }
    if (on) {
        if (c->audio) { set_error("channel %d carries a voice chain, which reads its IQ stream", chan_id); return RCF_ESTATE; }
        if (c->agc) { set_error("channel %d carries an AGC, which reads its IQ stream", chan_id); return RCF_ESTATE; }
        if (c->squelch) { set_error("channel %d carries the carrier detector, which reads its IQ stream", chan_id); return RCF_ESTATE; }
        if (c->capture) { set_error("channel %d carries the capture stage, which reads its IQ stream", chan_id); return RCF_ESTATE; }
        for (auto &kv : h->chans)
            if (kv.second->src == chan_id) { set_error("channel %d reads channel %d's IQ stream", kv.first, chan_id); return RCF_ESTATE; }
    } else if (c->fm_only) {
        c->rd_iq = c->pos.produced;                  // what lies behind was never written
    }
    if ((on != 0) != c->fm_only && c->pos.produced > 0) {
        // The newest ring sample is the "output before" of the next block's first discriminator sample, and the two modes
        // keep it differently: rotated by the channel's rotator (ordinary tap) or as the bare bin (discriminator only: that
        // path never rotates, it turns the conjugate product by the rotator's increment instead).  Convert the one sample,
        // so that no discriminator sample straddles two conventions.  Only its angle matters to the discriminator.
        RCF_HIP(hipStreamSynchronize(h->stream));
        float2 *at = c->d_iq + ((uint64_t)(c->pos.produced - 1) & h->ring_mask);
        float2 v;
        RCF_HIP(hipMemcpy(&v, at, sizeof(v), hipMemcpyDeviceToHost));
        const long double ang = c->pos.angle0 + (long double)(c->pos.produced - 1 - c->pos.n_seg0) * (long double)c->dangle;
        const double pr = std::cos((double)ang), pi = (on ? -1.0 : 1.0) * std::sin((double)ang);
        const float2 w = make_float2((float)(v.x * pr - v.y * pi), (float)(v.x * pi + v.y * pr));
        RCF_HIP(hipMemcpy(at, &w, sizeof(w), hipMemcpyHostToDevice));
    }
    c->fm_only = on != 0;
    return RCF_OK;
}

int rcf_source_shift(rcf_t *h, double delta_hz)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    h->shift_hz += delta_hz;
    for (auto &kv : h->chans)
        if (kv.second->src < 0 || kv.second->src >= RCF_SRC_PFB_BIN0) {
            int rc = upload_composite(h, kv.second.get());
            if (rc != RCF_OK) return rc;
        }
    if (h->pfb.open && h->pfb.d_fm_inc) return pfb_fm_upload_increments(h);     // the bank's own discriminator follows too
    return RCF_OK;
}

}  // extern "C"
