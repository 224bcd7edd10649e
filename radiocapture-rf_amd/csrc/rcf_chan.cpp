// rcf_chan.cpp -- channels: lifecycle (channel.channel / set_offset / destroy of /root/reference/rc_frontend/channel.py),
// the one read path of every host read, the P25 symbol filter and AGC, the SmartNet / EDACS symbol clock, the analog voice
// chain, source shift.
#include <atomic>

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
double pfb_tap_gr_dangle(const rcf_t *h, int bin)
{
    const Pfb &p = h->pfb;
    const int ks = bin < p.NB / 2 ? bin : bin - p.NB;
    const double f_k = (double)ks * h->fs / p.NB;
    const float fwT0 = (float)(kTwoPi * f_k / h->fs);
    const float a = -fwT0 * (float)p.D;
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
        c->start_sample = it->second->produced;
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
    c->d_rot = nullptr;
    bury(h, c->d_sym);
    bury(h, c->d_symtaps);
    bury(h, c->d_agc);
    c->d_agc = nullptr;
    bury(h, c->d_clk);                                    // ring, state and the caller's bank: one allocation
    c->d_clk = nullptr;
    c->d_clk_taps = nullptr;
    if (c->audio) { bury(h, c->audio->d_state); bury(h, c->audio->d_rings); bury(h, c->audio->d_taps); c->audio.reset(); }
    c->d_sym = nullptr;
    c->d_symtaps = nullptr;
    c->d_ctaps = nullptr;
    c->d_iq = nullptr;
    c->d_fm = nullptr;
    (void)h;
}

// the stream table of a channel: RCF_READ_IQ, RCF_READ_FM, RCF_READ_AGC, kReadSym -> ring, words per item, reader, and what
// a missing ring means
int chan_stream(rcf_t *h, Chan *c, int kind, RingStream *s)
{
    const struct { const void *ring; uint32_t item_w; int64_t *cursor; const char *refusal; } t[4] = {
        {c->fm_only ? nullptr : c->d_iq, 2, &c->rd_iq, "channel %d exposes its discriminator only (rcf_chan_set_fm_only)"},
        {c->d_fm, 1, &c->rd_fm, "channel %d has no discriminator ring"},
        {c->d_agc, 2, &c->rd_agc, "channel %d has no AGC"},
        {c->d_sym, 1, &c->rd_sym, "channel %d has no fm filter"},
    };
    if (!t[kind].ring) { set_error(t[kind].refusal, c->id); return RCF_ESTATE; }
    *s = RingStream{h, t[kind].ring, t[kind].item_w, 0u, c->produced, c->produced, t[kind].cursor};
    return RCF_OK;
}

int PinnedStage::ensure(size_t need, hipStream_t stream)
{
    if (need <= cap) return RCF_OK;
    if (h) { RCF_HIP(hipStreamSynchronize(stream)); release(); }
    size_t ncap = 1 << 16;
    while (ncap < need) ncap <<= 1;
    void *p = nullptr, *dv = nullptr;
    if (hipHostMalloc(&p, ncap, hipHostMallocDefault) != hipSuccess || hipHostGetDevicePointer(&dv, p, 0) != hipSuccess) {
        if (p) (void)hipHostFree(p);
        set_error("pinned staging of %zu bytes for the batched read failed", ncap);
        return RCF_ENOMEM;
    }
    h = static_cast<unsigned char *>(p);
    d = static_cast<unsigned char *>(dv);
    cap = ncap;
    return RCF_OK;
}

// One gather launch packs every entry's segment back to back into pinned host memory, one synchronisation, then the rows are
// handed out.  (A device round trip per channel -- a single reader in a loop -- costs ~10 us each: 256 tapped bins of ten
// front-ends are 25 ms per pass.)
int host_read(PinnedStage &stage, hipStream_t stream, rcf_t *const *idle, size_t n_idle, ReadEntry *es, size_t n)
{
    static std::atomic<uint64_t> calls{0};
    const uint64_t stamp = ++calls;
    uint64_t total = 0, total_w = 0;
    uint32_t max_w = 0, n_recs = 0;
    for (size_t i = 0; i < n; ++i) {
        ReadEntry &e = es[i];
        if (e.c) {
            if (e.c->many_stamp == stamp) { *e.count = RCF_EINVAL; e.s.ring = nullptr; continue; }   // listed twice
            e.c->many_stamp = stamp;
        }
        if (!e.s.ring) continue;
        *e.count = lag_clamp(e.s.h, e.s.cursor, e.s.newest, e.s.end, e.max);
        if (*e.count == 0) continue;
        total += (uint64_t)*e.count;
        total_w += (uint64_t)*e.count * e.s.item_w;
        max_w = std::max<uint32_t>(max_w, (uint32_t)*e.count * e.s.item_w);
        ++n_recs;
    }
    if (total == 0) return RCF_OK;
    if (total_w > 0xffffffffull) { set_error("batched read of %llu items exceeds the 32-bit word range", (unsigned long long)total); return RCF_ECAP; }
    const size_t rec_bytes = ((size_t)n_recs * sizeof(GatherRec) + 255) & ~(size_t)255;
    const int rc = stage.ensure(rec_bytes + (size_t)total_w * 4, stream);
    if (rc != RCF_OK) return rc;
    GatherRec *recs = reinterpret_cast<GatherRec *>(stage.h);
    uint32_t at_w = 0, k = 0;
    for (size_t i = 0; i < n; ++i) {
        const ReadEntry &e = es[i];
        if (!e.s.ring || *e.count == 0) continue;
        recs[k++] = gather_rec(e.s, *e.count, at_w, 0u, ~0u, e.gain);
        at_w += (uint32_t)*e.count * e.s.item_w;
    }
    launch_gather_rings(reinterpret_cast<const GatherRec *>(stage.d), (int)n_recs, reinterpret_cast<uint32_t *>(stage.d + rec_bytes),
                        max_w, stream);
    if (hipStreamSynchronize(stream) != hipSuccess) { set_error("stream sync failed"); return RCF_EHIP; }
    for (size_t j = 0; j < n_idle; ++j) free_graveyard_idle(idle[j]);   // retuned / closed channels' old buffers
    const unsigned char *src = stage.h + rec_bytes;
    for (size_t i = 0; i < n; ++i) {
        const ReadEntry &e = es[i];
        if (!e.s.ring || *e.count == 0) continue;
        const size_t bytes = (size_t)*e.count * e.s.item_w * 4;
        std::memcpy(e.out, src, bytes);
        src += bytes;
        *e.s.cursor += *e.count;
    }
    return RCF_OK;
}

int64_t read_one(rcf_t *h, const RingStream &s, float gain, void *out, size_t max_items)
{
    int64_t n = 0;
    ReadEntry e{s, nullptr, gain, out, (int64_t)max_items, &n};
    const int rc = host_read(h->host_stage, h->stream, &h, 1, &e, 1);
    return rc != RCF_OK ? rc : n;
}

int read_many(PinnedStage &stage, hipStream_t stream, rcf_t *const *hs, size_t n_hs, const int *ms, const int *chan_ids, int n,
              int what, float gain, void *out, size_t cap_each, int64_t *counts)
{
    const size_t row = cap_each * (what == RCF_READ_FM ? sizeof(float) : sizeof(float2));
    std::vector<ReadEntry> es((size_t)n);
    for (int i = 0; i < n; ++i) {
        ReadEntry &e = es[(size_t)i];
        e.count = &counts[i];
        const int m = ms ? ms[i] : 0;
        if (m < 0 || (size_t)m >= n_hs) { counts[i] = RCF_EINVAL; continue; }
        auto f = hs[m]->chans.find(chan_ids[i]);
        if (f == hs[m]->chans.end()) { counts[i] = RCF_ENOCHAN; continue; }
        e.c = f->second.get();
        counts[i] = chan_stream(hs[m], e.c, what, &e.s);       // RCF_ESTATE: no such stream on this channel
        e.gain = what == RCF_READ_FM ? gain : 1.0f;
        e.out = static_cast<unsigned char *>(out) + (size_t)i * row;
        e.max = (int64_t)cap_each;
    }
    return host_read(stage, stream, hs, n_hs, es.data(), es.size());
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
        const int ks = bin < p.NB / 2 ? bin : bin - p.NB;
        const double f_k = (double)ks * h->fs / p.NB;
        const float fwT0 = (float)(kTwoPi * f_k / h->fs);
        const float a = -fwT0 * (float)p.D;
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
        c->angle0 = (long double)cphase +
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

#define FIND_CHAN(h, id, c)                                                 \
    auto it_ = (h)->chans.find(id);                                         \
    if (it_ == (h)->chans.end()) { set_error("no such channel %d", id); return RCF_ENOCHAN; } \
    Chan *c = it_->second.get()

// a single reader of a channel stream
static int64_t chan_read_one(rcf_t *h, int chan_id, int kind, float gain, void *out, size_t max_items)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    RingStream s;
    const int rc = chan_stream(h, c, kind, &s);
    return rc != RCF_OK ? rc : read_one(h, s, gain, out, max_items);
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
    return c->produced;
}

int64_t rcf_chan_start(rcf_t *h, int chan_id)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    FIND_CHAN(h, chan_id, c);
    return c->start_sample;
}

int64_t rcf_chan_read_iq(rcf_t *h, int chan_id, float *out, size_t max_samples)
{
    return chan_read_one(h, chan_id, RCF_READ_IQ, 1.0f, out, max_samples);
}

int64_t rcf_chan_read_fm(rcf_t *h, int chan_id, float gain, float *out, size_t max_samples)
{
    return chan_read_one(h, chan_id, RCF_READ_FM, gain, out, max_samples);
}

int rcf_chan_read_many(rcf_t *h, int what, const int *chan_ids, int n_chans, float gain, void *out, size_t cap_each,
                       int64_t *counts)
{
    if (!h || !chan_ids || !out || !counts || n_chans < 0 || (what != RCF_READ_IQ && what != RCF_READ_FM && what != RCF_READ_AGC)) {
        set_error("bad batched read arguments");
        return RCF_EINVAL;
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    return read_many(h->host_stage, h->stream, &h, 1, nullptr, chan_ids, n_chans, what, gain, out, cap_each, counts);
}

int rcf_chan_fm_filter(rcf_t *h, int chan_id, float gain, const float *taps, int ntaps)
{
    if (!h || !taps || ntaps < 1 || ntaps > 4096) { set_error("bad fm filter arguments"); return RCF_EINVAL; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if ((size_t)ntaps * 2 > h->out_cap) { set_error("ring too small for %d taps", ntaps); return RCF_ECAP; }
    float *fresh = nullptr;
    RCF_HIP(hipMalloc(&fresh, sizeof(float) * (size_t)ntaps));
    RCF_HIP(hipMemcpy(fresh, taps, sizeof(float) * (size_t)ntaps, hipMemcpyHostToDevice));
    bury(h, c->d_symtaps);
    c->d_symtaps = fresh;
    c->sym_ntaps = ntaps;
    c->sym_gain = gain;
    ++h->chans_epoch;
    if (!c->d_sym) {
        RCF_HIP(hipMalloc(&c->d_sym, sizeof(float) * h->out_cap));
        RCF_HIP(hipMemsetAsync(c->d_sym, 0, sizeof(float) * h->out_cap, h->stream));
        c->sym_from = c->produced;      // a new GR block starts with zero history
        c->rd_sym = c->produced;
    }
    return RCF_OK;
}

int64_t rcf_chan_read_sym(rcf_t *h, int chan_id, float *out, size_t max_samples)
{
    return chan_read_one(h, chan_id, kReadSym, 1.0f, out, max_samples);
}

int rcf_chan_agc(rcf_t *h, int chan_id, int nsamples, float reference)
{
    if (!h || nsamples < 0 || nsamples > 4096 || !std::isfinite(reference)) { set_error("bad AGC arguments"); return RCF_EINVAL; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (nsamples == 0) {                // off: the ring goes once the stream has passed it
        if (c->d_agc) {
            bury(h, c->d_agc);
            c->d_agc = nullptr;
            c->agc_n = 0;
            ++h->chans_epoch;
        }
        return RCF_OK;
    }
    if (c->fm_only) { set_error("channel %d exposes its discriminator only: the AGC reads IQ", chan_id); return RCF_ESTATE; }
    if ((size_t)nsamples * 2 > h->out_cap) { set_error("ring of %zu too small for a %d-sample AGC window", h->out_cap, nsamples); return RCF_ECAP; }
    if (!c->d_agc) {
        RCF_HIP(hipMalloc(&c->d_agc, sizeof(float2) * h->out_cap));
        RCF_HIP(hipMemsetAsync(c->d_agc, 0, sizeof(float2) * h->out_cap, h->stream));
    }
    c->agc_n = nsamples;
    c->agc_ref = reference;
    c->agc_from = c->produced;          // a new GR block starts with zero history
    c->rd_agc = c->produced;
    ++h->chans_epoch;
    return RCF_OK;
}

int64_t rcf_chan_read_agc(rcf_t *h, int chan_id, float *out, size_t max_samples)
{
    return chan_read_one(h, chan_id, RCF_READ_AGC, 1.0f, out, max_samples);
}

int rcf_chan_agc_ring(rcf_t *h, int chan_id, void **agc_ring, size_t *capacity)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;                  // (zero-copy readers order themselves on rcf_stream: nothing stays deferred)
    FIND_CHAN(h, chan_id, c);
    RingStream s;
    const int rc = chan_stream(h, c, RCF_READ_AGC, &s);
    if (rc != RCF_OK) return rc;
    if (agc_ring) *agc_ring = const_cast<void *>(s.ring);
    if (capacity) *capacity = h->out_cap;
    return RCF_OK;
}

// ---- clock_recovery_mm_ff behind the discriminator (clock.hip)
static int clock_state(rcf_t *h, Chan *c, ClockState *st)
{
    RCF_HIP(hipMemcpyAsync(st, c->d_clk + h->out_cap, sizeof(*st), hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipStreamSynchronize(h->stream));
    return RCF_OK;
}

int rcf_chan_clock_mm(rcf_t *h, int chan_id, const rcf_clock_mm_params_t *p)
{
    if (!h) return RCF_EINVAL;
    if (p) {
        if (!std::isfinite(p->gain) || !std::isfinite(p->omega) || !std::isfinite(p->gain_omega) || !std::isfinite(p->mu) ||
            !std::isfinite(p->gain_mu) || !std::isfinite(p->omega_relative_limit)) {
            set_error("clock recovery: non-finite parameter");
            return RCF_EINVAL;
        }
        // GNU Radio's documented domain (omega stays >= 2 samples per symbol at its lower limit); mu selects a row of the bank
        if ((double)p->omega * (1.0 - (double)p->omega_relative_limit) < 2.0 || p->omega > 4096.f || p->mu < 0.f || p->mu > 1.f) {
            set_error("clock recovery: omega %g (relative limit %g) outside 2 / (1 - limit) .. 4096, or mu %g outside 0 .. 1",
                      p->omega, p->omega_relative_limit, p->mu);
            return RCF_EINVAL;
        }
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!p) {                           // off: ring, state and bank go once the stream has passed them
        if (c->d_clk) {
            bury(h, c->d_clk);
            c->d_clk = nullptr;
            c->d_clk_taps = nullptr;
            ++h->chans_epoch;
        }
        return RCF_OK;
    }
    if ((size_t)kClockTaps * 2 > h->out_cap) { set_error("ring of %zu too small for the clock's %d-sample window", h->out_cap, kClockTaps); return RCF_ECAP; }
    constexpr size_t kBank = (size_t)(kClockSteps + 1) * kClockTaps;
    if (!p->interp_taps && !h->d_mmse) {
        const std::vector<float> t = design_mmse_interpolator(kClockTaps, kClockSteps, 0.25);
        float *d = nullptr;
        RCF_HIP(hipMalloc(&d, sizeof(float) * kBank));
        if (!hip_ok(hipMemcpy(d, t.data(), sizeof(float) * kBank, hipMemcpyHostToDevice), "hipMemcpy(interpolator bank)")) { (void)hipFree(d); return RCF_EHIP; }
        h->d_mmse = d;
    }
    // every call is a new GR block: a fresh ring and state (symbol 0 is the first of this call), zero history
    const size_t state_at = h->out_cap, bank_at = h->out_cap + 64;       // in floats; the state record has 256 bytes to itself
    float *fresh = nullptr;
    RCF_HIP(hipMalloc(&fresh, sizeof(float) * (bank_at + (p->interp_taps ? kBank : 0))));
    Chan::ClockMm k;
    k.gain = p->gain; k.mu0 = p->mu; k.omega_mid = p->omega;
    k.omega_lim = k.omega_mid * p->omega_relative_limit;                 // (one float product)
    k.gain_omega = p->gain_omega; k.gain_mu = p->gain_mu;
    k.adv0 = (int)std::ceil(k.omega_mid);
    ClockState st0{};
    st0.p = c->produced - (kClockTaps - 1);                              // the first window: seven zeros and u[first]
    st0.mu = k.mu0; st0.omega = k.omega_mid; st0.last = 0.f;
    if (!hip_ok(hipMemcpy(fresh + state_at, &st0, sizeof(st0), hipMemcpyHostToDevice), "hipMemcpy(clock state)") ||
        (p->interp_taps && !hip_ok(hipMemcpy(fresh + bank_at, p->interp_taps, sizeof(float) * kBank, hipMemcpyHostToDevice), "hipMemcpy(interpolator bank)"))) {
        (void)hipFree(fresh);
        return RCF_EHIP;
    }
    bury(h, c->d_clk);
    c->d_clk = fresh;
    c->d_clk_taps = p->interp_taps ? fresh + bank_at : h->d_mmse;
    c->clk = k;
    c->clk_from = c->produced;
    c->rd_clk = 0;
    ++h->chans_epoch;
    return RCF_OK;
}

int rcf_chan_clock_produced(rcf_t *h, int chan_id, int64_t *n_symbols, int64_t *n_slips)
{
    if (!h || !n_symbols) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->d_clk) { set_error("channel %d has no symbol clock", chan_id); return RCF_ESTATE; }
    ClockState st{};
    const int rc = clock_state(h, c, &st);
    if (rc != RCF_OK) return rc;
    *n_symbols = st.n_out;
    if (n_slips) *n_slips = st.slips;
    return RCF_OK;
}

int64_t rcf_chan_read_clock(rcf_t *h, int chan_id, float *out, size_t max_symbols)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->d_clk) { set_error("channel %d has no symbol clock", chan_id); return RCF_ESTATE; }
    ClockState st{};
    const int rc = clock_state(h, c, &st);
    if (rc != RCF_OK) return rc;
    return read_one(h, RingStream{h, c->d_clk, 1u, 0u, st.n_out, st.n_out, &c->rd_clk}, 1.0f, out, max_symbols);
}

int rcf_chan_clock_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;                  // (zero-copy readers order themselves on rcf_stream: nothing stays deferred)
    FIND_CHAN(h, chan_id, c);
    if (!c->d_clk) { set_error("channel %d has no symbol clock", chan_id); return RCF_ESTATE; }
    if (sym_ring) *sym_ring = c->d_clk;
    if (capacity) *capacity = h->out_cap;
    return RCF_OK;
}

int rcf_chan_audio_open(rcf_t *h, int chan_id, const rcf_audio_params_t *p)
{
    if (!h || !p || !p->lpf_taps || !p->hpf_taps || !p->rs_taps || p->n_lpf < 1 || p->n_hpf < 1 || p->n_rs < 1 ||
        p->interpolation < 1 || p->decimation < 1 || p->deemph_a[0] == 0.0) {
        set_error("bad audio chain arguments");
        return RCF_EINVAL;
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (c->fm_only) { set_error("channel %d exposes its discriminator only: the voice chain reads IQ", chan_id); return RCF_ESTATE; }
    const int I = p->interpolation;
    const int n_rs_pad = (p->n_rs + I - 1) / I * I;              // rational_resampler_base: pad to a multiple of I
    const size_t reach = (size_t)std::max(std::max(p->n_lpf, p->n_hpf), n_rs_pad / I);
    if (reach * 2 > h->out_cap) { set_error("ring of %zu too small for %zu-tap audio filters", h->out_cap, reach); return RCF_ECAP; }
    std::unique_ptr<Chan::Audio> au(new Chan::Audio);
    au->n_lpf = p->n_lpf; au->n_hpf = p->n_hpf; au->nt_rs = n_rs_pad / I;
    au->interp = I; au->decim = p->decimation;
    au->gain = p->quad_gain;
    au->thr = std::pow(10.0, p->squelch_db / 10);                // pwr_squelch_cc::set_threshold
    au->alpha = p->squelch_alpha;
    // iir_filter(fftaps, fbtaps, oldstyle = false): feedback taps are negated, a[0] must be 1
    au->b0 = p->deemph_b[0]; au->b1 = p->deemph_b[1]; au->fb1 = -p->deemph_a[1];
    std::vector<float> taps((size_t)p->n_lpf + p->n_hpf + n_rs_pad, 0.0f);
    std::memcpy(taps.data(), p->lpf_taps, sizeof(float) * (size_t)p->n_lpf);
    std::memcpy(taps.data() + p->n_lpf, p->hpf_taps, sizeof(float) * (size_t)p->n_hpf);
    std::memcpy(taps.data() + p->n_lpf + p->n_hpf, p->rs_taps, sizeof(float) * (size_t)p->n_rs);
    RCF_HIP(hipMalloc(&au->d_taps, sizeof(float) * taps.size()));
    RCF_HIP(hipMemcpy(au->d_taps, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice));
    RCF_HIP(hipMalloc(&au->d_rings, sizeof(float) * 6 * h->out_cap));
    RCF_HIP(hipMemsetAsync(au->d_rings, 0, sizeof(float) * 6 * h->out_cap, h->stream));
    AudioState st0{};
    st0.muted = 1;                                               // squelch_base_cc starts in ST_MUTED
    RCF_HIP(hipMalloc(&au->d_state, sizeof(AudioState)));
    RCF_HIP(hipMemcpy(au->d_state, &st0, sizeof(st0), hipMemcpyHostToDevice));
    au->from = c->produced;                                      // a new flowgraph: zero state from here on
    if (c->audio) { bury(h, c->audio->d_state); bury(h, c->audio->d_rings); bury(h, c->audio->d_taps); }
    c->audio = std::move(au);
    ++h->chans_epoch;
    return RCF_OK;
}

int rcf_chan_audio_close(rcf_t *h, int chan_id)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (c->audio) { bury(h, c->audio->d_state); bury(h, c->audio->d_rings); bury(h, c->audio->d_taps); c->audio.reset(); }
    ++h->chans_epoch;
    return RCF_OK;
}

static int audio_counts(rcf_t *h, Chan *c, int64_t *n_audio, int64_t *n_ungated)
{
    AudioState st{};
    RCF_HIP(hipMemcpyAsync(&st, c->audio->d_state, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipStreamSynchronize(h->stream));
    const int64_t I = c->audio->interp, D = c->audio->decim;
    *n_ungated = st.n_a;
    *n_audio = (st.n_a * I + D - 1) / D;
    return RCF_OK;
}

int rcf_chan_audio_produced(rcf_t *h, int chan_id, int64_t *n_audio, int64_t *n_ungated)
{
    if (!h || !n_audio) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->audio) { set_error("channel %d has no audio chain", chan_id); return RCF_ESTATE; }
    int64_t a = 0, u = 0;
    const int rc = audio_counts(h, c, &a, &u);
    if (rc != RCF_OK) return rc;
    *n_audio = a;
    if (n_ungated) *n_ungated = u;
    return RCF_OK;
}

int64_t rcf_chan_read_audio(rcf_t *h, int chan_id, float *out, size_t max_samples)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->audio) { set_error("channel %d has no audio chain", chan_id); return RCF_ESTATE; }
    int64_t a = 0, u = 0;
    const int rc = audio_counts(h, c, &a, &u);
    if (rc != RCF_OK) return rc;
    return read_one(h, RingStream{h, c->audio->d_rings + 3 * h->out_cap, 1u, 0u, a, a, &c->audio->rd}, 1.0f, out, max_samples);
}

int rcf_chan_fm_level(rcf_t *h, int chan_id, float gain, int window, float *level)
{
    if (!h || !level || window < 1) { set_error("bad fm level arguments"); return RCF_EINVAL; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if ((size_t)window > h->out_cap) { set_error("window %d exceeds the ring", window); return RCF_ECAP; }
    if (!h->d_level) RCF_HIP(hipMalloc(&h->d_level, sizeof(float)));
    launch_fm_level(c->d_fm, c->produced, window, gain, h->ring_mask, h->d_level, h->stream);
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
        if (c->d_agc) { set_error("channel %d carries an AGC, which reads its IQ stream", chan_id); return RCF_ESTATE; }
        for (auto &kv : h->chans)
            if (kv.second->src == chan_id) { set_error("channel %d reads channel %d's IQ stream", kv.first, chan_id); return RCF_ESTATE; }
    } else if (c->fm_only) {
        c->rd_iq = c->produced;                  // what lies behind was never written
    }
    if ((on != 0) != c->fm_only && c->produced > 0) {
        // The newest ring sample is the "output before" of the next block's first discriminator sample, and the two modes
        // keep it differently: rotated by the channel's rotator (ordinary tap) or as the bare bin (discriminator only: that
        // path never rotates, it turns the conjugate product by the rotator's increment instead).  Convert the one sample,
        // so that no discriminator sample straddles two conventions.  Only its angle matters to the discriminator.
        RCF_HIP(hipStreamSynchronize(h->stream));
        float2 *at = c->d_iq + ((uint64_t)(c->produced - 1) & h->ring_mask);
        float2 v;
        RCF_HIP(hipMemcpy(&v, at, sizeof(v), hipMemcpyDeviceToHost));
        const long double ang = c->angle0 + (long double)(c->produced - 1 - c->n_seg0) * (long double)c->dangle;
        const double pr = std::cos((double)ang), pi = (on ? -1.0 : 1.0) * std::sin((double)ang);
        const float2 w = make_float2((float)(v.x * pr - v.y * pi), (float)(v.x * pi + v.y * pr));
        RCF_HIP(hipMemcpy(at, &w, sizeof(w), hipMemcpyHostToDevice));
    }
    c->fm_only = on != 0;
    return RCF_OK;
}

int rcf_chan_rings(rcf_t *h, int chan_id, void **iq_ring, void **fm_ring, size_t *capacity)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;                  // (zero-copy readers order themselves on rcf_stream: nothing stays deferred)
    FIND_CHAN(h, chan_id, c);
    RingStream s;
    if (iq_ring) {
        const int rc = chan_stream(h, c, RCF_READ_IQ, &s);
        if (rc != RCF_OK) return rc;
        *iq_ring = const_cast<void *>(s.ring);
    }
    if (fm_ring) *fm_ring = c->d_fm;
    if (capacity) *capacity = h->out_cap;
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
