// rcf_stage.cpp -- the optional stages behind a channel's rings (the records of Chan, rcf_state.h): the P25 symbol filter,
// the feed-forward AGC, the SmartNet / EDACS symbol clock, the P25 CQPSK Gardner / Costas loop, the P25 C4FM symbol loop and
// the analog voice chain, the slicer behind one of the loops and the frame decoder behind the slicer (P25 trunking blocks,
// EDACS control frames, SmartNet OSWs or P25 voice data units), the carrier detector and the carrier-operated capture over the IQ
// stream.
// Attach, off, and what they produced.
// An attach function allocates into Fresh<> holders and builds the new record completely; only then is it swapped into
// the channel and the old one released.  A HIP call that fails before that leaves the channel as it was.
// The three symbol loops share their record (Chan::Loop) and one attach path, attach_loop: an entry point validates its
// parameters, checks what the loop reads and the ring's size, and fills in its own constants and initial state.
// The four frame decoders likewise: one record (Slicer::Frames), one attach path, attach_frames, and one state path,
// frames_state; an entry point brings what it asks of the slicer and its own lines of the initial state.
#include "rcf_plan.h"
#define RCF_DEVFN static inline
#define RCF_DEVCONST static const
#include "tsbk_core.hpp"       // (kTsbkNoFrame, kTsbkRecWords)
#include "edacs_core.hpp"      // (kEdacsNoFrame, kEdacsRecWords; slice_sync_both_ok of slice_core.hpp)
#include "osw_core.hpp"        // (kOswSyncBits, kOswRecWords)
#include "p25lc_core.hpp"      // (kP25lcRecWords, kP25lcFlagCorrect)
#include "nid_core.hpp"        // (kNidFlagBch)
#include "squelch_core.hpp"    // (squelch_threshold)
#include "capture_core.hpp"    // (kCaptureRecWords, CaptureRec)
static_assert(rcfx::kP25lcFlagEs == RCF_P25LC_ES << 1 && rcfx::kP25lcFlagErasures == RCF_P25LC_ERASURES << 1, "the options travel in P25lcLaunch::flags behind kP25lcFlagCorrect");

namespace rcfx {

void Chan::Sym::release(rcf_t *h) { bury(h, rec.sym_ring); bury(h, const_cast<float *>(rec.taps)); rec.sym_ring = nullptr; rec.taps = nullptr; }
void Chan::Agc::release(rcf_t *h) { bury(h, rec.agc_ring); rec.agc_ring = nullptr; }
template <class R> static void release_frames(rcf_t *h, std::unique_ptr<R> &f) { if (f) { bury(h, f->rec.rec_ring); f.reset(); } }     // one allocation
void Chan::Slicer::release(rcf_t *h)                 // one allocation; the frame decoder goes with its slicer
{
    for_each_frames([h](auto &f) { release_frames(h, f); });
    bury(h, rec.word_ring);
    rec = SliceLaunch{};
}
void Chan::Squelch::release(rcf_t *h) { bury(h, rec.st); rec = SquelchLaunch{}; }
void Chan::Capture::release(rcf_t *h) { bury(h, rec.cap_ring); rec = CaptureLaunch{}; }       // one allocation
void Chan::Audio::release(rcf_t *h) { bury(h, rec.st); bury(h, rec.a_ring); bury(h, const_cast<float *>(rec.lpf)); rec = AudioLaunch{}; }

}  // namespace rcfx

using namespace rcfx;

// a stage switched off: nothing to do when the channel has none
template <class R> static int stage_off(rcf_t *h, std::unique_ptr<R> &stage)
{
    if (stage) { drop_stage(h, stage); ++h->chans_epoch; }
    return RCF_OK;
}

// A slicer reads the ring and the counter of ONE loop: when that loop goes, or starts again with a fresh ring at symbol 0,
// the slicer goes with it (rcf.h says so: the caller attaches it again behind the new loop)
template <class R> static void detach_slicer_of(rcf_t *h, Chan *c)
{
    if (c->slicer && c->slicer->source == R::kWhat) drop_stage(h, c->slicer);
}
template <class R> static int loop_off(rcf_t *h, Chan *c, std::unique_ptr<R> &stage)
{
    detach_slicer_of<R>(h, c);
    return stage_off(h, stage);
}

// the interpolator bank the symbol clocks, the Gardner / Costas loops and the C4FM loops share unless the caller brings one: built at first use
static int default_bank(rcf_t *h)
{
    if (h->d_mmse) return RCF_OK;
    constexpr size_t kBank = (size_t)(kClockSteps + 1) * kClockTaps;
    const std::vector<float> t = design_mmse_interpolator(kClockTaps, kClockSteps, 0.25);
    Fresh<float> d;
    RCF_HIP(d.alloc(kBank));
    if (!hip_ok(hipMemcpy(d.p, t.data(), sizeof(float) * kBank, hipMemcpyHostToDevice), "hipMemcpy(interpolator bank)")) return RCF_EHIP;
    h->d_mmse = d.take();
    return RCF_OK;
}

// What attaching a symbol loop comes to once its entry point has built the record k (its constants) and the initial state:
// one allocation -- soft-symbol ring of out_cap floats | the state record, in a slot of whole 256 bytes | the caller's bank,
// if any (out_cap is a power of two: the record's 64-bit fields are aligned) --, the two copies, and the swap.  Every call
// is a new block: a fresh ring and state (symbol 0 is the first of this call), zero history before the channel's next output.
template <class R>
static int attach_loop(rcf_t *h, Chan *c, std::unique_ptr<R> &stage, std::unique_ptr<R> k, const typename R::State &st0,
                       const float *interp_taps, const char *state_copy)
{
    constexpr size_t kBank = (size_t)(kClockSteps + 1) * kClockTaps;
    constexpr size_t kStateFloats = (sizeof(typename R::State) + 255) / 256 * 256 / sizeof(float);
    if (!interp_taps) { const int rc = default_bank(h); if (rc != RCF_OK) return rc; }
    const size_t state_at = h->out_cap, bank_at = state_at + kStateFloats;       // in floats
    Fresh<float> fresh;
    RCF_HIP(fresh.alloc(bank_at + (interp_taps ? kBank : 0)));
    if (!hip_ok(hipMemcpy(fresh.p + state_at, &st0, sizeof(st0), hipMemcpyHostToDevice), state_copy) ||
        (interp_taps && !hip_ok(hipMemcpy(fresh.p + bank_at, interp_taps, sizeof(float) * kBank, hipMemcpyHostToDevice), "hipMemcpy(interpolator bank)")))
        return RCF_EHIP;
    k->ring() = fresh.take();
    k->rec.st = reinterpret_cast<typename R::State *>(k->ring() + state_at);
    k->rec.taps = interp_taps ? k->ring() + bank_at : h->d_mmse;
    k->from = c->pos.produced;
    detach_slicer_of<R>(h, c);
    drop_stage(h, stage);
    stage = std::move(k);
    ++h->chans_epoch;
    return RCF_OK;
}

// What attaching a frame decoder R behind the slicer comes to; its entry point brings slicer_ok, what it asks of the slicer
// and of what else it carries (else RCF_ESTATE with `refusal`), and init, its own lines of the launch record and of the initial state.  p == nullptr: off.
// One allocation -- record ring of cap records | the state record, in a slot of 256 bytes (cap >= 16: the state's 64-bit
// fields are aligned) --, one copy, and the swap.  Every call is a new stream: a fresh ring and state, cursor 0; the first
// hit is the slicer's count as of everything queued (one round trip), which `now` hands to init as well.
template <class R, class P, class Ok, class Init>
static int attach_frames(rcf_t *h, int chan_id, const P *p, Ok &&slicer_ok, const char *refusal, Init &&init)
{
    if (!h) return RCF_EINVAL;
    int cap = 256;
    if (p) {
        if (p->capacity) cap = p->capacity;
        if (cap < 16 || cap > (1 << 20) || (cap & (cap - 1))) { set_error("%s stage: capacity %d is not a power of two 16 .. 2^20", R::kName, p->capacity); return RCF_EINVAL; }
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!p) {
        if (c->slicer && c->slicer->frames<R>()) { release_frames(h, c->slicer->frames<R>()); ++h->chans_epoch; }
        return RCF_OK;
    }
    if (!c->slicer || !slicer_ok(*c->slicer)) { set_error(refusal, chan_id); return RCF_ESTATE; }
    const SliceLaunch &sl = c->slicer->rec;
    std::unique_ptr<R> k(new R);
    typename R::Launch &r = k->rec;
    r.src = sl.st;
    r.word_ring = sl.word_ring; r.hit_ring = sl.hit_ring;
    r.word_mask = sl.word_mask; r.hit_mask = sl.hit_mask; r.rec_mask = (uint32_t)cap - 1;
    k->cap = (uint32_t)cap;
    k->serial = next_stage_serial();
    SliceState now{};
    const int rc = stage_state(h, sl.st, &now, offsetof(SliceState, partial));
    if (rc != RCF_OK) return rc;
    typename R::State st0{};
    st0.next_hit = now.n_hits;
    init(r, st0, sl, now);
    constexpr size_t kStateWords = 256 / sizeof(uint32_t);
    static_assert(sizeof(typename R::State) <= 256, "the state's slot");
    const size_t state_at = (size_t)cap * read_row(R::kKind).item_w;       // in words
    Fresh<uint32_t> fresh;
    RCF_HIP(fresh.alloc(state_at + kStateWords));
    char state_copy[32];
    snprintf(state_copy, sizeof(state_copy), "hipMemcpy(%s state)", R::kName);
    if (!hip_ok(hipMemcpy(fresh.p + state_at, &st0, sizeof(st0), hipMemcpyHostToDevice), state_copy)) return RCF_EHIP;
    r.rec_ring = fresh.take();
    r.st = reinterpret_cast<typename R::State *>(r.rec_ring + state_at);
    release_frames(h, c->slicer->frames<R>());
    c->slicer->frames<R>() = std::move(k);
    ++h->chans_epoch;
    return RCF_OK;
}
static_assert(read_row(kTsbk).item_w == kTsbkRecWords && read_row(kEdacs).item_w == kEdacsRecWords && read_row(kOsw).item_w == kOswRecWords &&
              read_row(kP25lc).item_w == kP25lcRecWords,
              "the stream table's words per record are the kernels'");

// the decoder's counters -- its state record up to next_hit -- as of everything queued; refused as its stream is
template <class R, class Out>
static int frames_state(rcf_t *h, int chan_id, const Out *out, typename R::State *st)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->slicer || !c->slicer->frames<R>()) { set_error(read_row(R::kKind).refusal, chan_id); return RCF_ESTATE; }
    return stage_state(h, c->slicer->frames<R>()->rec.st, st, offsetof(typename R::State, next_hit));
}

extern "C" {

int rcf_chan_fm_filter(rcf_t *h, int chan_id, float gain, const float *taps, int ntaps)
{
    if (!h || !taps || ntaps < 1 || ntaps > 4096) { set_error("bad fm filter arguments"); return RCF_EINVAL; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if ((size_t)ntaps * 2 > h->out_cap) { set_error("ring too small for %d taps", ntaps); return RCF_ECAP; }
    Fresh<float> d_taps, d_ring;
    RCF_HIP(d_taps.alloc((size_t)ntaps));
    RCF_HIP(hipMemcpy(d_taps.p, taps, sizeof(float) * (size_t)ntaps, hipMemcpyHostToDevice));
    if (!c->sym) {
        RCF_HIP(d_ring.alloc(h->out_cap));
        RCF_HIP(hipMemsetAsync(d_ring.p, 0, sizeof(float) * h->out_cap, h->stream));
        c->sym.reset(new Chan::Sym);
        c->sym->rec.fm_ring = c->d_fm;
        c->sym->rec.sym_ring = d_ring.take();
        c->sym->from = c->sym->rec.n_first = c->sym->rd = c->pos.produced;     // a new GR block starts with zero history
    }
    FmFirLaunch &rec = c->sym->rec;
    bury(h, const_cast<float *>(rec.taps));          // a second call: new taps and gain from the next block on, nothing else
    rec.taps = d_taps.take();
    rec.ntaps = ntaps;
    rec.gain = gain;
    ++h->chans_epoch;
    return RCF_OK;
}

int rcf_chan_agc(rcf_t *h, int chan_id, int nsamples, float reference)
{
    if (!h || nsamples < 0 || nsamples > 4096 || !std::isfinite(reference)) { set_error("bad AGC arguments"); return RCF_EINVAL; }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (nsamples == 0) {                // off
        if (c->costas) { set_error("channel %d: the Gardner / Costas stage reads the AGC (switch it off first)", chan_id); return RCF_ESTATE; }
        return stage_off(h, c->agc);
    }
    if (c->fm_only) { set_error("channel %d exposes its discriminator only: the AGC reads IQ", chan_id); return RCF_ESTATE; }
    if ((size_t)nsamples * 2 > h->out_cap) { set_error("ring of %zu too small for a %d-sample AGC window", h->out_cap, nsamples); return RCF_ECAP; }
    if (!c->agc) {
        Fresh<float2> d_ring;
        RCF_HIP(d_ring.alloc(h->out_cap));
        RCF_HIP(hipMemsetAsync(d_ring.p, 0, sizeof(float2) * h->out_cap, h->stream));
        c->agc.reset(new Chan::Agc);
        c->agc->rec.iq_ring = c->d_iq;
        c->agc->rec.agc_ring = d_ring.take();
    }
    c->agc->rec.nsamples = nsamples;
    c->agc->rec.reference = reference;
    c->agc->from = c->agc->rec.n_first = c->agc->rd = c->pos.produced;         // a new GR block starts with zero history
    ++h->chans_epoch;
    return RCF_OK;
}

// ---- clock_recovery_mm_ff behind the discriminator (clock.hip)
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
    if (!p) return loop_off(h, c, c->clock);
    if ((size_t)kClockTaps * 2 > h->out_cap) { set_error("ring of %zu too small for the clock's %d-sample window", h->out_cap, kClockTaps); return RCF_ECAP; }
    std::unique_ptr<Chan::Clock> k(new Chan::Clock);
    ClockLaunch &r = k->rec;                                             // the constants as the kernel takes them, rounded to float once
    r.fm_ring = c->d_fm;
    r.n_first = c->pos.produced;                                         // (== Loop::from: attach_loop)
    r.gain = p->gain; r.mu0 = p->mu; r.omega_mid = p->omega;
    r.omega_lim = r.omega_mid * p->omega_relative_limit;                 // (one float product)
    r.gain_omega = p->gain_omega; r.gain_mu = p->gain_mu;
    r.adv0 = (int)std::ceil(r.omega_mid);
    ClockState st0{};
    st0.p = c->pos.produced - (kClockTaps - 1);                          // the first window: seven zeros and u[first]
    st0.mu = r.mu0; st0.omega = r.omega_mid; st0.last = 0.f;
    return attach_loop(h, c, c->clock, std::move(k), st0, p->interp_taps, "hipMemcpy(clock state)");
}

// ---- Gardner / Costas symbol recovery behind the AGC (costas.hip)
int rcf_chan_costas(rcf_t *h, int chan_id, const rcf_costas_params_t *p)
{
    if (!h) return RCF_EINVAL;
    if (p) {
        const float v[7] = {p->omega, p->gain_mu, p->gain_omega, p->alpha, p->beta, p->max_freq, p->omega_limit};
        for (float x : v)
            if (!std::isfinite(x)) { set_error("Gardner / Costas: non-finite parameter"); return RCF_EINVAL; }
        // mu > 1 after every symbol (the loop consumes at least one input per symbol) and both windows inside 32 samples
        if (p->omega < 2.f || p->omega > 16.f || p->omega_limit < 0.f || p->max_freq < 0.f || (double)p->max_freq >= kTwoPi / 2 ||
            (double)p->omega - (double)p->omega_limit - (double)p->gain_mu < 2.0) {
            set_error("Gardner / Costas: omega %g outside 2 .. 16, omega - omega_limit %g - gain_mu %g < 2, a negative limit, or max_freq %g outside 0 .. pi",
                      p->omega, p->omega_limit, p->gain_mu, p->max_freq);
            return RCF_EINVAL;
        }
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!p) return loop_off(h, c, c->costas);
    if (!c->agc) { set_error("channel %d has no AGC for the Gardner / Costas stage to read", chan_id); return RCF_ESTATE; }
    if (h->out_cap < 64) { set_error("ring of %zu too small for the Gardner / Costas stage", h->out_cap); return RCF_ECAP; }
    std::unique_ptr<Chan::Costas> k(new Chan::Costas);
    CostasLaunch &r = k->rec;
    r.agc_ring = c->agc->rec.agc_ring;                                   // (the AGC keeps its ring on a re-call and cannot go before this stage: rcf_chan_agc)
    r.omega_mid = p->omega; r.omega_lim = p->omega_limit; r.gain_omega = p->gain_omega; r.gain_mu = p->gain_mu;
    r.alpha = p->alpha; r.beta = p->beta; r.max_freq = p->max_freq;
    r.window = std::max(2 * (int)std::ceil(r.omega_mid), (int)std::floor(r.omega_mid / 2) + 9);
    CostasState st0{};
    st0.mu = st0.omega = r.omega_mid;
    return attach_loop(h, c, c->costas, std::move(k), st0, p->interp_taps, "hipMemcpy(Gardner / Costas state)");
}

int rcf_chan_costas_state(rcf_t *h, int chan_id, rcf_costas_state_t *out)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->costas) { set_error("channel %d has no Gardner / Costas stage", chan_id); return RCF_ESTATE; }
    CostasState st{};                   // (its front, not the history behind it)
    const int rc = stage_state(h, c->costas->rec.st, &st, offsetof(CostasState, hist));
    if (rc != RCF_OK) return rc;
    out->n_symbols = st.n_out; out->n_slips = st.slips;
    out->mu = st.mu; out->omega = st.omega; out->freq = st.freq; out->phase = st.phase;
    return RCF_OK;
}

// ---- op25 fsk4_demod_ff behind the symbol filter (fsk4.hip)
int rcf_chan_fsk4(rcf_t *h, int chan_id, const rcf_fsk4_params_t *p)
{
    if (!h) return RCF_EINVAL;
    if (p) {
        const double v[8] = {p->sample_rate, p->symbol_rate, p->k_spread, p->k_timing, p->k_fine, p->k_coarse, p->spread_min, p->spread_max};
        for (double x : v)
            if (!std::isfinite(x)) { set_error("C4FM loop: non-finite parameter"); return RCF_EINVAL; }
        const double sps = p->sample_rate / p->symbol_rate;
        if (!(sps >= 2.0 && sps <= 4096.0) || !(p->spread_min > 0.0 && p->spread_min <= 2.0 && p->spread_max >= 2.0)) {
            set_error("C4FM loop: sample_rate %g / symbol_rate %g outside 2 .. 4096, or not 0 < spread_min %g <= 2 <= spread_max %g",
                      p->sample_rate, p->symbol_rate, p->spread_min, p->spread_max);
            return RCF_EINVAL;
        }
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!p) return loop_off(h, c, c->fsk4);
    if (!c->sym) { set_error("channel %d has no symbol filter (rcf_chan_fm_filter) for the C4FM loop to read", chan_id); return RCF_ESTATE; }
    if (h->out_cap < 16) { set_error("ring of %zu too small for the C4FM loop", h->out_cap); return RCF_ECAP; }
    std::unique_ptr<Chan::Fsk4> k(new Chan::Fsk4);
    Fsk4Launch &r = k->rec;
    r.sym_ring = c->sym->rec.sym_ring;                                   // (the symbol filter keeps its ring on a re-call and is never taken away)
    r.time = p->symbol_rate / p->sample_rate;
    r.k_spread = p->k_spread; r.k_timing = p->k_timing; r.k_fine = p->k_fine; r.k_coarse = p->k_coarse;
    r.spread_min = p->spread_min; r.spread_max = p->spread_max;
    Fsk4State st0{};
    st0.spread = 2.0;
    return attach_loop(h, c, c->fsk4, std::move(k), st0, p->interp_taps, "hipMemcpy(C4FM loop state)");
}

int rcf_chan_fsk4_state(rcf_t *h, int chan_id, rcf_fsk4_state_t *out)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->fsk4) { set_error("channel %d has no C4FM symbol loop (rcf_chan_fsk4)", chan_id); return RCF_ESTATE; }
    Fsk4State st{};
    const int rc = stage_state(h, c->fsk4->rec.st, &st, offsetof(Fsk4State, hist));
    if (rc != RCF_OK) return rc;
    out->n_symbols = st.n_out; out->n_slips = st.slips;
    out->clock = st.clock; out->spread = st.spread; out->fine = st.fine; out->coarse = st.coarse;
    return RCF_OK;
}

// ---- hard decisions behind one of the three loops (slice.hip)
int rcf_chan_slicer(rcf_t *h, int chan_id, const rcf_slicer_params_t *p)
{
    if (!h) return RCF_EINVAL;
    int bps = 0, hit_cap = 256;
    if (p) {
        if (p->source != RCF_READ_CLOCK && p->source != RCF_READ_COSTAS && p->source != RCF_READ_FSK4) {
            set_error("slicer: source %d is none of RCF_READ_CLOCK, RCF_READ_COSTAS, RCF_READ_FSK4", p->source);
            return RCF_EINVAL;
        }
        if (p->mode != RCF_SLICE_BINARY && p->mode != RCF_SLICE_FSK4) { set_error("slicer: unknown mode %d", p->mode); return RCF_EINVAL; }
        bps = p->mode == RCF_SLICE_BINARY ? 1 : 2;
        if (bps == 2)
            for (int i = 0; i < 4; ++i)
                if (!std::isfinite(p->levels[i]) || (i && p->levels[i] < p->levels[i - 1])) {
                    set_error("slicer: levels %g %g %g %g not finite or not non-decreasing", p->levels[0], p->levels[1], p->levels[2], p->levels[3]);
                    return RCF_EINVAL;
                }
        if (p->sync_bits != 0 && (p->sync_bits < 8 || p->sync_bits > 64 || p->sync_bits % bps)) {
            set_error("slicer: sync_bits %d is not 0 or 8 .. 64 and a multiple of %d", p->sync_bits, bps);
            return RCF_EINVAL;
        }
        if (p->sync_max_errors < 0 || p->sync_max_errors > std::max(0, p->sync_bits - 1)) {
            set_error("slicer: sync_max_errors %d outside 0 .. sync_bits - 1", p->sync_max_errors);
            return RCF_EINVAL;
        }
        if (!slice_sync_both_ok(p->sync_bits, p->sync_max_errors, p->sync_both)) {
            set_error("slicer: sync_both %d is not 0 or 1, or 2 x sync_max_errors %d reaches sync_bits %d", p->sync_both, p->sync_max_errors, p->sync_bits);
            return RCF_EINVAL;
        }
        if (p->hit_capacity) hit_cap = p->hit_capacity;
        if (hit_cap < 16 || hit_cap > (1 << 26) || (hit_cap & (hit_cap - 1))) {
            set_error("slicer: hit_capacity %d is not a power of two 16 .. 2^26", p->hit_capacity);
            return RCF_EINVAL;
        }
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!p) return stage_off(h, c->slicer);
    const float *soft = nullptr;
    const void *counters = nullptr;
    if (p->source == RCF_READ_CLOCK && c->clock) { soft = c->clock->ring(); counters = c->clock->counters(); }
    if (p->source == RCF_READ_COSTAS && c->costas) { soft = c->costas->ring(); counters = c->costas->counters(); }
    if (p->source == RCF_READ_FSK4 && c->fsk4) { soft = c->fsk4->ring(); counters = c->fsk4->counters(); }
    if (!soft) { set_error("channel %d does not carry the loop (%d) the slicer is to read", chan_id, p->source); return RCF_ESTATE; }
    if (h->out_cap < 64) { set_error("ring of %zu too small for the slicer", h->out_cap); return RCF_ECAP; }
    std::unique_ptr<Chan::Slicer> k(new Chan::Slicer);
    SliceLaunch &r = k->rec;
    r.soft_ring = soft;
    r.src_n_out = static_cast<const int64_t *>(counters);
    // the stage's symbol 0: the loop's count as of everything queued (one round trip)
    int rc = stage_state(h, r.src_n_out, &r.src0, sizeof(r.src0));
    if (rc != RCF_OK) return rc;
    r.bps = bps;
    r.sync_word = p->sync_bits >= 64 ? p->sync_word : p->sync_word & ((1ull << p->sync_bits) - 1);
    r.sync_bits = p->sync_bits; r.sync_max_errors = p->sync_max_errors; r.sync_both = p->sync_both;
    for (int i = 0; i < 3; ++i) r.levels[i] = p->levels[i];
    r.soft_mask = r.word_mask = (uint32_t)(h->out_cap - 1);
    r.hit_mask = (uint32_t)hit_cap - 1;
    k->source = p->source;
    k->hit_cap = (uint32_t)hit_cap;
    k->serial = next_stage_serial();
    constexpr size_t kStateWords = 256 / sizeof(uint32_t);
    static_assert(sizeof(SliceState) <= 256, "the state's slot");
    const size_t state_at = h->out_cap, hits_at = state_at + kStateWords;          // in words (out_cap >= 64: the record's 64-bit fields are aligned)
    Fresh<uint32_t> fresh;
    RCF_HIP(fresh.alloc(hits_at + (size_t)hit_cap));
    const SliceState st0{};
    if (!hip_ok(hipMemcpy(fresh.p + state_at, &st0, sizeof(st0), hipMemcpyHostToDevice), "hipMemcpy(slicer state)")) return RCF_EHIP;
    r.word_ring = fresh.take();
    r.st = reinterpret_cast<SliceState *>(r.word_ring + state_at);
    r.hit_ring = r.word_ring + hits_at;
    drop_stage(h, c->slicer);
    c->slicer = std::move(k);
    ++h->chans_epoch;
    return RCF_OK;
}

int rcf_chan_slicer_state(rcf_t *h, int chan_id, rcf_slicer_state_t *out)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->slicer) { set_error("channel %d has no slicer (rcf_chan_slicer)", chan_id); return RCF_ESTATE; }
    SliceState st{};                    // (its three counters)
    const int rc = stage_state(h, c->slicer->rec.st, &st, offsetof(SliceState, partial));
    if (rc != RCF_OK) return rc;
    out->n_symbols = st.n_symbols; out->n_words = st.n_words; out->n_hits = st.n_hits;
    return RCF_OK;
}

// ---- the frame decoders behind the slicer (tsbk.hip, edacs.hip, osw.hip, p25lc.hip)
// the NID option of the two P25 stages: RCF_NID_RAW or RCF_NID_BCH, as the launch record's flag
static bool nid_ok(const void *p, uint32_t nid, const char *name)
{
    if (p && nid != RCF_NID_RAW && nid != RCF_NID_BCH) { set_error("%s stage: nid %u is neither RCF_NID_RAW nor RCF_NID_BCH", name, nid); return false; }
    return true;
}

int rcf_chan_tsbk(rcf_t *h, int chan_id, const rcf_tsbk_params_t *p) { return rcf_chan_tsbk_ex(h, chan_id, p, RCF_NID_RAW); }

int rcf_chan_tsbk_ex(rcf_t *h, int chan_id, const rcf_tsbk_params_t *p, uint32_t nid) { return rcf_chan_tsbk_opt(h, chan_id, p, nid, RCF_TRELLIS_GREEDY); }

int rcf_chan_tsbk_opt(rcf_t *h, int chan_id, const rcf_tsbk_params_t *p, uint32_t nid, uint32_t trellis)
{
    if (!nid_ok(p, nid, "TSBK")) return RCF_EINVAL;
    if (p && trellis != RCF_TRELLIS_GREEDY && trellis != RCF_TRELLIS_VITERBI) {
        set_error("TSBK stage: trellis %u is neither RCF_TRELLIS_GREEDY nor RCF_TRELLIS_VITERBI", trellis);
        return RCF_EINVAL;
    }
    return attach_frames<Chan::Slicer::Tsbk>(h, chan_id, p,
        [](const Chan::Slicer &l) { return l.rec.bps == 2 && l.rec.sync_bits == 48 && !l.rec.sync_both && !l.p25lc; },
        "channel %d has no slicer in RCF_SLICE_FSK4 mode that searches a 48-bit sync word in one polarity, or that slicer carries the P25 voice stage",
        [nid, trellis](TsbkLaunch &r, TsbkState &st0, const SliceLaunch &, const SliceState &) {
            r.flags = (nid == RCF_NID_BCH ? kNidFlagBch : 0u) | (trellis == RCF_TRELLIS_VITERBI ? kTsbkFlagViterbi : 0u);
            st0.k_last = kTsbkNoFrame;
        });
}

// the trellis decoder's counters: the end of the TSBK stage's state record
int rcf_chan_trellis_state(rcf_t *h, int chan_id, rcf_trellis_state_t *out)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->slicer || !c->slicer->tsbk) { set_error(read_row(Chan::Slicer::Tsbk::kKind).refusal, chan_id); return RCF_ESTATE; }
    int64_t four[4];
    const int rc = stage_state(h, &c->slicer->tsbk->rec.st->vit_decoded, four, sizeof(four));
    if (rc != RCF_OK) return rc;
    out->n_decoded = four[0]; out->n_clean = four[1]; out->n_bits = four[2]; out->n_words = four[3];
    return RCF_OK;
}

// the NID decoder's counters: the end of the state record of whichever of the two stages the slicer carries
int rcf_chan_nid_state(rcf_t *h, int chan_id, rcf_nid_state_t *out)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    static_assert(offsetof(TsbkState, nid_decoded) == offsetof(P25lcState, nid_decoded), "one place for both stages");
    const char *st = c->slicer && c->slicer->tsbk ? reinterpret_cast<const char *>(c->slicer->tsbk->rec.st) :
                     c->slicer && c->slicer->p25lc ? reinterpret_cast<const char *>(c->slicer->p25lc->rec.st) : nullptr;
    if (!st) { set_error("channel %d has neither the TSBK stage nor the P25 voice stage", chan_id); return RCF_ESTATE; }
    int64_t four[4];
    const int rc = stage_state(h, st + offsetof(TsbkState, nid_decoded), four, sizeof(four));
    if (rc != RCF_OK) return rc;
    out->n_decoded = four[0]; out->n_fixed = four[1]; out->n_bits = four[2]; out->n_bad = four[3];
    return RCF_OK;
}

int rcf_chan_tsbk_state(rcf_t *h, int chan_id, rcf_tsbk_state_t *out)
{
    TsbkState st{};                     // (its five counters)
    const int rc = frames_state<Chan::Slicer::Tsbk>(h, chan_id, out, &st);
    if (rc != RCF_OK) return rc;
    out->n_records = st.n_records; out->n_frames = st.n_frames; out->n_blocks = st.n_blocks; out->n_crc_bad = st.n_crc_bad; out->n_lost = st.n_lost;
    return RCF_OK;
}

int rcf_chan_edacs(rcf_t *h, int chan_id, const rcf_edacs_params_t *p)
{
    return attach_frames<Chan::Slicer::Edacs>(h, chan_id, p,
        [](const Chan::Slicer &l) { return l.rec.bps == 1 && l.rec.sync_bits == kEdacsSyncBits; },
        "channel %d has no slicer in RCF_SLICE_BINARY mode that searches a 48-bit sync word",
        [p](EdacsLaunch &r, EdacsState &st0, const SliceLaunch &sl, const SliceState &) {
            r.flags = (sl.sync_both ? kEdacsFlagBoth : 0u) | (p->esk ? kEdacsFlagEsk : 0u);
            st0.k_last = kEdacsNoFrame;
        });
}

int rcf_chan_edacs_state(rcf_t *h, int chan_id, rcf_edacs_state_t *out)
{
    EdacsState st{};                    // (its five counters)
    const int rc = frames_state<Chan::Slicer::Edacs>(h, chan_id, out, &st);
    if (rc != RCF_OK) return rc;
    out->n_records = st.n_records; out->n_frames = st.n_frames; out->n_msgs = st.n_msgs; out->n_msgs_none = st.n_msgs_none; out->n_lost = st.n_lost;
    return RCF_OK;
}

int rcf_chan_osw(rcf_t *h, int chan_id, const rcf_osw_params_t *p)
{
    return attach_frames<Chan::Slicer::Osw>(h, chan_id, p,
        [](const Chan::Slicer &l) { return l.rec.bps == 1 && l.rec.sync_bits == kOswSyncBits && l.rec.sync_max_errors == 0 && !l.rec.sync_both; },
        "channel %d has no slicer in RCF_SLICE_BINARY mode that searches an 8-bit sync word exactly, in one polarity",
        [](OswLaunch &, OswState &st0, const SliceLaunch &, const SliceState &now) { st0.pos = now.n_symbols; });     // its cursor
}

int rcf_chan_osw_state(rcf_t *h, int chan_id, rcf_osw_state_t *out)
{
    OswState st{};                      // (its five counters and the lock)
    const int rc = frames_state<Chan::Slicer::Osw>(h, chan_id, out, &st);
    if (rc != RCF_OK) return rc;
    out->n_records = st.n_records; out->n_frames = st.n_frames; out->n_bad = st.n_bad; out->n_rejects = st.n_rejects; out->n_lost = st.n_lost;
    out->locked = st.locked; out->is_locked = st.is_locked;
    return RCF_OK;
}

int rcf_chan_p25lc(rcf_t *h, int chan_id, const rcf_p25lc_params_t *p) { return rcf_chan_p25lc_opt(h, chan_id, p, 0u); }

int rcf_chan_p25lc_opt(rcf_t *h, int chan_id, const rcf_p25lc_params_t *p, uint32_t options) { return rcf_chan_p25lc_ex(h, chan_id, p, options, RCF_NID_RAW); }

int rcf_chan_p25lc_ex(rcf_t *h, int chan_id, const rcf_p25lc_params_t *p, uint32_t options, uint32_t nid)
{
    if (!nid_ok(p, nid, "P25 voice")) return RCF_EINVAL;
    if (p && p->correct != 0 && p->correct != 1) { set_error("P25 voice stage: correct %d is not 0 or 1", p->correct); return RCF_EINVAL; }
    if (p && (options & ~(RCF_P25LC_ES | RCF_P25LC_ERASURES))) { set_error("P25 voice stage: unknown option bits 0x%x", options); return RCF_EINVAL; }
    if (p && (options & RCF_P25LC_ERASURES) && !p->correct) { set_error("P25 voice stage: RCF_P25LC_ERASURES needs correct = 1"); return RCF_EINVAL; }
    return attach_frames<Chan::Slicer::P25lc>(h, chan_id, p,
        [](const Chan::Slicer &l) { return l.rec.bps == 2 && l.rec.sync_bits == 48 && !l.rec.sync_both && !l.tsbk; },
        "channel %d has no slicer in RCF_SLICE_FSK4 mode that searches a 48-bit sync word in one polarity, or that slicer carries the TSBK stage",
        [p, options, nid](P25lcLaunch &r, P25lcState &st0, const SliceLaunch &, const SliceState &) {
            r.flags = (p->correct ? kP25lcFlagCorrect : 0u) | options << 1 | (nid == RCF_NID_BCH ? kNidFlagBch : 0u);
            st0.k_last = kTsbkNoFrame;
        });
}

int rcf_chan_p25lc_state(rcf_t *h, int chan_id, rcf_p25lc_state_t *out)
{
    P25lcState st{};                    // (its five counters)
    const int rc = frames_state<Chan::Slicer::P25lc>(h, chan_id, out, &st);
    if (rc != RCF_OK) return rc;
    out->n_records = st.n_records; out->n_frames = st.n_frames; out->n_decoded = st.n_decoded; out->n_rs_bad = st.n_rs_bad; out->n_lost = st.n_lost;
    return RCF_OK;
}

// ---- carrier detect over the IQ stream (squelch.hip)
int rcf_chan_squelch(rcf_t *h, int chan_id, const rcf_squelch_params_t *p)
{
    if (!h) return RCF_EINVAL;
    if (p && (!std::isfinite(p->threshold_db) || !(p->alpha > 0.0 && p->alpha <= 1.0))) {
        set_error("carrier detect: threshold %g dB is not finite, or alpha %g outside (0, 1]", p->threshold_db, p->alpha);
        return RCF_EINVAL;
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!p) return stage_off(h, c->squelch);
    if (c->fm_only) { set_error("channel %d exposes its discriminator only: the carrier detector reads IQ", chan_id); return RCF_ESTATE; }
    std::unique_ptr<Chan::Squelch> k(new Chan::Squelch);
    SquelchLaunch &r = k->rec;
    r.iq_ring = c->d_iq;
    r.thr = squelch_threshold(p->threshold_db);
    r.alpha = p->alpha;
    SquelchState st0{};
    st0.first_open = st0.last_open = -1;
    Fresh<SquelchState> d_state;
    RCF_HIP(d_state.alloc(1));
    if (!hip_ok(hipMemcpy(d_state.p, &st0, sizeof(st0), hipMemcpyHostToDevice), "hipMemcpy(carrier detect state)")) return RCF_EHIP;
    r.st = d_state.take();
    k->from = c->pos.produced;                                   // a new GR block: level 0 from the channel's next output on
    drop_stage(h, c->squelch);
    c->squelch = std::move(k);
    ++h->chans_epoch;
    return RCF_OK;
}

int rcf_chan_squelch_state(rcf_t *h, int chan_id, rcf_squelch_state_t *out)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->squelch) { set_error("channel %d has no carrier detector (rcf_chan_squelch)", chan_id); return RCF_ESTATE; }
    SquelchState st{};
    const int rc = stage_state(h, c->squelch->rec.st, &st, sizeof(st));
    if (rc != RCF_OK) return rc;
    out->level = st.level;
    out->n_seen = st.n_seen; out->n_open = st.n_open; out->first_open = st.first_open; out->last_open = st.last_open;
    out->unmuted = st.unmuted;
    return RCF_OK;
}

// ---- carrier-operated capture over the IQ stream (capture.hip)
static_assert(read_row(kCaptureRec).item_w == kCaptureRecWords && sizeof(rcf_capture_rec_t) == 4 * kCaptureRecWords && sizeof(CaptureRec) == sizeof(rcf_capture_rec_t) &&
              offsetof(rcf_capture_rec_t, sample) == 8 && offsetof(rcf_capture_rec_t, pos) == 16 && offsetof(rcf_capture_rec_t, peak) == 24,
              "the stream table's words per record and the ABI's record are the kernel's");
static_assert(RCF_CAPTURE_OPEN == kCaptureOpen && RCF_CAPTURE_CLOSE == kCaptureClose, "the record kinds");

// the most outputs one block of the handle can give c (rcf.h at rcf_chan_capture: M_0 = block capacity, M_i = M_(i-1) / D_i + 1
// down the channel's chain of decimations, the filterbank's first for a channel on a bin)
static int64_t max_block_outputs(rcf_t *h, const Chan *c)
{
    int64_t m = (int64_t)h->block_cap;
    if (c->src >= RCF_SRC_PFB_BIN0) m = m / std::max(1, h->pfb.D) + 1;
    else if (c->src >= 0) {
        auto it = h->chans.find(c->src);
        if (it != h->chans.end()) m = max_block_outputs(h, it->second.get());
    }
    return m / std::max(1, c->D) + 1;
}

int rcf_chan_capture(rcf_t *h, int chan_id, const rcf_capture_params_t *p)
{
    if (!h) return RCF_EINVAL;
    size_t cap = 0, rec_cap = 256;
    if (p) {
        if (!std::isfinite(p->threshold_db) || !(p->alpha > 0.0 && p->alpha <= 1.0)) {
            set_error("capture: threshold %g dB is not finite, or alpha %g outside (0, 1]", p->threshold_db, p->alpha);
            return RCF_EINVAL;
        }
        if (p->pre < 0 || p->hang < 0 || p->hang > (int64_t(1) << 60)) {
            set_error("capture: pre %lld or hang %lld is negative (or hang beyond 2^60)", (long long)p->pre, (long long)p->hang);
            return RCF_EINVAL;
        }
        if (p->capacity > (1u << 26) || p->rec_capacity > (1u << 20)) {
            set_error("capture: capacity %u beyond 2^26 samples, or rec_capacity %u beyond 2^20 records", p->capacity, p->rec_capacity);
            return RCF_EINVAL;
        }
        cap = p->capacity;
        if (p->rec_capacity) rec_cap = p->rec_capacity;
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!p) return stage_off(h, c->capture);
    if (c->fm_only) { set_error("channel %d exposes its discriminator only: the capture stage reads IQ", chan_id); return RCF_ESTATE; }
    const int64_t most = max_block_outputs(h, c);
    if (p->pre + most > (int64_t)h->out_cap) {
        set_error("capture: pre %lld + the %lld outputs a block can give channel %d > ring capacity %zu", (long long)p->pre, (long long)most, chan_id, h->out_cap);
        return RCF_ECAP;
    }
    cap = pow2_at_least(std::max<size_t>(cap ? cap : h->out_cap, 64));
    rec_cap = pow2_at_least(std::max<size_t>(rec_cap, 16));
    std::unique_ptr<Chan::Capture> k(new Chan::Capture);
    CaptureLaunch &r = k->rec;
    r.iq_ring = c->d_iq;
    r.thr = squelch_threshold(p->threshold_db);
    r.alpha = p->alpha;
    r.pre = (int32_t)p->pre;
    r.hang = p->hang;
    r.cap_mask = (uint32_t)cap - 1;
    r.rec_mask = (uint32_t)rec_cap - 1;
    k->cap = (uint32_t)cap;
    k->rec_cap = (uint32_t)rec_cap;
    CaptureState st0{};
    st0.last_open = -1;
    // one allocation, in words: captured ring | record ring | the state record's slot (cap >= 64: its 64-bit fields are aligned)
    constexpr size_t kStateWords = 256 / sizeof(uint32_t);
    static_assert(sizeof(CaptureState) <= 256, "the state's slot");
    const size_t recs_at = cap * 2, state_at = recs_at + rec_cap * kCaptureRecWords;
    Fresh<uint32_t> fresh;
    RCF_HIP(fresh.alloc(state_at + kStateWords));
    if (!hip_ok(hipMemcpy(fresh.p + state_at, &st0, sizeof(st0), hipMemcpyHostToDevice), "hipMemcpy(capture state)")) return RCF_EHIP;
    uint32_t *base = fresh.take();
    r.cap_ring = reinterpret_cast<float2 *>(base);
    r.rec_ring = base + recs_at;
    r.st = reinterpret_cast<CaptureState *>(base + state_at);
    r.a = k->from = c->pos.produced;                             // the attach point: level 0 from the channel's next output on
    drop_stage(h, c->capture);
    c->capture = std::move(k);
    ++h->chans_epoch;
    return RCF_OK;
}

int rcf_chan_capture_state(rcf_t *h, int chan_id, rcf_capture_state_t *out)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (!c->capture) { set_error(read_row(kCapture).refusal, chan_id); return RCF_ESTATE; }
    CaptureState st{};
    const int rc = stage_state(h, c->capture->rec.st, &st, sizeof(st));
    if (rc != RCF_OK) return rc;
    out->level = st.level;
    out->n_seen = st.n_seen; out->n_decided = st.n_decided; out->n_kept = st.n_kept; out->n_records = st.n_records;
    out->n_windows = st.n_windows; out->last_open = st.last_open;
    out->in_window = st.in_window; out->unmuted = st.unmuted;
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
    AudioLaunch &r = au->rec;
    r.n_lpf = p->n_lpf; r.n_hpf = p->n_hpf; r.nt_rs = n_rs_pad / I;
    r.interp = I; r.decim = p->decimation;
    r.gain = p->quad_gain;
    r.thr = std::pow(10.0, p->squelch_db / 10);                  // pwr_squelch_cc::set_threshold
    r.alpha = p->squelch_alpha;
    // iir_filter(fftaps, fbtaps, oldstyle = false): feedback taps are negated, a[0] must be 1
    r.b0 = p->deemph_b[0]; r.b1 = p->deemph_b[1]; r.fb1 = -p->deemph_a[1];
    std::vector<float> taps((size_t)p->n_lpf + p->n_hpf + n_rs_pad, 0.0f);
    std::memcpy(taps.data(), p->lpf_taps, sizeof(float) * (size_t)p->n_lpf);
    std::memcpy(taps.data() + p->n_lpf, p->hpf_taps, sizeof(float) * (size_t)p->n_hpf);
    std::memcpy(taps.data() + p->n_lpf + p->n_hpf, p->rs_taps, sizeof(float) * (size_t)p->n_rs);
    Fresh<float> d_taps, d_rings;
    Fresh<AudioState> d_state;
    RCF_HIP(d_taps.alloc(taps.size()));
    RCF_HIP(hipMemcpy(d_taps.p, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice));
    RCF_HIP(d_rings.alloc(6 * h->out_cap));
    RCF_HIP(hipMemsetAsync(d_rings.p, 0, sizeof(float) * 6 * h->out_cap, h->stream));
    AudioState st0{};
    st0.muted = 1;                                               // squelch_base_cc starts in ST_MUTED
    RCF_HIP(d_state.alloc(1));
    RCF_HIP(hipMemcpy(d_state.p, &st0, sizeof(st0), hipMemcpyHostToDevice));
    r.iq_ring = c->d_iq;
    r.st = d_state.take();
    r.a_ring = d_rings.take();                                   // a | l | h | o | c (cf32), out_cap samples each
    r.l_ring = r.a_ring + h->out_cap; r.h_ring = r.a_ring + 2 * h->out_cap; r.o_ring = r.a_ring + 3 * h->out_cap;
    r.c_ring = reinterpret_cast<float2 *>(r.a_ring + 4 * h->out_cap);
    r.lpf = d_taps.take();                                       // lpf | hpf | rs (padded)
    r.hpf = r.lpf + r.n_lpf; r.rs = r.hpf + r.n_hpf;
    au->from = c->pos.produced;                                  // a new flowgraph: zero state from here on
    drop_stage(h, c->audio);
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
    drop_stage(h, c->audio);
    ++h->chans_epoch;
    return RCF_OK;
}

// what a stage has produced so far: the end of its stream, and beside it word `word` of its counters (stream_count): the
// clock's slips stand behind its symbol count; the samples that passed the voice chain's squelch ARE its counter
static int stage_produced(rcf_t *h, int chan_id, int kind, int64_t *n, int64_t *beside, int word)
{
    if (!h || !n) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    Stream s;
    int64_t two[2];
    int rc = chan_stream(h, c, kind, &s);
    if (rc != RCF_OK || (rc = stream_count(h, s, n, two)) != RCF_OK) return rc;
    if (beside) *beside = two[word];
    return RCF_OK;
}

int rcf_chan_clock_produced(rcf_t *h, int chan_id, int64_t *n_symbols, int64_t *n_slips) { return stage_produced(h, chan_id, kClock, n_symbols, n_slips, 1); }
int rcf_chan_audio_produced(rcf_t *h, int chan_id, int64_t *n_audio, int64_t *n_ungated) { return stage_produced(h, chan_id, kAudio, n_audio, n_ungated, 0); }

}  // extern "C"
