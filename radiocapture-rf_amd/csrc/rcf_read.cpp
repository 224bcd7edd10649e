// rcf_read.cpp -- the stream table of a channel (chan_stream: ten streams, one row each; counted_stream: the six whose end
// is a device counter, without the round trip) and the one read path of every host read (host_read: one gather launch, one
// synchronisation), with the read and ring entry points of the C ABI.
#include <atomic>

#include "rcf_plan.h"

namespace rcfx {

// ring, words per item, reader, and what a missing ring means
struct StreamRow { const void *ring; uint32_t item_w; int64_t *cursor; const char *refusal; };
static int stream_row(Chan *c, int kind, StreamRow *r)
{
    Chan::Agc *ag = c->agc.get();
    Chan::Sym *sy = c->sym.get();
    Chan::Clock *ck = c->clock.get();
    Chan::Audio *au = c->audio.get();
    Chan::Costas *gc = c->costas.get();
    Chan::Fsk4 *fk = c->fsk4.get();
    Chan::Slicer *sl = c->slicer.get();
    const StreamRow t[10] = {
        {c->fm_only ? nullptr : c->d_iq, 2, &c->rd_iq, "channel %d exposes its discriminator only (rcf_chan_set_fm_only)"},
        {c->d_fm, 1, &c->rd_fm, "channel %d has no discriminator ring"},
        {ag ? ag->rec.agc_ring : nullptr, 2, ag ? &ag->rd : nullptr, "channel %d has no AGC"},
        {sy ? sy->rec.sym_ring : nullptr, 1, sy ? &sy->rd : nullptr, "channel %d has no fm filter"},
        {ck ? ck->ring() : nullptr, 1, ck ? &ck->rd : nullptr, "channel %d has no symbol clock"},
        {au ? au->rec.o_ring : nullptr, 1, au ? &au->rd : nullptr, "channel %d has no audio chain"},
        {gc ? gc->ring() : nullptr, 1, gc ? &gc->rd : nullptr, "channel %d has no Gardner / Costas stage"},
        {fk ? fk->ring() : nullptr, 1, fk ? &fk->rd : nullptr, "channel %d has no C4FM symbol loop (rcf_chan_fsk4)"},
        {sl ? sl->rec.word_ring : nullptr, 1, sl ? &sl->rd_words : nullptr, "channel %d has no slicer (rcf_chan_slicer)"},
        {sl ? sl->rec.hit_ring : nullptr, 1, sl ? &sl->rd_hits : nullptr, "channel %d has no slicer (rcf_chan_slicer)"},
    };
    if (!t[kind].ring) { set_error(t[kind].refusal, c->id); return RCF_ESTATE; }
    *r = t[kind];
    return RCF_OK;
}

int stage_state(rcf_t *h, const void *d_state, void *st, size_t bytes)
{
    RCF_HIP(hipMemcpyAsync(st, d_state, bytes, hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipStreamSynchronize(h->stream));
    return RCF_OK;
}

int counted_stream(Chan *c, int kind, CountedStream *s)
{
    StreamRow r;
    const int rc = stream_row(c, kind, &r);
    if (rc != RCF_OK) return rc;
    *s = CountedStream{r.ring, nullptr, 1u, 1u, r.cursor, 0};
    switch (kind) {
        case kReadClock:  s->counter = static_cast<const int64_t *>(c->clock->counters()); s->serial = c->clock->serial; break;
        case kReadCostas: s->counter = static_cast<const int64_t *>(c->costas->counters()); s->serial = c->costas->serial; break;
        case kReadFsk4:   s->counter = static_cast<const int64_t *>(c->fsk4->counters()); s->serial = c->fsk4->serial; break;
        case kHardBits:   s->counter = &c->slicer->rec.st->n_words; break;
        case kHardSync:   s->counter = &c->slicer->rec.st->n_hits; s->cap = c->slicer->hit_cap; break;
        default:                                         // kReadAudio: ceil(n_a * interp / decim), as chan_stream has it
            s->counter = &c->audio->rec.st->n_a;
            s->interp = (uint32_t)c->audio->rec.interp; s->decim = (uint32_t)c->audio->rec.decim;
            s->serial = c->audio->serial;
    }
    return RCF_OK;
}

int chan_stream(rcf_t *h, Chan *c, int kind, RingStream *s, int64_t *aux)
{
    StreamRow r;
    int rc = stream_row(c, kind, &r);
    if (rc != RCF_OK) return rc;
    int64_t end = c->pos.produced, beside = 0;
    if (kind_counted(kind)) {
        // the counter and the word behind it: the loops' {n_out, slips}, the voice chain's {n_a, n_prev}
        static_assert(offsetof(AudioState, n_prev) == offsetof(AudioState, n_a) + sizeof(int64_t), "n_a, then n_prev");
        CountedStream cs;
        int64_t two[2] = {0, 0};
        if ((rc = counted_stream(c, kind, &cs)) != RCF_OK || (rc = stage_state(h, cs.counter, two, sizeof(two))) != RCF_OK) return rc;
        end = (two[0] * cs.interp + cs.decim - 1) / cs.decim;
        beside = kind == kReadAudio ? two[0] : two[1];
    }
    if (aux) *aux = beside;
    *s = RingStream{h, r.ring, r.item_w, 0u, end, end, r.cursor};
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
// front-ends are 25 ms per pass.)  Counted entries ride in a launch of their own kind behind the same synchronisation: the
// host does not know their lengths, so each reserves the most it may take -- min(max, out_cap) -- and the launch's result
// words {items, cursor after} say what came.
// Staging: GatherRec[] | CountedRec[] | result words | the plain entries' rows | the counted entries' rows
int host_read(PinnedStage &stage, hipStream_t stream, rcf_t *const *idle, size_t n_idle, ReadEntry *es, size_t n)
{
    static std::atomic<uint64_t> calls{0};
    const uint64_t stamp = ++calls;
    uint64_t total = 0, total_w = 0, counted_w = 0;
    uint32_t max_w = 0, n_recs = 0, max_c = 0, n_crecs = 0;
    for (size_t i = 0; i < n; ++i) {
        ReadEntry &e = es[i];
        if (e.c) {
            if (e.c->many_stamp == stamp) { *e.count = RCF_EINVAL; e.s.ring = nullptr; continue; }   // listed twice
            e.c->many_stamp = stamp;
        }
        if (!e.s.ring) continue;
        if (e.counter) {
            *e.count = 0;
            if (!e.cap) e.cap = (uint32_t)e.s.h->out_cap;
            e.max = std::min<int64_t>(e.max, (int64_t)e.cap);
            if (e.max <= 0) { e.s.ring = nullptr; continue; }
            counted_w += (uint64_t)e.max;
            max_c = std::max<uint32_t>(max_c, (uint32_t)e.max);
            ++n_crecs;
            continue;
        }
        *e.count = lag_clamp(e.s.h, e.s.cursor, e.s.newest, e.s.end, e.max);
        if (*e.count == 0) continue;
        total += (uint64_t)*e.count;
        total_w += (uint64_t)*e.count * e.s.item_w;
        max_w = std::max<uint32_t>(max_w, (uint32_t)*e.count * e.s.item_w);
        ++n_recs;
    }
    if (total == 0 && n_crecs == 0) return RCF_OK;
    if (total_w + counted_w > 0xffffffffull) { set_error("batched read of %llu items exceeds the 32-bit word range", (unsigned long long)(total + counted_w)); return RCF_ECAP; }
    const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t rec_bytes = pad((size_t)n_recs * sizeof(GatherRec)), crec_at = rec_bytes;
    const size_t res_at = crec_at + pad((size_t)n_crecs * sizeof(CountedRec)), data_at = res_at + pad((size_t)n_crecs * 2 * sizeof(int64_t));
    const int rc = stage.ensure(data_at + (size_t)(total_w + counted_w) * 4, stream);
    if (rc != RCF_OK) return rc;
    GatherRec *recs = reinterpret_cast<GatherRec *>(stage.h);
    CountedRec *crecs = reinterpret_cast<CountedRec *>(stage.h + crec_at);
    const int64_t *res = reinterpret_cast<const int64_t *>(stage.h + res_at);
    uint32_t at_w = 0, k = 0;
    for (size_t i = 0; i < n; ++i) {
        const ReadEntry &e = es[i];
        if (!e.s.ring || e.counter || *e.count == 0) continue;
        recs[k++] = gather_rec(e.s, *e.count, at_w, 0u, ~0u, e.gain);
        at_w += (uint32_t)*e.count * e.s.item_w;
    }
    k = 0;
    for (size_t i = 0; i < n; ++i) {
        const ReadEntry &e = es[i];
        if (!e.s.ring || !e.counter) continue;
        crecs[k] = CountedRec{static_cast<const uint32_t *>(e.s.ring), e.counter, nullptr, nullptr,
                              reinterpret_cast<int64_t *>(stage.d + res_at) + 2 * k, *e.s.cursor, 0, e.interp, e.decim,
                              e.cap, (uint32_t)e.max, at_w, ~0u, 3u, 0u};
        ++k;
        at_w += (uint32_t)e.max;
    }
    uint32_t *d_dst = reinterpret_cast<uint32_t *>(stage.d + data_at);
    launch_gather_rings(reinterpret_cast<const GatherRec *>(stage.d), (int)n_recs, d_dst, max_w, stream);
    if (n_crecs) launch_gather_counted(reinterpret_cast<const CountedRec *>(stage.d + crec_at), (int)n_crecs, d_dst, max_c, stream);
    if (hipStreamSynchronize(stream) != hipSuccess) { set_error("stream sync failed"); return RCF_EHIP; }
    for (size_t j = 0; j < n_idle; ++j) free_graveyard_idle(idle[j]);   // retuned / closed channels' old buffers
    const unsigned char *src = stage.h + data_at;
    for (size_t i = 0; i < n; ++i) {
        const ReadEntry &e = es[i];
        if (!e.s.ring || e.counter || *e.count == 0) continue;
        const size_t bytes = (size_t)*e.count * e.s.item_w * 4;
        std::memcpy(e.out, src, bytes);
        src += bytes;
        *e.s.cursor += *e.count;
    }
    k = 0;
    for (size_t i = 0; i < n; ++i) {
        const ReadEntry &e = es[i];
        if (!e.s.ring || !e.counter) continue;
        *e.count = res[2 * k];                            // (pos0 = 0: the items copied)
        *e.s.cursor = res[2 * k + 1];
        ++k;
        std::memcpy(e.out, src, (size_t)*e.count * 4);
        src += (size_t)e.max * 4;
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
    const int kind = stream_kind(what);
    const size_t row = cap_each * stream_item_bytes(kind);
    std::vector<ReadEntry> es((size_t)n);
    for (int i = 0; i < n; ++i) {
        ReadEntry &e = es[(size_t)i];
        e.count = &counts[i];
        const int m = ms ? ms[i] : 0;
        if (m < 0 || (size_t)m >= n_hs) { counts[i] = RCF_EINVAL; continue; }
        auto f = hs[m]->chans.find(chan_ids[i]);
        if (f == hs[m]->chans.end()) { counts[i] = RCF_ENOCHAN; continue; }
        e.c = f->second.get();
        if (kind_counted(kind)) {                              // the device finds the stream's end: no round trip here
            CountedStream cs;
            if ((counts[i] = counted_stream(e.c, kind, &cs)) == RCF_OK) {
                e.s = RingStream{hs[m], cs.ring, 1u, 0u, 0, 0, cs.cursor};
                e.counter = cs.counter; e.interp = cs.interp; e.decim = cs.decim; e.cap = cs.cap;
            }
        } else {
            counts[i] = chan_stream(hs[m], e.c, kind, &e.s);   // RCF_ESTATE: no such stream on this channel
        }
        e.gain = kind == RCF_READ_FM ? gain : 1.0f;
        e.out = static_cast<unsigned char *>(out) + (size_t)i * row;
        e.max = (int64_t)cap_each;
    }
    return host_read(stage, stream, hs, n_hs, es.data(), es.size());
}

}  // namespace rcfx

using namespace rcfx;

extern "C" {

// a single reader of a channel stream
static int64_t chan_read_one(rcf_t *h, int chan_id, int kind, float gain, void *out, size_t max_items)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    if (kind_hard(kind)) {            // the slicer's streams: a counted entry (the device finds the end; the hit ring's own capacity)
        CountedStream cs;
        int64_t n = 0;
        int rc = counted_stream(c, kind, &cs);
        if (rc != RCF_OK) return rc;
        ReadEntry e{RingStream{h, cs.ring, 1u, 0u, 0, 0, cs.cursor}, nullptr, 1.0f, out, (int64_t)max_items, &n, cs.counter, cs.interp, cs.decim, cs.cap};
        rc = host_read(h->host_stage, h->stream, &h, 1, &e, 1);
        return rc != RCF_OK ? rc : n;
    }
    RingStream s;
    const int rc = chan_stream(h, c, kind, &s);
    return rc != RCF_OK ? rc : read_one(h, s, gain, out, max_items);
}

int64_t rcf_chan_read_iq(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_IQ, 1.0f, out, n); }
int64_t rcf_chan_read_fm(rcf_t *h, int chan_id, float gain, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_FM, gain, out, n); }
int64_t rcf_chan_read_sym(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadSym, 1.0f, out, n); }
int64_t rcf_chan_read_agc(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_AGC, 1.0f, out, n); }
int64_t rcf_chan_read_clock(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadClock, 1.0f, out, n); }
int64_t rcf_chan_read_costas(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadCostas, 1.0f, out, n); }
int64_t rcf_chan_read_fsk4(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadFsk4, 1.0f, out, n); }
int64_t rcf_chan_read_audio(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadAudio, 1.0f, out, n); }
int64_t rcf_chan_read_hard(rcf_t *h, int chan_id, uint32_t *out, size_t n) { return chan_read_one(h, chan_id, kHardBits, 1.0f, out, n); }
int64_t rcf_chan_read_sync(rcf_t *h, int chan_id, uint32_t *out, size_t n) { return chan_read_one(h, chan_id, kHardSync, 1.0f, out, n); }

int rcf_chan_read_many(rcf_t *h, int what, const int *chan_ids, int n_chans, float gain, void *out, size_t cap_each,
                       int64_t *counts)
{
    if (!h || !chan_ids || !out || !counts || n_chans < 0 || stream_kind(what) < 0) {
        set_error("bad batched read arguments");
        return RCF_EINVAL;
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    return read_many(h->host_stage, h->stream, &h, 1, nullptr, chan_ids, n_chans, what, gain, out, cap_each, counts);
}

// a zero-copy reader's view of a channel: the device ring of stream `kind` if the channel has it (`always`: or else
// RCF_ESTATE even when nobody asked for the pointer), the discriminator ring, the rings' capacity
static int chan_rings(rcf_t *h, int chan_id, int kind, bool always, void **ring, void **fm_ring, size_t *capacity)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;                  // (zero-copy readers order themselves on rcf_stream: nothing stays deferred)
    FIND_CHAN(h, chan_id, c);
    if (ring || always) {
        StreamRow r;
        const int rc = stream_row(c, kind, &r);
        if (rc != RCF_OK) return rc;
        if (ring) *ring = const_cast<void *>(r.ring);
    }
    if (fm_ring) *fm_ring = c->d_fm;
    if (capacity) *capacity = h->out_cap;
    return RCF_OK;
}

int rcf_chan_rings(rcf_t *h, int chan_id, void **iq_ring, void **fm_ring, size_t *capacity) { return chan_rings(h, chan_id, RCF_READ_IQ, false, iq_ring, fm_ring, capacity); }
int rcf_chan_agc_ring(rcf_t *h, int chan_id, void **agc_ring, size_t *capacity) { return chan_rings(h, chan_id, RCF_READ_AGC, true, agc_ring, nullptr, capacity); }
int rcf_chan_clock_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity) { return chan_rings(h, chan_id, kReadClock, true, sym_ring, nullptr, capacity); }
int rcf_chan_costas_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity) { return chan_rings(h, chan_id, kReadCostas, true, sym_ring, nullptr, capacity); }
int rcf_chan_fsk4_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity) { return chan_rings(h, chan_id, kReadFsk4, true, sym_ring, nullptr, capacity); }
int rcf_chan_slicer_rings(rcf_t *h, int chan_id, void **word_ring, size_t *word_capacity, void **hit_ring, size_t *hit_capacity)
{
    const int rc = chan_rings(h, chan_id, kHardBits, true, word_ring, nullptr, word_capacity);
    if (rc != RCF_OK) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    FIND_CHAN(h, chan_id, c);
    if (!c->slicer) { set_error("channel %d has no slicer (rcf_chan_slicer)", chan_id); return RCF_ESTATE; }   // (closed in between)
    if (hit_ring) *hit_ring = c->slicer->rec.hit_ring;
    if (hit_capacity) *hit_capacity = c->slicer->hit_cap;
    return RCF_OK;
}

}  // extern "C"
