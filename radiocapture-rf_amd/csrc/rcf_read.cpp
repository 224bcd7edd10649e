// rcf_read.cpp -- a channel's streams (chan_stream: the channel's side of the stream table, rcf_streams.h) and the one read
// path of every host read (host_read: one gather launch, one synchronisation), with the read and ring entry points of the
// C ABI.
#include <atomic>

#include "rcf_plan.h"

namespace rcfx {

namespace {

// a plain row ends at the channel's `produced`; a counted row at its stage's device counter
void plain_row(Chan *c, Stream *s, const void *ring, int64_t *cursor) { s->ring = ring; s->cursor = cursor; s->end = s->newest = c->pos.produced; }
void counted_row(Stream *s, const void *ring, int64_t *cursor, const int64_t *counter, uint64_t serial, int interp = 1, int decim = 1)
{
    s->ring = ring; s->cursor = cursor; s->counter = counter; s->serial = serial;
    s->interp = (uint32_t)interp; s->decim = (uint32_t)decim;
}
template <class L> void loop_row(L *l, Stream *s) { if (l) counted_row(s, l->ring(), &l->rd, static_cast<const int64_t *>(l->counters()), l->serial); }
// a frame decoder's records: a ring of the decoder's own capacity
template <class R> void frames_row(Chan *c, Stream *s)
{
    if (R *t = c->slicer ? c->slicer->frames<R>().get() : nullptr) { counted_row(s, t->rec.rec_ring, &t->rd, &t->rec.st->n_records, t->serial); s->cap = t->cap; }
}
// ring, reader and counter of every row of kStreams and of the readers' rows behind it, in their order; a row that leaves the
// ring null is refused
void (*const kRows[kReadRowsEnd])(Chan *, Stream *) = {
    [](Chan *c, Stream *s) { if (!c->fm_only) plain_row(c, s, c->d_iq, &c->rd_iq); },
    [](Chan *c, Stream *s) { plain_row(c, s, c->d_fm, &c->rd_fm); },
    [](Chan *c, Stream *s) { if (c->agc) plain_row(c, s, c->agc->rec.agc_ring, &c->agc->rd); },
    [](Chan *c, Stream *s) { if (c->sym) plain_row(c, s, c->sym->rec.sym_ring, &c->sym->rd); },
    [](Chan *c, Stream *s) { loop_row(c->clock.get(), s); },
    [](Chan *c, Stream *s) { if (Chan::Audio *a = c->audio.get()) counted_row(s, a->rec.o_ring, &a->rd, &a->rec.st->n_a, a->serial, a->rec.interp, a->rec.decim); },
    [](Chan *c, Stream *s) { loop_row(c->costas.get(), s); },
    [](Chan *c, Stream *s) { loop_row(c->fsk4.get(), s); },
    [](Chan *c, Stream *s) { if (Chan::Slicer *l = c->slicer.get()) counted_row(s, l->rec.word_ring, &l->rd_words, &l->rec.st->n_words, l->serial); },
    [](Chan *c, Stream *s) { if (Chan::Slicer *l = c->slicer.get()) { counted_row(s, l->rec.hit_ring, &l->rd_hits, &l->rec.st->n_hits, l->serial); s->cap = l->hit_cap; } },
    frames_row<Chan::Slicer::Tsbk>,
    frames_row<Chan::Slicer::Edacs>,
    frames_row<Chan::Slicer::Osw>,
    frames_row<Chan::Slicer::P25lc>,
    [](Chan *c, Stream *s) { if (Chan::Capture *k = c->capture.get()) { counted_row(s, k->rec.cap_ring, &k->rd, &k->rec.st->n_kept, k->serial); s->cap = k->cap; } },
    [](Chan *c, Stream *s) { if (Chan::Capture *k = c->capture.get()) { counted_row(s, k->rec.rec_ring, &k->rd_rec, &k->rec.st->n_records, k->serial); s->cap = k->rec_cap; } },
};

}  // namespace

int chan_stream(rcf_t *h, Chan *c, int kind, Stream *s)
{
    *s = Stream{h, nullptr, read_row(kind).item_w, 0u, (uint32_t)h->out_cap};
    kRows[kind](c, s);
    if (!s->ring) { set_error(read_row(kind).refusal, c->id); return RCF_ESTATE; }
    return RCF_OK;
}

int stage_state(rcf_t *h, const void *d_state, void *st, size_t bytes)
{
    RCF_HIP(hipMemcpyAsync(st, d_state, bytes, hipMemcpyDeviceToHost, h->stream));
    RCF_HIP(hipStreamSynchronize(h->stream));
    return RCF_OK;
}

int stream_count(rcf_t *h, const Stream &s, int64_t *end, int64_t two[2])
{
    static_assert(offsetof(AudioState, n_prev) == offsetof(AudioState, n_a) + sizeof(int64_t), "n_a, then n_prev");
    two[0] = two[1] = 0;
    const int rc = stage_state(h, s.counter, two, 2 * sizeof(int64_t));
    if (rc == RCF_OK) *end = count_end(two[0], s.interp, s.decim);
    return rc;
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
// host does not know their lengths, so each reserves the most it may take -- min(max, cap) items -- and the launch's result
// words {items, cursor after} say what came.
// Staging: GatherRec[] | CountedRec[] | result words | the plain entries' rows | the counted entries' rows
int host_read(PinnedStage &stage, hipStream_t stream, rcf_t *const *idle, size_t n_idle, ReadEntry *es, size_t n)
{
    static std::atomic<uint64_t> calls{0};
    const uint64_t stamp = ++calls;
    std::vector<ReadEntry *> plain, counted;              // the entries with something to read, in order: here the two kinds part
    uint64_t total = 0, total_w = 0, counted_w = 0;
    uint32_t max_w = 0, max_c = 0;
    for (size_t i = 0; i < n; ++i) {
        ReadEntry &e = es[i];
        if (e.c) {
            if (e.c->many_stamp == stamp) { *e.count = RCF_EINVAL; continue; }   // listed twice
            e.c->many_stamp = stamp;
        }
        if (!e.s.ring) continue;
        if (e.s.counter) {
            *e.count = 0;
            e.max = std::min<int64_t>(e.max, (int64_t)e.s.cap);
            if (e.max <= 0) continue;
            counted_w += (uint64_t)e.max * e.s.item_w;
            max_c = std::max<uint32_t>(max_c, (uint32_t)e.max * e.s.item_w);
            counted.push_back(&e);
        } else {
            *e.count = lag_clamp((int64_t)e.s.cap, e.s.cursor, e.s.newest, e.s.end, e.max);
            if (*e.count == 0) continue;
            total += (uint64_t)*e.count;
            total_w += (uint64_t)*e.count * e.s.item_w;
            max_w = std::max<uint32_t>(max_w, (uint32_t)*e.count * e.s.item_w);
            plain.push_back(&e);
        }
    }
    if (plain.empty() && counted.empty()) return RCF_OK;
    if (total_w + counted_w > 0xffffffffull) { set_error("batched read of %llu items exceeds the 32-bit word range", (unsigned long long)(total + counted_w)); return RCF_ECAP; }
    const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t crec_at = pad(plain.size() * sizeof(GatherRec));
    const size_t res_at = crec_at + pad(counted.size() * sizeof(CountedRec)), data_at = res_at + pad(counted.size() * 2 * sizeof(int64_t));
    const int rc = stage.ensure(data_at + (size_t)(total_w + counted_w) * 4, stream);
    if (rc != RCF_OK) return rc;
    GatherRec *recs = reinterpret_cast<GatherRec *>(stage.h);
    CountedRec *crecs = reinterpret_cast<CountedRec *>(stage.h + crec_at);
    const int64_t *res = reinterpret_cast<const int64_t *>(stage.h + res_at);
    uint32_t at_w = 0;
    for (const ReadEntry *e : plain) {
        *recs++ = gather_rec(e->s, *e->count, at_w, 0u, ~0u, e->gain);
        at_w += (uint32_t)*e->count * e->s.item_w;
    }
    for (size_t k = 0; k < counted.size(); ++k) {
        const ReadEntry &e = *counted[k];                 // (the host owns the cursor and the row starts at 0: flags 3)
        crecs[k] = CountedRec{static_cast<const uint32_t *>(e.s.ring), e.s.counter, nullptr, nullptr,
                              reinterpret_cast<int64_t *>(stage.d + res_at) + 2 * k, *e.s.cursor, 0, e.s.interp, e.s.decim,
                              e.s.cap, (uint32_t)e.max, at_w, ~0u, 3u, e.s.item_w};
        at_w += (uint32_t)e.max * e.s.item_w;
    }
    uint32_t *d_dst = reinterpret_cast<uint32_t *>(stage.d + data_at);
    launch_gather_rings(reinterpret_cast<const GatherRec *>(stage.d), (int)plain.size(), d_dst, max_w, stream);
    launch_gather_counted(reinterpret_cast<const CountedRec *>(stage.d + crec_at), (int)counted.size(), d_dst, max_c, stream);
    if (hipStreamSynchronize(stream) != hipSuccess) { set_error("stream sync failed"); return RCF_EHIP; }
    for (size_t j = 0; j < n_idle; ++j) free_graveyard_idle(idle[j]);   // retuned / closed channels' old buffers
    const unsigned char *src = stage.h + data_at;
    for (const ReadEntry *e : plain) {
        const size_t bytes = (size_t)*e->count * e->s.item_w * 4;
        std::memcpy(e->out, src, bytes);
        src += bytes;
        *e->s.cursor += *e->count;
    }
    for (size_t k = 0; k < counted.size(); ++k) {
        const ReadEntry &e = *counted[k];
        *e.count = res[2 * k];                            // (pos0 = 0: the items copied)
        *e.s.cursor = res[2 * k + 1];
        std::memcpy(e.out, src, (size_t)*e.count * e.s.item_w * 4);
        src += (size_t)e.max * e.s.item_w * 4;
    }
    return RCF_OK;
}

int64_t read_one(rcf_t *h, const Stream &s, float gain, void *out, size_t max_items)
{
    int64_t n = 0;
    ReadEntry e{s, nullptr, gain, out, (int64_t)max_items, &n};
    const int rc = host_read(h->host_stage, h->stream, &h, 1, &e, 1);
    return rc != RCF_OK ? rc : n;
}

// the entry of channel chan_id of h as stream `kind`, for a single reader as for entry i of a batched one; when there is
// nothing to read -- no such channel, no such stream on it -- *count says why and the entry has no ring
static void chan_entry(rcf_t *h, int chan_id, int kind, float gain, void *out, size_t max_items, int64_t *count, ReadEntry *e)
{
    e->gain = kind == kFm ? gain : 1.0f;
    e->out = out;
    e->max = (int64_t)max_items;
    e->count = count;
    auto f = h->chans.find(chan_id);
    if (f == h->chans.end()) { set_error("no such channel %d", chan_id); *count = RCF_ENOCHAN; return; }
    e->c = f->second.get();
    if ((*count = chan_stream(h, e->c, kind, &e->s)) != RCF_OK) e->s.ring = nullptr;
}

int read_many(PinnedStage &stage, hipStream_t stream, rcf_t *const *hs, size_t n_hs, const int *ms, const int *chan_ids, int n,
              int what, float gain, void *out, size_t cap_each, int64_t *counts)
{
    const int kind = row_kind(what);
    const size_t row = cap_each * read_row(kind).item_w * 4;
    std::vector<ReadEntry> es((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int m = ms ? ms[i] : 0;
        if (m < 0 || (size_t)m >= n_hs) { es[(size_t)i].count = &counts[i]; counts[i] = RCF_EINVAL; continue; }
        chan_entry(hs[m], chan_ids[i], kind, gain, static_cast<unsigned char *>(out) + (size_t)i * row, cap_each, &counts[i], &es[(size_t)i]);
    }
    return host_read(stage, stream, hs, n_hs, es.data(), es.size());
}

}  // namespace rcfx

using namespace rcfx;

extern "C" {

// a single reader of a channel stream
static int64_t chan_read_one(rcf_t *h, int chan_id, int what, float gain, void *out, size_t max_items)
{
    if (!h || !out) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    int64_t n = 0;
    ReadEntry e;
    chan_entry(h, chan_id, row_kind(what), gain, out, max_items, &n, &e);
    return e.s.ring ? read_one(h, e.s, e.gain, out, max_items) : n;
}

int64_t rcf_chan_read_iq(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_IQ, 1.0f, out, n); }
int64_t rcf_chan_read_fm(rcf_t *h, int chan_id, float gain, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_FM, gain, out, n); }
int64_t rcf_chan_read_sym(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_SYM, 1.0f, out, n); }
int64_t rcf_chan_read_agc(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_AGC, 1.0f, out, n); }
int64_t rcf_chan_read_clock(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_CLOCK, 1.0f, out, n); }
int64_t rcf_chan_read_costas(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_COSTAS, 1.0f, out, n); }
int64_t rcf_chan_read_fsk4(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_FSK4, 1.0f, out, n); }
int64_t rcf_chan_read_audio(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_AUDIO, 1.0f, out, n); }
int64_t rcf_chan_read_hard(rcf_t *h, int chan_id, uint32_t *out, size_t n) { return chan_read_one(h, chan_id, RCF_HARD_BITS, 1.0f, out, n); }
int64_t rcf_chan_read_sync(rcf_t *h, int chan_id, uint32_t *out, size_t n) { return chan_read_one(h, chan_id, RCF_HARD_SYNC, 1.0f, out, n); }
int64_t rcf_chan_read_tsbk(rcf_t *h, int chan_id, uint32_t *out, size_t n) { return chan_read_one(h, chan_id, RCF_HARD_TSBK, 1.0f, out, n); }
int64_t rcf_chan_read_edacs(rcf_t *h, int chan_id, uint32_t *out, size_t n) { return chan_read_one(h, chan_id, RCF_HARD_EDACS, 1.0f, out, n); }
int64_t rcf_chan_read_osw(rcf_t *h, int chan_id, uint32_t *out, size_t n) { return chan_read_one(h, chan_id, RCF_HARD_OSW, 1.0f, out, n); }
int64_t rcf_chan_read_p25lc(rcf_t *h, int chan_id, uint32_t *out, size_t n) { return chan_read_one(h, chan_id, RCF_HARD_P25LC, 1.0f, out, n); }
int64_t rcf_chan_read_capture(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_CAPTURE, 1.0f, out, n); }
int64_t rcf_chan_read_capture_rec(rcf_t *h, int chan_id, uint32_t *out, size_t n) { return chan_read_one(h, chan_id, RCF_HARD_CAPTURE, 1.0f, out, n); }

int rcf_chan_read_many(rcf_t *h, int what, const int *chan_ids, int n_chans, float gain, void *out, size_t cap_each,
                       int64_t *counts)
{
    if (!h || !chan_ids || !out || !counts || n_chans < 0 || row_kind(what) < 0) {
        set_error("bad batched read arguments");
        return RCF_EINVAL;
    }
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    return read_many(h->host_stage, h->stream, &h, 1, nullptr, chan_ids, n_chans, what, gain, out, cap_each, counts);
}

// a zero-copy reader's view of c's stream `kind`: its device ring and that ring's capacity, the handle's out_cap or the
// ring's own; RCF_ESTATE when the channel does not carry it.  (The caller holds the lock.)
static int stream_ring(rcf_t *h, Chan *c, int kind, void **ring, size_t *capacity)
{
    Stream s;
    const int rc = chan_stream(h, c, kind, &s);
    if (rc != RCF_OK) return rc;
    if (ring) *ring = const_cast<void *>(s.ring);
    if (capacity) *capacity = s.cap;
    return RCF_OK;
}

// ... of a channel: the ring of stream `kind` if the channel has it (`always`: or else RCF_ESTATE even when nobody asked
// for the pointer), the discriminator ring, the rings' capacity
static int chan_rings(rcf_t *h, int chan_id, int kind, bool always, void **ring, void **fm_ring, size_t *capacity)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;                  // (zero-copy readers order themselves on rcf_stream: nothing stays deferred)
    FIND_CHAN(h, chan_id, c);
    if (ring || always) {
        const int rc = stream_ring(h, c, kind, ring, capacity);
        if (rc != RCF_OK) return rc;
    } else if (capacity) *capacity = h->out_cap;
    if (fm_ring) *fm_ring = c->d_fm;
    return RCF_OK;
}

int rcf_chan_rings(rcf_t *h, int chan_id, void **iq_ring, void **fm_ring, size_t *capacity) { return chan_rings(h, chan_id, kIq, false, iq_ring, fm_ring, capacity); }
int rcf_chan_agc_ring(rcf_t *h, int chan_id, void **agc_ring, size_t *capacity) { return chan_rings(h, chan_id, kAgc, true, agc_ring, nullptr, capacity); }
int rcf_chan_clock_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity) { return chan_rings(h, chan_id, kClock, true, sym_ring, nullptr, capacity); }
int rcf_chan_costas_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity) { return chan_rings(h, chan_id, kCostas, true, sym_ring, nullptr, capacity); }
int rcf_chan_fsk4_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity) { return chan_rings(h, chan_id, kFsk4, true, sym_ring, nullptr, capacity); }
int rcf_chan_slicer_rings(rcf_t *h, int chan_id, void **word_ring, size_t *word_capacity, void **hit_ring, size_t *hit_capacity)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    const int rc = stream_ring(h, c, kHardBits, word_ring, word_capacity);
    return rc != RCF_OK ? rc : stream_ring(h, c, kHardSync, hit_ring, hit_capacity);
}
int rcf_chan_capture_rings(rcf_t *h, int chan_id, void **cap_ring, size_t *capacity, void **rec_ring, size_t *rec_capacity)
{
    if (!h) return RCF_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (set_dev(h)) return RCF_EHIP;
    FIND_CHAN(h, chan_id, c);
    const int rc = stream_ring(h, c, kCapture, cap_ring, capacity);
    return rc != RCF_OK ? rc : stream_ring(h, c, kCaptureRec, rec_ring, rec_capacity);
}
int rcf_chan_tsbk_ring(rcf_t *h, int chan_id, void **rec_ring, size_t *capacity) { return chan_rings(h, chan_id, kTsbk, true, rec_ring, nullptr, capacity); }
int rcf_chan_edacs_ring(rcf_t *h, int chan_id, void **rec_ring, size_t *capacity) { return chan_rings(h, chan_id, kEdacs, true, rec_ring, nullptr, capacity); }
int rcf_chan_osw_ring(rcf_t *h, int chan_id, void **rec_ring, size_t *capacity) { return chan_rings(h, chan_id, kOsw, true, rec_ring, nullptr, capacity); }
int rcf_chan_p25lc_ring(rcf_t *h, int chan_id, void **rec_ring, size_t *capacity) { return chan_rings(h, chan_id, kP25lc, true, rec_ring, nullptr, capacity); }

}  // extern "C"
