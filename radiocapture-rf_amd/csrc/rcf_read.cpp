// rcf_read.cpp -- the stream table of a channel (chan_stream: eight streams, one row each) and the one read path of every
// host read (host_read: one gather launch, one synchronisation), with the read and ring entry points of the C ABI.
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
    const StreamRow t[8] = {
        {c->fm_only ? nullptr : c->d_iq, 2, &c->rd_iq, "channel %d exposes its discriminator only (rcf_chan_set_fm_only)"},
        {c->d_fm, 1, &c->rd_fm, "channel %d has no discriminator ring"},
        {ag ? ag->rec.agc_ring : nullptr, 2, ag ? &ag->rd : nullptr, "channel %d has no AGC"},
        {sy ? sy->rec.sym_ring : nullptr, 1, sy ? &sy->rd : nullptr, "channel %d has no fm filter"},
        {ck ? ck->ring() : nullptr, 1, ck ? &ck->rd : nullptr, "channel %d has no symbol clock"},
        {au ? au->rec.o_ring : nullptr, 1, au ? &au->rd : nullptr, "channel %d has no audio chain"},
        {gc ? gc->ring() : nullptr, 1, gc ? &gc->rd : nullptr, "channel %d has no Gardner / Costas stage"},
        {fk ? fk->ring() : nullptr, 1, fk ? &fk->rd : nullptr, "channel %d has no C4FM symbol loop (rcf_chan_fsk4)"},
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

int chan_stream(rcf_t *h, Chan *c, int kind, RingStream *s, int64_t *aux)
{
    StreamRow r;
    int rc = stream_row(c, kind, &r);
    if (rc != RCF_OK) return rc;
    int64_t end = c->pos.produced, beside = 0;
    const void *loop = kind == kReadClock ? c->clock->counters() : kind == kReadCostas ? c->costas->counters()
                     : kind == kReadFsk4 ? c->fsk4->counters() : nullptr;
    if (loop) {                                      // the three loops alike
        int64_t n_out_slips[2] = {0, 0};
        if ((rc = stage_state(h, loop, n_out_slips, sizeof(n_out_slips))) != RCF_OK) return rc;
        end = n_out_slips[0];
        beside = n_out_slips[1];
    } else if (kind == kReadAudio) {
        AudioState st{};
        if ((rc = stage_state(h, c->audio->rec.st, &st, sizeof(st))) != RCF_OK) return rc;
        const int64_t I = c->audio->rec.interp, D = c->audio->rec.decim;
        end = (st.n_a * I + D - 1) / D;
        beside = st.n_a;
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

extern "C" {

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

int64_t rcf_chan_read_iq(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_IQ, 1.0f, out, n); }
int64_t rcf_chan_read_fm(rcf_t *h, int chan_id, float gain, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_FM, gain, out, n); }
int64_t rcf_chan_read_sym(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadSym, 1.0f, out, n); }
int64_t rcf_chan_read_agc(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, RCF_READ_AGC, 1.0f, out, n); }
int64_t rcf_chan_read_clock(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadClock, 1.0f, out, n); }
int64_t rcf_chan_read_costas(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadCostas, 1.0f, out, n); }
int64_t rcf_chan_read_fsk4(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadFsk4, 1.0f, out, n); }
int64_t rcf_chan_read_audio(rcf_t *h, int chan_id, float *out, size_t n) { return chan_read_one(h, chan_id, kReadAudio, 1.0f, out, n); }

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

}  // extern "C"
