// rcf_pump.cpp -- the native real-time pump: one thread per group of front-ends that takes whichever input blocks are
// complete, issues them as one group block (rcf_group.cpp), keeps two group blocks in flight and delivers every channel's
// output into its pinned host ring.  It replaces the interpreter between "the block's last sample exists" and "its outputs
// are in host memory" (the per-source work loop of rc_frontend/receiver.py:477-700 as GNU Radio's scheduler threads run it).
#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <sys/resource.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <thread>

#include "rcf_group.h"

using namespace rcfx;

// =================================================================== the pump
struct rcf_pump {
    rcf_group *g = nullptr;
    rcf_pump_config_t cfg{};
    std::vector<const unsigned char *> rings, rings_dev;     // host address / the same memory as the device sees it (or nullptr)
    std::vector<size_t> ring_blocks;
    std::vector<double> phase;
    std::vector<const volatile uint64_t *> written;
    // Subscription slots (guarded by g->mu), fixed at start (cfg.n_read of them subscribed, room for max_read):
    // rcf_pump_subscribe / rcf_pump_unsubscribe move channels in and out while the thread runs.  A counted slot's cursor in
    // the stage's stream and its item count live in d_cstate, {cursor, items} twice per slot -- a gather reads the copy
    // `par` and writes the other (CountedRec; DESIGN.md, "Counted slots") --, and its `queued` is an UPPER bound: every
    // gather adds the most it may take, and its completion puts the bound back on the true count its result words report.
    struct Slot {
        int member = -1;                           // -1: free
        int chan = -1;                             // the member's channel, or RCF_SRC_PFB_BIN0 + a bin of its fused discriminator ring
        int kind = kIq;                            // the stream delivered: a reader's kind (read_kind / read_row; kFm x gain)
        float gain = 1.0f;
        Chan *c = nullptr;                         // the channel, resolved once per channel-set epoch (null: closed, or a bin)
        int64_t bin_rd = 0;                        // a bin's slot: frames delivered
        int64_t queued = 0;                        // items ever queued for the slot's host ring
        bool par = false;                          // the copy of d_cstate the slot's next gather reads
        bool fresh = true;                         // the next gather takes cursor and item count from the host: a new subscription
        bool last_counted = false;                 // the slot's last tenant was counted (its count is the bound, not exact)
        uint64_t serial = 0;                       // the attachment of the stage the device cursor belongs to (Stream::serial)
        uint32_t gen = 0;                          // bumped by every subscription: gathers of an earlier tenant no longer count
    };
    std::vector<Slot> slots;
    std::vector<std::vector<int>> entries_of;      // member -> its slots
    std::vector<uint64_t> epoch_of;                // per member: the epoch Slot::c was resolved at (~0: resolve again)
    int64_t *d_cstate = nullptr;
    unsigned char *h_crecs = nullptr, *h_crecs_dev = nullptr;   // pinned, per in-flight block: CountedRec[recs_cap] | result words[recs_cap][2]
    size_t out_cap = 0;                            // host ring length per slot (items of up to 8 bytes, power of two)
    static constexpr size_t kSlotItemBytes = 8;    // every slot is out_cap x 8 bytes (a discriminator slot uses half; 32-byte
                                                   // records: out_cap / 4 of them -- ring_items)
    unsigned char *h_out = nullptr, *h_out_dev = nullptr;   // the slots' rings
    std::unique_ptr<std::atomic<int64_t>[]> out_written;    // items delivered per slot
    std::unique_ptr<std::atomic<int64_t>[]> out_queued;     // items whose gather has been (or is about to be) launched
    // gather records of the two group blocks in flight (pinned)
    unsigned char *h_recs = nullptr, *h_recs_dev = nullptr;
    size_t recs_cap = 0;                           // records per slot
    hipEvent_t slot_ev[2] = {nullptr, nullptr};
    std::thread th;
    std::atomic<bool> stop{false}, running{false};
    std::atomic<int> error{0}, rt_granted{0};
    std::mutex st_mu;                              // the statistics below
    std::vector<float> lat_ms;
    int64_t blocks_done = 0, judged = 0, late = 0, overruns = 0, group_blocks = 0, max_batch = 0, samples_out = 0;
    double plan_ms = 0, wait_ms = 0;
    double max_plan_ms = 0, max_wait_ms = 0, max_idle_gap_ms = 0;   // longest single planning / device wait / sleep overshoot
    int64_t slow_plans = 0, slow_waits = 0, slow_sleeps = 0;        // ... and how many of them exceeded 5 / 5 / 2 ms (after the warm-up)
    bool warm_done = false;
    // why late: run-queue delay of the thread (schedstat), see rcf_pump_stats_t
    double runq_total_ms = -1, slow_wait_total_ms = 0, runq_in_slow_waits_ms = 0, slow_sleep_total_ms = 0, runq_in_slow_sleeps_ms = 0;
    int64_t nivcsw = 0;
    std::chrono::steady_clock::time_point t_start, t_end;
    char err_text[256] = "";
    size_t item_bytes(int e) const { return read_row(slots[(size_t)e].kind).item_w * 4u; }
    size_t ring_items(int e) const { return (size_t)slot_items(slots[(size_t)e].kind, (int64_t)out_cap); }   // the slot's host ring, in ITS items
    // Slot e takes a new tenant.  Its counters go on from where the previous tenant left them: the new stream starts at
    // `queued`.  Gathers still in flight for a COUNTED previous tenant no longer count (gen): the new stream starts at the
    // bound they stay below, and the slot's item count jumps there
    void occupy(int e, int member, int chan, int kind, float gain_, int64_t bin_rd_ = 0)
    {
        Slot &t = slots[(size_t)e];
        t.member = member; t.chan = chan; t.kind = kind; t.gain = gain_; t.bin_rd = bin_rd_;
        ++t.gen;
        if (t.last_counted) out_written[(size_t)e].store(t.queued, std::memory_order_release);
        t.last_counted = read_row(kind).counted;
        t.fresh = true;
        t.c = nullptr;
        entries_of[(size_t)member].push_back(e);
        epoch_of[(size_t)member] = ~0ull;          // resolved at the member's next block
    }
    void vacate(int e)
    {
        Slot &t = slots[(size_t)e];
        auto &v = entries_of[(size_t)t.member];
        v.erase(std::remove(v.begin(), v.end(), e), v.end());
        t.member = t.chan = -1;
        t.c = nullptr;
    }
    size_t crecs_bytes() const { return recs_cap * (sizeof(CountedRec) + 2 * sizeof(int64_t)); }   // of one in-flight block
    ~rcf_pump()
    {
        // (also what an rcf_pump_start that fails half-way leaves through: pinned rings, records, events)
        for (int i = 0; i < 2; ++i) if (slot_ev[i]) (void)hipEventDestroy(slot_ev[i]);
        if (h_recs) (void)hipHostFree(h_recs);
        if (h_crecs) (void)hipHostFree(h_crecs);
        if (d_cstate) (void)hipFree(d_cstate);
        if (h_out) (void)hipHostFree(h_out);
    }
};

namespace {

using Clock = std::chrono::steady_clock;
inline double secs(Clock::duration d) { return std::chrono::duration<double>(d).count(); }

struct InFlight {
    bool busy = false;
    std::vector<int> members;          // member indices of the batch
    std::vector<double> due;           // per member: when its block was complete (seconds since t0)
    std::vector<int64_t> kidx;         // per member: which of its blocks
    std::vector<std::pair<int, int64_t>> delivered;   // (entry, items) to publish once the gather has run
    struct Counted { int entry; uint32_t gen; int64_t bound; int rec; };
    std::vector<Counted> counted;      // counted slots: the tenant the gather was for, the most it takes, its result words
};

// nanoseconds this thread has spent runnable without a CPU (second field of /proc/thread-self/schedstat); -1: unreadable
long long run_delay_ns(int fd)
{
    if (fd < 0) return -1;
    char b[96];
    const ssize_t n = pread(fd, b, sizeof b - 1, 0);
    if (n <= 0) return -1;
    b[n] = 0;
    long long run = 0, delay = 0;
    return std::sscanf(b, "%lld %lld", &run, &delay) == 2 ? delay : -1;
}

long thread_nivcsw()
{
    rusage ru{};
    return getrusage(RUSAGE_THREAD, &ru) == 0 ? ru.ru_nivcsw : 0;
}

// pinned host memory and the address the device sees it at; false, with the error text: none to be had
bool pinned_alloc(size_t bytes, unsigned char **h, unsigned char **dev, const char *what)
{
    void *hp = nullptr, *dv = nullptr;
    if (hipHostMalloc(&hp, bytes, hipHostMallocDefault) != hipSuccess || hipHostGetDevicePointer(&dv, hp, 0) != hipSuccess) {
        if (hp) (void)hipHostFree(hp);
        (void)hipGetLastError();
        set_error("pinned %s of %zu bytes failed", what, bytes);
        return false;
    }
    *h = static_cast<unsigned char *>(hp);
    *dev = static_cast<unsigned char *>(dv);
    return true;
}

void pump_fail(rcf_pump *p, int code)
{
    p->error.store(code);
    std::snprintf(p->err_text, sizeof p->err_text, "%s", rcf_last_error());
}

// ---- the read of a group block: every subscribed channel of its members, straight into the host rings.  The caller
// holds g->mu and the members' locks.
constexpr uint32_t kSlotW = (uint32_t)(rcf_pump::kSlotItemBytes / 4);   // words per item a slot is laid out for

struct Gather {
    rcf_pump *p;
    int block;                         // which of the two in flight
    InFlight &s;
    GatherRec *recs;                   // the block's records (pinned), and the counted ones as the host and the device see them
    CountedRec *crecs;
    unsigned char *crecs_dev;
    int n_recs = 0, n_crecs = 0;
    uint32_t max_w = 0, max_c = 0;
    void plain(int e, const Stream &st);
    void counted(int e, const Stream &st);
    int launch();                      // both gathers, and the event the block's completion waits for
};

// channels were opened / closed on member m: look its slots' channels up again
void resolve_member(rcf_pump *p, int m, rcf_t *h)
{
    for (int e : p->entries_of[(size_t)m]) {
        rcf_pump::Slot &t = p->slots[(size_t)e];
        if (t.chan >= RCF_SRC_PFB_BIN0) continue;
        auto f = h->chans.find(t.chan);
        t.c = f == h->chans.end() ? nullptr : f->second.get();
    }
    p->epoch_of[(size_t)m] = h->chans_epoch;
}

// what the slot delivers, or false: it starves (no such bin, a channel closed under the pump, a stream or stage it lacks)
bool slot_stream(rcf_pump::Slot &t, rcf_t *h, Stream *st)
{
    if (t.chan >= RCF_SRC_PFB_BIN0) return pfb_fm_stream(h, t.chan - RCF_SRC_PFB_BIN0, &t.bin_rd, true, st);
    return t.c && chan_stream(h, t.c, t.kind, st) == RCF_OK;
}

void Gather::plain(int e, const Stream &st)
{
    rcf_pump::Slot &t = p->slots[(size_t)e];
    const int64_t n = ring_room(st.cursor, lag_clamp((int64_t)st.cap, st.cursor, st.newest, st.end, INT64_MAX), (int64_t)p->out_cap);
    if (n == 0) return;
    const uint32_t ew = st.item_w;                         // words per item of this slot's stream
    const uint64_t dst_pos = (uint64_t)t.queued & (p->out_cap - 1);
    t.queued += n;
    // (published BEFORE the launch: a reader that copied positions this gather overwrites finds out)
    p->out_queued[(size_t)e].store(t.queued, std::memory_order_release);
    recs[n_recs++] = gather_rec(st, n, (uint32_t)((size_t)e * p->out_cap * kSlotW), (uint32_t)(dst_pos * ew),
                                (uint32_t)(p->out_cap * ew - 1), t.kind == kFm ? t.gain : 1.0f);
    max_w = std::max<uint32_t>(max_w, (uint32_t)n * ew);
    *st.cursor += n;
    s.delivered.push_back({e, n});
}

void Gather::counted(int e, const Stream &st)
{
    rcf_pump::Slot &t = p->slots[(size_t)e];
    // a new subscription starts at the channel's own reader and at the slot's item count; a stage attached again (the host
    // did it, under the member's lock) at symbol 0 of the new ring
    const bool fresh = t.fresh, again = !fresh && t.serial != st.serial;
    t.fresh = false;
    t.serial = st.serial;
    // the most this gather may take (the kernel holds it to that; a rest waits for the next block): steady state, what the
    // block made; a first gather, whatever the ring holds
    const int64_t n_k = std::max<int64_t>(0, t.c->pos.blk_after - t.c->pos.blk_before);
    // (a hard stream: what its framing rule allows with the slicer's bits per symbol; 2, the larger figure, should a hard row
    // ever come without a slicer)
    const Chan::Slicer *sl = t.c->slicer.get();
    const int64_t hard = hard_bound(t.kind, n_k, sl ? sl->rec.bps : 2);
    // (the capture stage's two streams: what the gate's rule allows, capture_bound / capture_rec_bound of rcf_streams.h)
    const Chan::Capture *cp = t.c->capture.get();
    const int64_t steady = t.kind == kCapture ? capture_bound(n_k)
                         : t.kind == kCaptureRec ? capture_rec_bound(n_k, cp ? cp->rec.pre : 0, cp ? cp->rec.hang : 0)
                         : hard < 0 ? steady_bound(n_k, st.interp, st.decim) : hard;
    const int64_t R = (int64_t)p->ring_items(e);
    const int64_t bound = std::min<int64_t>(fresh || again ? (int64_t)st.cap : steady, R);
    int64_t *cs = p->d_cstate + (size_t)e * 4;
    const int par = t.par;
    t.par = !t.par;
    crecs[n_crecs] = CountedRec{static_cast<const uint32_t *>(st.ring), st.counter, cs + 2 * par, cs + 2 * (par ^ 1),
                                reinterpret_cast<int64_t *>(crecs_dev + p->recs_cap * sizeof(CountedRec)) + 2 * n_crecs,
                                fresh ? *st.cursor : 0, t.queued, st.interp, st.decim, st.cap,
                                (uint32_t)bound, (uint32_t)((size_t)e * p->out_cap * kSlotW), (uint32_t)((size_t)R * st.item_w - 1),
                                fresh ? 3u : again ? 1u : 0u, st.item_w};
    s.counted.push_back({e, t.gen, bound, n_crecs++});
    max_c = std::max<uint32_t>(max_c, (uint32_t)bound * st.item_w);
    t.queued += bound;
    // (published BEFORE the launch, like a plain slot's: covers all this gather may write)
    p->out_queued[(size_t)e].store(t.queued, std::memory_order_release);
}

int Gather::launch()
{
    uint32_t *out = reinterpret_cast<uint32_t *>(p->h_out_dev);
    launch_gather_rings(reinterpret_cast<const GatherRec *>(p->h_recs_dev + (size_t)block * p->recs_cap * sizeof(GatherRec)), n_recs, out, max_w, p->g->stream);
    launch_gather_counted(reinterpret_cast<const CountedRec *>(crecs_dev), n_crecs, out, max_c, p->g->stream);
    if (hipEventRecord(p->slot_ev[block], p->g->stream) != hipSuccess) { set_error("pump: event record failed"); return RCF_EHIP; }
    return RCF_OK;
}

// What the counted gathers of the finished block `s` took: each slot's true item count from its result words; the bound
// goes back on it, plus what the other block in flight may still take (under g->mu).  Returns the items delivered
int64_t rebase_counted(rcf_pump *p, const InFlight &s, const InFlight &other, const int64_t *res)
{
    int64_t items_out = 0;
    for (const InFlight::Counted &c : s.counted) {
        const size_t e = (size_t)c.entry;
        rcf_pump::Slot &t = p->slots[e];
        if (c.gen != t.gen) continue;                                 // the slot has a new tenant, whose stream began above this
        const int64_t now_at = res[2 * c.rec];
        int64_t ahead = 0;
        if (other.busy) for (const InFlight::Counted &o : other.counted) if (o.entry == c.entry && o.gen == c.gen) ahead += o.bound;
        items_out += now_at - p->out_written[e].load(std::memory_order_relaxed);
        p->out_written[e].store(now_at, std::memory_order_release);
        t.queued = now_at + ahead;
        p->out_queued[e].store(t.queued, std::memory_order_release);
    }
    return items_out;
}

void pump_main(rcf_pump *p)
{
    rcf_group *g = p->g;
    const rcf_pump_config_t &cfg = p->cfg;
    const size_t G = g->members.size();
    if (cfg.cpu >= 0) {
        cpu_set_t set;
        CPU_ZERO(&set);
        CPU_SET(cfg.cpu, &set);
        (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
    }
    if (cfg.rt_priority > 0) {
        sched_param sp{};
        sp.sched_priority = cfg.rt_priority;
        p->rt_granted.store(pthread_setschedparam(pthread_self(), SCHED_FIFO, &sp) == 0 ? 1 : 0);
    }
    (void)hipSetDevice(g->device);
    const int sfd = open("/proc/thread-self/schedstat", O_RDONLY | O_CLOEXEC);
    long long rq_warm = -1;                        // run_delay / involuntary switches when the judged region began
    long nv_warm = 0;
    const double period = (double)cfg.block_samples / cfg.samp_rate;
    const size_t blk_bytes = cfg.block_samples * group_sample_bytes(cfg.fmt);
    const Clock::time_point t0 = Clock::now() + std::chrono::duration_cast<Clock::duration>(std::chrono::duration<double>(cfg.start_delay_s));
    { std::lock_guard<std::mutex> l(p->st_mu); p->t_start = t0; }
    std::vector<int64_t> next_k(G, 0);             // next block of each member
    std::vector<double> seen_at(G, -1.0);          // counter-fed members: when the pump first saw block next_k complete
    InFlight slots[2];
    int head = 0, in_flight = 0;                   // slots[head] is the oldest busy one
    std::vector<GroupItem> items;

    auto complete_oldest = [&](bool block) -> bool {
        InFlight &s = slots[head];
        if (!s.busy) return false;
        if (!block && hipEventQuery(p->slot_ev[head]) != hipSuccess) { (void)hipGetLastError(); return false; }
        const long long rq0 = run_delay_ns(sfd);
        const Clock::time_point w0 = Clock::now();
        if (hipEventSynchronize(p->slot_ev[head]) != hipSuccess) { set_error("pump: event wait failed"); pump_fail(p, RCF_EHIP); return false; }
        const Clock::time_point now = Clock::now();
        const long long rq1 = secs(now - w0) > 5e-3 ? run_delay_ns(sfd) : -1;
        const double t_done = secs(now - t0);
        int64_t items_out = 0;
        for (auto &d : s.delivered) { p->out_written[(size_t)d.first].fetch_add(d.second, std::memory_order_release); items_out += d.second; }
        if (!s.counted.empty()) {
            std::lock_guard<std::mutex> gl(g->mu);
            items_out += rebase_counted(p, s, slots[head ^ 1], reinterpret_cast<const int64_t *>(p->h_crecs + (size_t)head * p->crecs_bytes() + p->recs_cap * sizeof(CountedRec)));
        }
        {
            std::lock_guard<std::mutex> l(p->st_mu);
            p->wait_ms += secs(now - w0) * 1e3;
            if (p->warm_done) {
                p->max_wait_ms = std::max(p->max_wait_ms, secs(now - w0) * 1e3);
                if (secs(now - w0) > 5e-3) {
                    ++p->slow_waits;
                    p->slow_wait_total_ms += secs(now - w0) * 1e3;
                    if (rq0 >= 0 && rq1 >= 0) p->runq_in_slow_waits_ms += (double)(rq1 - rq0) * 1e-6;
                }
            }
            p->samples_out += items_out;
            for (size_t i = 0; i < s.members.size(); ++i) {
                ++p->blocks_done;
                if (s.kidx[i] >= cfg.warm_blocks) {
                    const double lat = t_done - s.due[i];
                    p->lat_ms.push_back((float)(lat * 1e3));
                    ++p->judged;
                    if (lat > period) ++p->late;
                }
            }
        }
        s.busy = false;
        head ^= 1;
        --in_flight;
        return true;
    };

    while (!p->stop.load(std::memory_order_relaxed) && !p->error.load()) {
        // members whose next block is complete
        const double now_s = secs(Clock::now() - t0);
        items.clear();
        std::vector<double> due;
        double next_due = 1e300;
        bool all_finished = true;
        for (size_t m = 0; m < G; ++m) {
            const int64_t k = next_k[m];
            if (cfg.n_blocks > 0 && k >= cfg.n_blocks) continue;
            all_finished = false;
            if (cfg.max_batch > 0 && (int)items.size() >= cfg.max_batch) { next_due = std::min(next_due, now_s); continue; }
            double d;
            if (p->written[m]) {
                if (*p->written[m] <= (uint64_t)k) { next_due = std::min(next_due, now_s + 50e-6); continue; }
                if (seen_at[m] < 0) seen_at[m] = now_s;
                d = seen_at[m];
            } else {
                d = (double)(k + 1) * period + p->phase[m];
                if (d > now_s) { next_due = std::min(next_due, d); continue; }
            }
            const size_t at = (size_t)(k % (int64_t)p->ring_blocks[m]) * blk_bytes;
            items.push_back(GroupItem{(int)m, cfg.block_samples, p->rings[m] + at, p->rings_dev[m] ? p->rings_dev[m] + at : nullptr});
            due.push_back(d);
        }
        if (all_finished && in_flight == 0) break;
        // batching window: the first block that is complete waits up to batch_window_s for company -- every block that
        // completes meanwhile rides in the same launches (at K front-ends a block completes every period / K)
        bool hold = false;
        if (!items.empty() && cfg.batch_window_s > 0 && !(cfg.max_batch > 0 && (int)items.size() >= cfg.max_batch)) {
            const double oldest = *std::min_element(due.begin(), due.end());
            if (now_s - oldest < cfg.batch_window_s) { hold = true; next_due = std::min(next_due, oldest + cfg.batch_window_s); }
        }
        if (!items.empty() && !hold && in_flight < 2) {
            const Clock::time_point p0 = Clock::now();
            const int slot = head ^ (in_flight & 1);
            InFlight &s = slots[slot];
            s.members.clear();
            s.kidx.clear();
            s.due = due;
            s.delivered.clear();
            s.counted.clear();
            int n_over = 0;
            for (size_t i = 0; i < items.size(); ++i) {
                s.members.push_back(items[i].m);
                s.kidx.push_back(next_k[(size_t)items[i].m]);
                if (now_s - due[i] > period && next_k[(size_t)items[i].m] >= cfg.warm_blocks) ++n_over;
            }
            int rc;
            {
                std::lock_guard<std::mutex> gl(g->mu);
                MemberLocks ml(g->members);
                rc = group_process(g, items, cfg.fmt, cfg.scale, cfg.offset, false);
                if (rc == RCF_OK) {
                    Gather ga{p, slot, s, reinterpret_cast<GatherRec *>(p->h_recs + (size_t)slot * p->recs_cap * sizeof(GatherRec)),
                              reinterpret_cast<CountedRec *>(p->h_crecs + (size_t)slot * p->crecs_bytes()), p->h_crecs_dev + (size_t)slot * p->crecs_bytes()};
                    for (const GroupItem &it : items) {
                        rcf_t *h = g->members[(size_t)it.m];
                        if (p->epoch_of[(size_t)it.m] != h->chans_epoch) resolve_member(p, it.m, h);
                        for (int e : p->entries_of[(size_t)it.m]) {
                            Stream st;
                            if (!slot_stream(p->slots[(size_t)e], h, &st)) continue;
                            if (st.counter) ga.counted(e, st); else ga.plain(e, st);
                        }
                    }
                    rc = ga.launch();
                }
            }
            if (rc != RCF_OK) { pump_fail(p, rc); break; }
            for (const GroupItem &it : items) { ++next_k[(size_t)it.m]; seen_at[(size_t)it.m] = -1.0; }
            s.busy = true;
            ++in_flight;
            {
                std::lock_guard<std::mutex> l(p->st_mu);
                p->plan_ms += secs(Clock::now() - p0) * 1e3;
                if (!p->warm_done && *std::min_element(s.kidx.begin(), s.kidx.end()) >= cfg.warm_blocks) {
                    p->warm_done = true;
                    rq_warm = run_delay_ns(sfd);
                    nv_warm = thread_nivcsw();
                }
                if (p->warm_done) {
                    p->max_plan_ms = std::max(p->max_plan_ms, secs(Clock::now() - p0) * 1e3);
                    if (secs(Clock::now() - p0) > 5e-3) ++p->slow_plans;
                }
                ++p->group_blocks;
                p->max_batch = std::max<int64_t>(p->max_batch, (int64_t)items.size());
                p->overruns += n_over;
            }
            (void)complete_oldest(false);          // (usually the previous batch has finished by now)
            continue;
        }
        if (in_flight > 0) {
            // nothing to queue (or both slots taken): the oldest batch's outputs are what the host waits for
            if ((!items.empty() && !hold) || next_due - now_s > 200e-6) { (void)complete_oldest(true); continue; }
            if (complete_oldest(false)) continue;
        }
        const double wait_s = next_due - secs(Clock::now() - t0);
        if (wait_s > 0) {
            const double want = std::min(wait_s, 1e-3);
            const long long rq0 = run_delay_ns(sfd);
            const Clock::time_point s0 = Clock::now();
            if (cfg.spin_us > 0 && want <= cfg.spin_us * 1e-6) {
                while (secs(Clock::now() - s0) < want && !p->stop.load(std::memory_order_relaxed)) __builtin_ia32_pause();
            } else {
                std::this_thread::sleep_for(std::chrono::duration<double>(cfg.spin_us > 0 ? want - cfg.spin_us * 0.5e-6 : want));
                while (secs(Clock::now() - s0) < want && cfg.spin_us > 0) __builtin_ia32_pause();
            }
            const double over = (secs(Clock::now() - s0) - want) * 1e3;      // how much later than asked the thread came back
            if (p->warm_done && over > 2.0) {
                const long long rq1 = run_delay_ns(sfd);
                std::lock_guard<std::mutex> l(p->st_mu);
                ++p->slow_sleeps;
                p->max_idle_gap_ms = std::max(p->max_idle_gap_ms, over);
                p->slow_sleep_total_ms += over;
                if (rq0 >= 0 && rq1 >= 0) p->runq_in_slow_sleeps_ms += (double)(rq1 - rq0) * 1e-6;
            }
        }
    }
    while (in_flight > 0 && !p->error.load()) (void)complete_oldest(true);
    (void)hipStreamSynchronize(g->stream);
    {
        const long long rq_end = run_delay_ns(sfd);
        std::lock_guard<std::mutex> l(p->st_mu);
        p->t_end = Clock::now();
        if (rq_warm >= 0 && rq_end >= 0) p->runq_total_ms = (double)(rq_end - rq_warm) * 1e-6;
        p->nivcsw = thread_nivcsw() - nv_warm;
    }
    if (sfd >= 0) close(sfd);
    p->running.store(false);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ pump
int rcf_pump_start(rcf_group_t *g, const rcf_pump_config_t *cfg, rcf_pump_t **out)
{
    if (!g || !cfg || !out || cfg->block_samples == 0 || !(cfg->samp_rate > 0) || !cfg->rings || !cfg->ring_blocks ||
        cfg->n_read < 0 || (cfg->n_read && (!cfg->read_members || !cfg->read_chans)) ||
        stream_kind(cfg->what) < 0 || !kStreams[stream_kind(cfg->what)].pumped || group_sample_bytes(cfg->fmt) == 0) {
        set_error("bad pump configuration");
        return RCF_EINVAL;
    }
    std::lock_guard<std::mutex> gl(g->mu);
    if (g->pump) { set_error("the group already has a pump"); return RCF_ESTATE; }
    RCF_HIP(hipSetDevice(g->device));
    const size_t G = g->members.size();
    std::unique_ptr<rcf_pump> p(new rcf_pump);
    p->g = g;
    p->cfg = *cfg;
    for (size_t m = 0; m < G; ++m) {
        if (!cfg->rings[m] || cfg->ring_blocks[m] == 0) { set_error("member %zu has no source ring", m); return RCF_EINVAL; }
        if (cfg->block_samples > g->members[m]->block_cap) { set_error("block of %zu samples exceeds member %zu's capacity", cfg->block_samples, m); return RCF_ECAP; }
        p->rings.push_back(static_cast<const unsigned char *>(cfg->rings[m]));
        void *rdv = nullptr;
        if (hipHostGetDevicePointer(&rdv, const_cast<void *>(cfg->rings[m]), 0) != hipSuccess) { rdv = nullptr; (void)hipGetLastError(); }
        p->rings_dev.push_back(static_cast<const unsigned char *>(rdv));
        p->ring_blocks.push_back(cfg->ring_blocks[m]);
        p->phase.push_back(cfg->phase_s ? cfg->phase_s[m] : 0.0);
        p->written.push_back(cfg->written ? cfg->written[m] : nullptr);
    }
    const int n_slots = std::max(std::max(cfg->n_read, cfg->max_read), 1);
    p->entries_of.resize(G);
    p->slots.resize((size_t)n_slots);
    p->epoch_of.assign(G, ~0ull);
    for (int e = 0; e < cfg->n_read; ++e)
        if (cfg->read_members[e] < 0 || cfg->read_members[e] >= (int)G) { set_error("subscribed channel %d: no such member", e); return RCF_EINVAL; }
    // the configuration's arrays belong to the caller: from here on the pump's own copies are used
    p->cfg.rings = nullptr; p->cfg.ring_blocks = nullptr; p->cfg.phase_s = nullptr; p->cfg.written = nullptr;
    p->cfg.read_members = nullptr; p->cfg.read_chans = nullptr;
    p->out_cap = pow2_at_least(cfg->out_ring_samples ? cfg->out_ring_samples : 4096);
    const size_t out_bytes = std::max<size_t>(64, (size_t)n_slots * p->out_cap * rcf_pump::kSlotItemBytes);
    if ((uint64_t)out_bytes / 4 > 0xffffffffull) { set_error("host rings of %zu bytes exceed the 32-bit word range", out_bytes); return RCF_ECAP; }
    if (!pinned_alloc(out_bytes, &p->h_out, &p->h_out_dev, "host rings")) return RCF_ENOMEM;
    p->out_written.reset(new std::atomic<int64_t>[(size_t)n_slots]);
    p->out_queued.reset(new std::atomic<int64_t>[(size_t)n_slots]);
    for (int e = 0; e < n_slots; ++e) { p->out_written[(size_t)e].store(0); p->out_queued[(size_t)e].store(0); }
    p->recs_cap = (size_t)n_slots;
    if (!pinned_alloc(2 * p->recs_cap * sizeof(GatherRec), &p->h_recs, &p->h_recs_dev, "gather records") ||      // (~rcf_pump releases
        !pinned_alloc(2 * p->crecs_bytes(), &p->h_crecs, &p->h_crecs_dev, "counted-gather records")) return RCF_ENOMEM;   // what there is)
    RCF_HIP(hipMalloc(&p->d_cstate, (size_t)n_slots * 4 * sizeof(int64_t)));
    RCF_HIP(hipMemset(p->d_cstate, 0, (size_t)n_slots * 4 * sizeof(int64_t)));
    for (int i = 0; i < 2; ++i) RCF_HIP(hipEventCreateWithFlags(&p->slot_ev[i], hipEventDisableTiming));
    // room in the group's arena for a group block of ALL members at once (after a hiccup everything that is complete goes
    // out together): growing the arena means a stream synchronisation and pinned allocations -- not in the middle of a run
    {
        MemberLocks ml(g->members);
        size_t all = 65536;
        for (rcf_t *h : g->members) all += arena_need_bound(h) + 1024;
        if (!g->arenas.h[0] && g->arenas.cap < all) { size_t c_ = g->arenas.cap; while (c_ < all) c_ *= 2; g->arenas.cap = c_; }
        if (g->arenas.reserve(all, g->stream) != RCF_OK) return RCF_EHIP;
    }
    // the configured subscriptions; their readers start at what has been produced so far
    {
        MemberLocks ml(g->members);
        for (int e = 0; e < cfg->n_read; ++e) {
            const int m = cfg->read_members[e], chan = cfg->read_chans[e];
            rcf_t *h = g->members[(size_t)m];
            if (chan >= RCF_SRC_PFB_BIN0) { p->occupy(e, m, chan, kFm, cfg->gain, h->pfb.produced); continue; }   // a bin of the fused discriminator ring
            p->occupy(e, m, chan, stream_kind(cfg->what), cfg->gain);
            auto f = h->chans.find(chan);
            if (f == h->chans.end()) continue;
            Stream st;
            int64_t two[2];
            if (chan_stream(h, f->second.get(), p->slots[(size_t)e].kind, &st) != RCF_OK) continue;
            // (a counted stream's end is fetched from the device here -- the one place the pump may wait for the stream; the
            // slot's first gather takes the cursor from there)
            if (!st.counter) *st.cursor = st.end;
            else if (stream_count(h, st, &st.end, two) == RCF_OK) *st.cursor = st.end;
        }
    }
    p->running.store(true);
    g->pump = p.get();
    rcf_pump *raw = p.release();
    raw->th = std::thread(pump_main, raw);
    *out = raw;
    return RCF_OK;
}

int rcf_pump_stats(rcf_pump_t *p, rcf_pump_stats_t *st)
{
    if (!p || !st) return RCF_EINVAL;
    std::vector<float> lat;
    {
        std::lock_guard<std::mutex> l(p->st_mu);
        st->blocks_done = p->blocks_done;
        st->blocks_judged = p->judged;
        st->late = p->late;
        st->overruns = p->overruns;
        st->group_blocks = p->group_blocks;
        st->max_batch = p->max_batch;
        st->samples_out = p->samples_out;
        st->host_plan_ms = p->plan_ms;
        st->host_wait_ms = p->wait_ms;
        st->max_plan_ms = p->max_plan_ms;
        st->max_wait_ms = p->max_wait_ms;
        st->max_sleep_overshoot_ms = p->max_idle_gap_ms;
        st->slow_plans = p->slow_plans;
        st->slow_waits = p->slow_waits;
        st->slow_sleeps = p->slow_sleeps;
        st->cpu = p->cfg.cpu;
        st->runq_ms_total = p->runq_total_ms;
        st->slow_wait_ms_total = p->slow_wait_total_ms;
        st->runq_ms_in_slow_waits = p->runq_in_slow_waits_ms;
        st->slow_sleep_ms_total = p->slow_sleep_total_ms;
        st->runq_ms_in_slow_sleeps = p->runq_in_slow_sleeps_ms;
        st->involuntary_switches = p->nivcsw;
        const bool run = p->running.load();
        st->elapsed_s = secs((run ? Clock::now() : p->t_end) - p->t_start);
        st->running = run ? 1 : 0;
        st->rt_priority_granted = p->rt_granted.load();
        st->error = p->error.load();
        lat = p->lat_ms;
    }
    st->latency_ms_p50 = st->latency_ms_p99 = st->latency_ms_max = 0.0;
    if (!lat.empty()) {
        std::sort(lat.begin(), lat.end());
        st->latency_ms_p50 = lat[lat.size() / 2];
        st->latency_ms_p99 = lat[std::min(lat.size() - 1, (size_t)(0.99 * (double)lat.size()))];
        st->latency_ms_max = lat.back();
    }
    if (st->error) set_error("pump stopped: %s", p->err_text);
    return RCF_OK;
}

int64_t rcf_pump_written(rcf_pump_t *p, int entry)
{
    if (!p || entry < 0 || entry >= (int)p->slots.size()) return RCF_EINVAL;
    return p->out_written[(size_t)entry].load(std::memory_order_acquire);
}

// one slot's new items from *cursor on -> out; the items the pump has meanwhile queued over (up to two gathers are in flight and
// write [written, queued) of the ring -- the oldest region a lagging reader may be copying) are dropped from the
// front AFTER the copy, so that what is returned was whole when it was read.  The ring is the slot's own: R of its items
static int64_t pump_read_slot(rcf_pump *p, int entry, int64_t *cursor, unsigned char *out, size_t max_items)
{
    const size_t elem = p->item_bytes(entry), R = p->ring_items(entry);
    const int64_t w = p->out_written[(size_t)entry].load(std::memory_order_acquire);
    int64_t avail = w - *cursor;
    if (avail <= 0 || max_items == 0) return 0;
    const int64_t q0 = p->out_queued[(size_t)entry].load(std::memory_order_acquire);
    if (*cursor < q0 - (int64_t)R) { *cursor = q0 - (int64_t)R; avail = w - *cursor; if (avail <= 0) return 0; }
    int64_t n = std::min<int64_t>(avail, (int64_t)max_items);
    const unsigned char *ring = p->h_out + (size_t)entry * p->out_cap * rcf_pump::kSlotItemBytes;
    const size_t pos = (size_t)((uint64_t)*cursor & (R - 1));
    const size_t first = std::min<size_t>((size_t)n, R - pos);
    std::memcpy(out, ring + pos * elem, first * elem);
    if ((size_t)n > first) std::memcpy(out + first * elem, ring, ((size_t)n - first) * elem);
    std::atomic_thread_fence(std::memory_order_acquire);
    const int64_t lo = p->out_queued[(size_t)entry].load(std::memory_order_acquire) - (int64_t)R;
    if (lo > *cursor) {                               // overwritten while it was copied: what is left starts at lo
        const int64_t drop = std::min<int64_t>(n, lo - *cursor);
        if (drop < n) std::memmove(out, out + (size_t)drop * elem, (size_t)(n - drop) * elem);
        *cursor += drop;
        n -= drop;
    }
    *cursor += n;
    return n;
}

int64_t rcf_pump_read(rcf_pump_t *p, int entry, int64_t *cursor, void *out, size_t max_items)
{
    if (!p || !cursor || !out || entry < 0 || entry >= (int)p->slots.size()) { set_error("bad pump read arguments"); return RCF_EINVAL; }
    return pump_read_slot(p, entry, cursor, static_cast<unsigned char *>(out), max_items);
}

int rcf_pump_read_many(rcf_pump_t *p, const int *entries, int64_t *cursors, int n, void *out, size_t cap_each, int64_t *counts)
{
    if (!p || n < 0 || (n && (!entries || !cursors || !out || !counts))) { set_error("bad pump read arguments"); return RCF_EINVAL; }
    for (int i = 0; i < n; ++i) {
        if (entries[i] < 0 || entries[i] >= (int)p->slots.size()) { counts[i] = -1; continue; }
        // (row i is cap_each x 8 bytes whatever the slot delivers: cap_each items of up to 8 bytes, cap_each / 4 records)
        counts[i] = pump_read_slot(p, entries[i], &cursors[i], static_cast<unsigned char *>(out) + (size_t)i * cap_each * rcf_pump::kSlotItemBytes,
                                   (size_t)slot_items(p->slots[(size_t)entries[i]].kind, (int64_t)cap_each));
    }
    return RCF_OK;
}

// a subscription of either entry point: `kind` is the reader's kind of `what`, which the entry point has admitted
static int pump_subscribe(rcf_pump *p, int member, int chan_id, int what, int kind, float gain, int64_t *cursor)
{
    rcf_group *g = p->g;
    std::lock_guard<std::mutex> gl(g->mu);
    if (member < 0 || member >= (int)g->members.size()) { set_error("no such member %d", member); return RCF_EINVAL; }
    int e = -1;
    for (size_t i = 0; i < p->slots.size(); ++i) if (p->slots[i].member < 0) { e = (int)i; break; }
    if (e < 0) { set_error("all %zu subscription slots of the pump are taken (rcf_pump_config_t.max_read)", p->slots.size()); return RCF_ECAP; }
    rcf_t *h = g->members[(size_t)member];
    int64_t bin_start = 0;
    {
        // (the channel's own reader position is left where it is: a channel nobody has read yet is delivered from its
        // first output on -- what rcf_chan_read_iq would have handed out -- as far as its device ring still holds it)
        std::lock_guard<std::mutex> l(h->mu);
        if (chan_id >= RCF_SRC_PFB_BIN0) {
            // a bin of the member's fused discriminator ring (rcf_pfb_fm_enable): delivered from the bank's next frame on
            const int bin = chan_id - RCF_SRC_PFB_BIN0;
            Stream st;
            if (what != RCF_READ_FM || !pfb_fm_stream(h, bin, nullptr, true, &st)) {
                set_error("member %d has no fused discriminator ring with a bin %d (rcf_pfb_fm_enable; what = RCF_READ_FM)", member, bin);
                return RCF_EINVAL;
            }
            bin_start = st.end;
        } else if (h->chans.find(chan_id) == h->chans.end()) {
            set_error("no such channel %d on member %d", chan_id, member);
            return RCF_EINVAL;
        }
    }
    p->occupy(e, member, chan_id, kind, gain, bin_start);
    // the new stream starts at `queued`, which the reader's cursor is set to (the gathers still in flight for the previous
    // tenant end below it)
    if (cursor) *cursor = p->slots[(size_t)e].queued;
    return e;
}

int rcf_pump_subscribe(rcf_pump_t *p, int member, int chan_id, int what, float gain, int64_t *cursor)
{
    // (the captured stream of rcf_chan_capture stands behind the table: the one row there this entry point delivers)
    if (p && what == RCF_READ_CAPTURE && chan_id < RCF_SRC_PFB_BIN0) return pump_subscribe(p, member, chan_id, what, kCapture, 1.0f, cursor);
    if (!p || stream_kind(what) < 0 || !kStreams[stream_kind(what)].pumped) { set_error("bad subscription"); return RCF_EINVAL; }
    return pump_subscribe(p, member, chan_id, what, stream_kind(what), gain, cursor);
}

// The streams behind the slicer.  The table's `pumped` column and stream_kind stay what the two entry points above refuse
// by; this one admits exactly the counted uint32 rows, of the table and behind it
int rcf_pump_subscribe_hard(rcf_pump_t *p, int member, int chan_id, int what, int64_t *cursor)
{
    const int kind = row_kind(what);
    if (!p || kind < 0 || (hard_bound(kind, 0, 1) < 0 && kind != kCaptureRec) || chan_id >= RCF_SRC_PFB_BIN0) { set_error("bad subscription: %d is no stream behind a slicer", what); return RCF_EINVAL; }
    if (slot_items(kind, (int64_t)p->out_cap) < 16) {
        set_error("host rings of %zu x 8 bytes hold fewer than 16 items of stream %d (rcf_pump_config_t.out_ring_samples)", p->out_cap, what);
        return RCF_ECAP;
    }
    return pump_subscribe(p, member, chan_id, what, kind, 1.0f, cursor);
}

int rcf_pump_unsubscribe(rcf_pump_t *p, int entry)
{
    if (!p) return RCF_EINVAL;
    rcf_group *g = p->g;
    std::lock_guard<std::mutex> gl(g->mu);
    if (entry < 0 || entry >= (int)p->slots.size() || p->slots[(size_t)entry].member < 0) { set_error("no such subscription %d", entry); return RCF_EINVAL; }
    p->vacate(entry);
    return RCF_OK;
}

int rcf_pump_stop(rcf_pump_t *p)
{
    if (!p) return RCF_EINVAL;
    p->stop.store(true);
    if (p->th.joinable()) p->th.join();
    rcf_group *g = p->g;
    {
        std::lock_guard<std::mutex> gl(g->mu);
        (void)hipSetDevice(g->device);
        (void)hipStreamSynchronize(g->stream);
        g->pump = nullptr;
    }
    delete p;                                          // (~rcf_pump: events, records, rings)
    return RCF_OK;
}

}  // extern "C"
