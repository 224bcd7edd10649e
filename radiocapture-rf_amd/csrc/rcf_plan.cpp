// rcf_plan.cpp -- the per-block schedule.  Everything one commit schedules is built on the host first (a BlockPlan:
// launch records in the pinned arena, jobs per dependency depth), then uploaded with one copy and launched in
// dependency order (rcf_launch.cpp).  process_block() is the sequence; the plan_*() functions each build one part.
#include <atomic>
#include <chrono>

#include "rcf_plan.h"

namespace rcfx {

namespace {
std::atomic<uint64_t> g_prof_ns[PlanProf::N];
std::atomic<uint64_t> g_prof_cnt[PlanProf::N];
std::atomic<uint64_t> g_prof_max[PlanProf::N];
const char *g_prof_name[PlanProf::N];
void prof_dump()
{
    for (int i = 0; i < PlanProf::N; ++i)
        if (g_prof_cnt[i].load())
            fprintf(stderr, "RCF_PLAN_PROF %-28s %10.3f ms  %9llu calls  %8.3f us/call  %10.3f us longest\n",
                    g_prof_name[i] ? g_prof_name[i] : "?", g_prof_ns[i].load() * 1e-6, (unsigned long long)g_prof_cnt[i].load(),
                    g_prof_ns[i].load() * 1e-3 / (double)g_prof_cnt[i].load(), g_prof_max[i].load() * 1e-3);
}
}  // namespace

bool PlanProf::on()
{
    static const bool v = [] {
        const char *e = getenv("RCF_PLAN_PROF");
        const bool o = e && atoi(e) != 0;
        if (o) atexit(prof_dump);
        return o;
    }();
    return v;
}

void PlanProf::add(int slot, const char *name, std::chrono::steady_clock::time_point &from)
{
    const auto now = std::chrono::steady_clock::now();
    const uint64_t ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(now - from).count();
    g_prof_ns[slot] += ns;
    g_prof_cnt[slot] += 1;
    for (uint64_t m = g_prof_max[slot].load(); ns > m && !g_prof_max[slot].compare_exchange_weak(m, ns);) {}   // (several pump threads)
    g_prof_name[slot] = name;
    from = now;
}

// the channel set's planning summary (see rcf_t::PlanCache), rebuilt when a channel was opened or closed or changed kind
const rcf_t::PlanCache &plan_cache(rcf_t *h)
{
    rcf_t::PlanCache &pc = h->plan_cache;
    if (pc.epoch == h->chans_epoch) return pc;
    pc.reach_x.clear();
    pc.max_depth = 0; pc.min_d0 = 0; pc.max_reach = 1;
    // (one pass over the channel map for everything that needs one: at 196608 channels each pass is ~8 ms of
    // pointer chasing)
    size_t need = 4096, pfb_reach = 0, n_fir = 0;
    for (auto &kv : h->chans) {
        Chan &c = *kv.second;
        // (a filterbank tap has one short record; a FIR channel up to two launch records -- matrix-core launch and
        // zero-history fix-up --, a discriminator record, an exact-rotator fill, its bank-matrix dirty flag)
        need += c.is_tap ? sizeof(TapLaunch) + 8 : 2 * sizeof(ChanLaunch) + sizeof(DiscLaunch) + sizeof(RotFill) + 12 + 128;
        n_fir += c.is_tap ? 0 : 1;
        // a stage: its launch record, and how far behind a block's first output it reads the channel's own rings (the voice
        // chain's reach is into its own rings: the widest window only)
        c.for_each_stage([&](const auto &stage, size_t rec_bytes, bool own_rings) {
            if (!stage) return;
            const size_t reach = stage->reach();
            need += rec_bytes;
            if (!own_rings) { size_t &own = pc.reach_x[c.id]; own = std::max(own, reach); }
            pc.max_reach = std::max(pc.max_reach, reach);
        });
        pc.max_depth = std::max(pc.max_depth, c.depth);
        if (c.src < 0 && (pc.min_d0 == 0 || c.D < pc.min_d0)) pc.min_d0 = c.D;
        if (c.src >= RCF_SRC_PFB_BIN0) {              // (the bank's ring: one entry for all of its consumers, set after the loop)
            pfb_reach = std::max<size_t>(pfb_reach, (size_t)(c.T - 1 + c.D));
        } else if (c.src >= 0) {
            size_t &r = pc.reach_x[c.src];
            r = std::max<size_t>(r, (size_t)(c.T - 1 + c.D));
            pc.max_reach = std::max(pc.max_reach, r);
        }
    }
    if (pfb_reach) {
        size_t &r = pc.reach_x[RCF_SRC_PFB_BIN0];
        r = std::max(r, pfb_reach);
        pc.max_reach = std::max(pc.max_reach, r);
    }
    need += 64 * (n_fir / 4 + 64);                        // per-class alignment slack
    pc.arena_need = need;
    // channels by depth, then by (D, T) class (a front-end has a handful of classes: linear search, then sorted -- the
    // order classes are launched in is the key order, channels inside a class in id order)
    pc.by_depth.assign((size_t)pc.max_depth + 1, {});
    for (auto &kv : h->chans) {
        Chan *c = kv.second.get();
        auto &lvl = pc.by_depth[(size_t)c->depth];
        const std::pair<int, int> key{c->D, c->T};
        size_t q = 0;
        while (q < lvl.size() && lvl[q].first != key) ++q;
        if (q == lvl.size()) lvl.push_back(rcf_t::PlanCache::ClassBucket{key, {}});
        lvl[q].second.push_back(c);
    }
    for (auto &classes : pc.by_depth)
        std::sort(classes.begin(), classes.end(), [](const rcf_t::PlanCache::ClassBucket &a, const rcf_t::PlanCache::ClassBucket &b) { return a.first < b.first; });
    pc.epoch = h->chans_epoch;
    return pc;
}

// an upper bound of what plan_arena() will ask for, without planning anything (a group sizes its arena for all of its
// members before it plans any of them)
size_t arena_need_bound(rcf_t *h) { return plan_cache(h).arena_need; }

// arena for this commit: sized for every channel's launch records before anything is scheduled, so the schedule
// cannot run out half way (it mutates channel state as it goes); also the consumers' reach and the deepest chain
int plan_arena(rcf_t *h, BlockPlan &bp)
{
    const rcf_t::PlanCache &pc = plan_cache(h);
    bp.reach_x = &pc.reach_x;
    bp.max_depth = pc.max_depth;
    bp.min_d0 = pc.min_d0;
    bp.max_reach = pc.max_reach;
    bp.arena_need = pc.arena_need;
    const size_t arena_need = pc.arena_need;
    if (bp.ar != &bp.own_ar) return RCF_OK;        // a group's block: the group reserved its arena for all members
    // (a lagging stage-2 launch reads its records in the current arena: it goes out before the arenas are re-allocated or
    // the one it lives in can come round again)
    if (h->lag.pending && (arena_need > h->arenas.cap || h->arenas.fill + arena_need > h->arenas.cap)) flush_lagged(h);
    if (h->arenas.reserve(arena_need, h->stream) != RCF_OK) return RCF_EHIP;
    bp.a = h->arenas.cur;
    bp.arena_base = h->arenas.fill;
    bp.own_ar = Arena{h->arenas.h[bp.a], h->arenas.d[bp.a], bp.arena_base, h->arenas.cap};
    return RCF_OK;
}

// the filterbank's share of the block (derived channels need its new range)
int plan_pfb(rcf_t *h, BlockPlan &bp)
{
    const int64_t S0 = bp.S0, S1 = bp.S1;
    const size_t n = bp.n;
    PfbLaunch &pl = bp.pl;
    bool &run_pfb = bp.run_pfb;

    if (h->pfb.open) {
        Pfb &p = h->pfb;
        const int64_t n_lo = std::max(ceil_div(S0, p.D), p.n_abs0);
        const int64_t n_hi = floor_div(S1 - 1, p.D);
        p.produced_before = p.produced;
        if (n_hi >= n_lo) {
            const int64_t cnt = n_hi - n_lo + 1;
            if ((size_t)cnt + (bp.reach_x && bp.reach_x->count(RCF_SRC_PFB_BIN0) ? bp.reach_x->at(RCF_SRC_PFB_BIN0) : 0) > h->out_cap) {
                set_error("block yields %lld PFB frames (+%zu of history its stage-2 channels need) > ring capacity %zu",
                          (long long)cnt, bp.reach_x && bp.reach_x->count(RCF_SRC_PFB_BIN0) ? bp.reach_x->at(RCF_SRC_PFB_BIN0) : (size_t)0, h->out_cap);
                return RCF_ECAP;
            }
            if (p.fm_mode && p.d_fm_edge && ceil_div(cnt, p.shape.chunk_frames) > p.fm_slots) {
                // the look-back form's invariant: one hand-over row and flag per chunk of the launch (rcf_pfb_fm_enable
                // sizes them for the largest launch the handle accepts, so this does not fire); two chunks of one launch on
                // one row would wait for a tag that was overwritten and take a wrong predecessor frame
                set_error("block yields %lld chunks of the fused discriminator > %d hand-over rows",
                          (long long)ceil_div(cnt, p.shape.chunk_frames), p.fm_slots);
                return RCF_ECAP;
            }
            pl.src.base = h->d_buf[h->cur];
            pl.src.mask = ~0ull;
            pl.src.origin = S0 - (int64_t)h->hist_cap;
            pl.src.stride = 1;
            pl.frame_major = p.shape.frame_major ? 1 : 0;
            pl.ptaps = p.d_ptaps;
            pl.tw = p.d_tw;
            pl.bins_ring = p.d_bins;
            pl.ring_mask = h->ring_mask;
            pl.tile_pitch = pfb_tile_pitch(p.NB);
            pl.n_lo = n_lo;
            pl.n_abs0 = p.n_abs0;
            pl.start_sample = p.start_sample;
            pl.src_len = (int64_t)(h->hist_cap + n);
            pl.n_frames = (int32_t)cnt;
            pl.NB = p.NB; pl.D = p.D; pl.P = p.P;
            if (p.fm_mode) {                    // the discriminator of every bin, in the bank's own kernel (rcf_pfb_fm_enable)
                pl.fm_ring = p.d_fm;
                pl.fm_inc = p.d_fm_inc;
                pl.atan_tab = h->d_atan;
                pl.fm_mode = p.fm_mode;
                pl.fm_span = 0;                 // chosen at the launch (pfb5_fm_span_for)
                if (p.d_fm_edge) {              // look-back form: the chunks' workgroups hand their last frames over
                    pl.fm_edge = p.d_fm_edge;
                    pl.fm_flag = p.d_fm_flag;
                    pl.fm_err = p.d_fm_err;
                    pl.fm_slots = p.fm_slots;
                    pl.fm_local = p.fm_local;
                    // a tag of its own per launch: the rows and flags of the launch before are never taken for this one's.
                    // Launches of one bank are in stream order -- the handle's own stream, or, while it is a group member,
                    // the group's for all of them, single or grouped (rcf_group_open waits for the member's stream first,
                    // rcf_group_close for the group's) -- so no earlier launch writes a row this one reads.
                    pl.fm_tag = (unsigned long long)(++p.fm_serial) << 32;
                }
            } else {
                pl.fm_ring = nullptr;
                pl.fm_edge = nullptr;
                pl.fm_mode = 0;
            }
            // the one place a launch's zero-history question is asked: the launchers and the group take the answer.  A fused
            // launch also recomputes the chunk before its first frame (the halo)
            bp.shape = p.shape;
            bp.pfb_zero_history = pfb_zero_history(p.shape, n_lo, p.start_sample, p.fm_mode ? p.shape.chunk_frames : 0);
            run_pfb = true;
            bp.run_pfb_squelch = p.sq.on;
            p.produced = n_hi - p.n_abs0 + 1;
        }
    }
    return RCF_OK;
}

// ---- a channel's share of a block, in two steps: its source's new range, then what the channel makes of it.  plan_channel()
// and the dry pass (check_block_capacity) both take them, so the pass that refuses and the pass that plans cannot disagree.
namespace {

typedef std::pair<int64_t, int64_t> Range;     // [first, second)

// c's source in this block -- the wideband stream, a filterbank bin or another channel: its new samples and the view a
// kernel reads them through.  false: the source is closed, c starves.  What the block gave a source CHANNEL is the one
// thing the two passes know differently: chained(source) says it.
template <class Chained> bool block_source(rcf_t *h, const BlockPlan &bp, const Chan &c, Chained &&chained, SrcRange *sr)
{
    if (c.src < 0 || c.src >= RCF_SRC_PFB_BIN0) return source_range(h, c.src, bp.S0, bp.S1, sr);
    auto it = h->chans.find(c.src);
    if (it == h->chans.end()) return false;
    sr->view.base = it->second->d_iq;
    sr->view.mask = h->ring_mask;
    sr->view.origin = 0;
    sr->view.stride = 1;
    const Range r = chained(*it->second);
    sr->p0 = r.first;
    sr->p1 = r.second;
    return true;
}

struct Share {
    int64_t k_lo = 0, cnt = 0;      // outputs k_lo .. k_lo + cnt - 1 in the channel's absolute index; cnt == 0: none in this block
    int64_t n_lo = 0;               // k_lo relative to the channel's first output
    int64_t a_lo = 0, a_n = 0;      // a voice chain's part of them, from its start on (a_n <= 0: nothing yet)
};

// What c makes of its source's new samples [p0, p1) -- and the one place a block is refused for a ring too small: the
// channel's own (its outputs plus what its consumers still read behind them) or its voice chain's.  *s: a fresh Share.
// (Inlined: plan_channel takes this step for every channel of every block.)
__forceinline__ int block_share(const rcf_t *h, const BlockPlan &bp, const Chan &c, int64_t p0, int64_t p1, Share *s)
{
    const int64_t k_lo = std::max(ceil_div(p0, c.D), c.k_abs0);
    const int64_t k_hi = floor_div(p1 - 1, c.D);
    if (p1 <= p0 || k_hi < k_lo) return RCF_OK;
    s->k_lo = k_lo;
    s->cnt = k_hi - k_lo + 1;
    s->n_lo = k_lo - c.k_abs0;
    if ((size_t)s->cnt + bp.reach(c.id) > h->out_cap) {
        set_error("block yields %lld outputs (+%zu of history its consumers need) > ring capacity %zu",
                  (long long)s->cnt, bp.reach(c.id), h->out_cap);
        return RCF_ECAP;
    }
    if (c.audio) {
        s->a_lo = std::max(s->n_lo, c.audio->from);
        s->a_n = s->n_lo + s->cnt - s->a_lo;
        if (s->a_n > 0 && (size_t)s->a_n + c.audio->reach() > h->out_cap) {
            set_error("block yields %lld channel samples: audio rings of %zu too small", (long long)s->a_n, h->out_cap);
            return RCF_ECAP;
        }
    }
    return RCF_OK;
}

}  // namespace

// one channel's launch records and the advance of its state: range -> tap record or FIR record (+ exact-rotator fill) and
// discriminator record -> stages -> advance.  Returns RCF_OK also when the channel has nothing to do in this block.
int plan_channel(rcf_t *h, BlockPlan &bp, ClassPlan &cp, Chan *c)
{
    Chan::Pos &pos = c->pos;
    SrcRange sr{};
    const auto live = [&bp](const Chan &sc) {      // the source was planned before c (a smaller depth): its counters say
        const Chan::Pos &q = sc.pos;
        return q.blk_serial == bp.serial ? Range{q.blk_before, q.blk_after} : Range{q.produced, q.produced};
    };
    if (!block_source(h, bp, *c, live, &sr)) return RCF_OK;
    if (c->src >= 0) cp.shared_src = false;
    if (c->src < RCF_SRC_PFB_BIN0) cp.all_bank_src = false;
    Share s;
    const int rc = block_share(h, bp, *c, sr.p0, sr.p1, &s);
    if (rc != RCF_OK) return rc;
    const int64_t before = pos.produced;
    if (s.cnt == 0) { pos.blk_serial = bp.serial; pos.blk_before = pos.blk_after = before; return RCF_OK; }
    if (c->is_tap) {                            // served through the tap matrix, not by a FIR launch: its own short record
        TapLaunch tl{};
        tl.iq_ring = c->d_iq;
        tl.fm_ring = c->d_fm;
        tl.k_lo = s.k_lo; tl.k_abs0 = c->k_abs0; tl.n_seg0 = pos.n_seg0;
        tl.angle0 = (double)pos.angle0; tl.dangle = c->dangle; tl.logmag0 = pos.logmag0; tl.dlogmag = c->dlogmag;
        tl.n_k = (int32_t)s.cnt;
        tl.bin = c->src - RCF_SRC_PFB_BIN0;
        tl.fm_only = c->fm_only ? 1 : 0;
        bp.tap_list.push_back(tl);
        bp.tap_bins.push_back(tl.bin);
    } else {
        ChanLaunch L{};
        L.ctaps = c->d_ctaps;
        L.fm_ring = c->d_fm;
        L.iq_ring = c->d_iq;
        L.src = sr.view;
        L.k_lo = s.k_lo;
        L.k_abs0 = c->k_abs0;
        L.start_sample = c->start_sample;
        L.n_seg0 = pos.n_seg0;
        L.angle0 = (double)pos.angle0;
        L.dangle = c->dangle;
        L.logmag0 = pos.logmag0;
        L.dlogmag = c->dlogmag;
        L.n_k = (int32_t)s.cnt;
        // exact rotator: plain channels only (a filterbank tap's rotator carries the bank's own phases too)
        if (c->d_rot && c->extra_dangle == 0.0 && c->extra_dlogmag == 0.0) {
            L.rot_ring = c->d_rot;
            L.rot_mask = h->ring_mask;
            RotFill rf{};
            rf.ring = c->d_rot;
            rf.state = reinterpret_cast<float *>(c->d_rot + h->out_cap);
            rf.n_from = s.n_lo;
            rf.n_k = (int32_t)s.cnt;
            rf.incr_re = c->incr[0];
            rf.incr_im = c->incr[1];
            bp.rot_fills.push_back(rf);
        }
        DiscLaunch dl{};
        dl.iq_ring = c->d_iq;
        dl.fm_ring = c->d_fm;
        dl.n_lo = s.n_lo;
        dl.n_k = (int32_t)s.cnt;
        cp.launches.push_back(L);
        cp.launched.push_back(c);
        cp.discs.push_back(dl);
        cp.max_n = std::max(cp.max_n, (int)s.cnt);
    }
    // a stage's step: its record as attached, the new outputs from the stage's start on -> (n_lo, n_k); n_k <= 0: nothing yet
    const auto stage = [&s](auto rec, int64_t from, auto &recs) {
        rec.n_lo = std::max(s.n_lo, from);
        rec.n_k = (int32_t)(s.n_lo + s.cnt - rec.n_lo);
        if (rec.n_k > 0) recs.add(rec);
    };
    if (c->sym) stage(c->sym->rec, c->sym->from, bp.tails.symf);       // (Sym::from never exceeds `produced`: n_k is the block's count)
    if (c->agc) stage(c->agc->rec, c->agc->from, bp.tails.agcf);
    if (c->clock) stage(c->clock->rec, c->clock->from, bp.tails.clkf);
    // (the two loops behind another stage start where both have started: the AGC's start moves on a re-call)
    if (c->costas) stage(c->costas->rec, std::max(c->costas->from, c->agc->from), bp.tails.gcf);
    if (c->fsk4) stage(c->fsk4->rec, std::max(c->fsk4->from, c->sym->from), bp.tails.f4f);
    if (c->slicer) {                   // bounded by its source loop's n_k of this block: a loop makes at most one symbol per input
        const int src = c->slicer->source;
        const int64_t from = src == RCF_READ_CLOCK ? c->clock->from : src == RCF_READ_COSTAS ? std::max(c->costas->from, c->agc->from)
                                                                                              : std::max(c->fsk4->from, c->sym->from);
        SliceLaunch rec = c->slicer->rec;
        rec.n_k = (int32_t)(s.n_lo + s.cnt - std::max(s.n_lo, from));
        if (rec.n_k > 0) bp.tails.slf.add(rec);
        if (rec.n_k > 0)                   // the frame decoder behind it sees what this block's slicer launch wrote
            c->slicer->for_each_frames([&](const auto &f) {
                if (!f) return;
                auto fr = f->rec;
                fr.n_k = rec.n_k;
                bp.tails.of<decltype(fr)>().add(fr);
            });
    }
    if (c->squelch) stage(c->squelch->rec, c->squelch->from, bp.tails.sqf);
    if (c->capture) stage(c->capture->rec, c->capture->from, bp.tails.capf);
    if (c->audio && s.a_n > 0) {
        AudioLaunch al = c->audio->rec;
        al.n_lo = s.a_lo;
        al.n_k = (int32_t)s.a_n;
        bp.audf.push_back(al);
        bp.audf_max_n = std::max(bp.audf_max_n, (int)al.n_k);
        if ((double)al.interp / al.decim > bp.audf_ratio) {
            bp.audf_ratio = (double)al.interp / al.decim; bp.audf_num = al.interp; bp.audf_den = al.decim;
        }
    }
    // advance channel state: rebase the rotator model at the next output index
    const int64_t n_next = s.n_lo + s.cnt;
    const int64_t r512 = n_next & ~(int64_t)511;
    const long double adv = (long double)(n_next - pos.n_seg0) * (long double)c->dangle;
    pos.logmag0 = (r512 > pos.n_seg0) ? (double)(n_next - r512) * c->dlogmag
                                      : pos.logmag0 + (double)(n_next - pos.n_seg0) * c->dlogmag;
    pos.angle0 = fmodl(pos.angle0 + adv, (long double)kTwoPi);
    pos.n_seg0 = n_next;
    pos.produced = n_next;
    pos.blk_serial = bp.serial; pos.blk_before = before; pos.blk_after = n_next;
    return RCF_OK;
}

// ---- the launches of one (depth, D, T) class, three decisions: which channels take the matrix-core launch (split_class),
// the bank matrix that launch reads (plan_bank_matrix), and the jobs that result (plan_class_jobs)
namespace {

struct ClassSplit {
    std::vector<ChanLaunch> clean, fixups, rest;    // matrix-core launch, its zero-history fix-ups, vector launch
    std::vector<Chan *> clean_ch;
    int n_common = 0;                               // outputs per channel of the matrix-core launch
};

// Matrix-core path: channels on one shared source with one common output range.  A channel that was just
// opened still has outputs whose taps reach before its start (GR zero history) -- at most ceil((T-1)/D)
// of them, four for the reference's shapes.  It joins the matrix-core launch anyway (which computes those
// few outputs from real history, i.e. wrongly) and a vector-kernel launch AFTER it on the same stream
// rewrites just those outputs with the per-tap mask: opening 16384 channels at once used to put one
// whole block (70 ms) on the vector kernel.  Channels that start later inside the block keep the vector
// kernel for that block.
ClassSplit split_class(const rcf_t *h, ClassPlan &cp, int depth, int D, int T)
{
    ClassSplit sp;
    sp.n_common = cp.max_n;
    if (!(cp.shared_src && depth == 0 && mfma2_applicable(D, T, h->hist_cap, h->hist_cap + h->block_cap))) {
        sp.rest.swap(cp.launches);
        return sp;
    }
    int64_t k_common = -1;
    for (auto &L : cp.launches)                                 // the range most channels share: the earliest
        if (k_common < 0 || L.k_lo < k_common) { k_common = L.k_lo; sp.n_common = L.n_k; }
    const auto common = [&](const ChanLaunch &L) { return L.k_lo == k_common && L.n_k == sp.n_common; };
    const size_t n_ok = (size_t)std::count_if(cp.launches.begin(), cp.launches.end(), common);
    if (n_ok == cp.launches.size()) {              // the steady state: the whole class, no record copied
        sp.clean.swap(cp.launches);
        sp.clean_ch.swap(cp.launched);
    } else {
        sp.clean.reserve(n_ok);
        sp.clean_ch.reserve(n_ok);
        for (size_t i = 0; i < cp.launches.size(); ++i) {
            const ChanLaunch &L = cp.launches[i];
            if (!common(L)) { sp.rest.push_back(L); continue; }
            sp.clean.push_back(L);
            sp.clean_ch.push_back(cp.launched[i]);
        }
    }
    for (const ChanLaunch &L : sp.clean)
        if (L.k_lo * D - L.start_sample < (int64_t)(T - 1)) {
            // outputs k with k D - (T-1) < start: k < ceil((start + T - 1) / D)
            const int64_t k_end = ceil_div(L.start_sample + (int64_t)(T - 1), D);
            ChanLaunch F = L;
            F.n_k = (int32_t)std::min<int64_t>(L.n_k, std::max<int64_t>(0, k_end - L.k_lo));
            if (F.n_k > 0) sp.fixups.push_back(F);
        }
    // (no size limit on a class: every group of 32 channels has its own tap slab)
    if ((int)sp.clean.size() < kM2MinChans) {
        sp.rest.insert(sp.rest.end(), sp.clean.begin(), sp.clean.end());   // (order within a vector launch is free)
        sp.clean.clear();
        sp.clean_ch.clear();
        sp.fixups.clear();
    }
    return sp;
}

// The class's bank matrix for the matrix-core job mj over `chans`: as cached when membership and taps are what it was built
// from; else the job's pack launch rebuilds it -- all of it when it had to grow, otherwise the groups of 32 that changed.
int plan_bank_matrix(rcf_t *h, Arena &ar, std::pair<int, int> cls_key, const std::vector<Chan *> &chans, FirJob &mj)
{
    const int T = cls_key.second;
    rcf::BankCache &bc = h->banks[cls_key];
    std::vector<std::pair<int, uint64_t>> key;
    key.reserve(chans.size());
    for (Chan *c : chans) key.push_back({c->id, c->taps_version});
    mj.bc = nullptr;
    mj.dirty = nullptr;
    mj.repack = key != bc.key;
    if (mj.repack) {
        const size_t ng = (chans.size() + kM2Group - 1) / kM2Group;
        // + one chunk of slack: the kernel prefetches one chunk past a group's last
        const size_t need = ng * bank2_group_floats(T) + (size_t)kM2ChunkSteps * 1024;
        const bool fresh = need > bc.cap;
        // grow with headroom: a class that gains channels one by one must not reallocate each time
        const int rc = grow_buried(h, bc.d, bc.cap, need, std::max(need, bc.cap + bc.cap / 2));
        if (rc != RCF_OK) return rc;
        if (!fresh) {
            // rebuild only the groups of 32 whose membership or taps changed
            std::vector<unsigned char> dirty(ng, 0);
            for (size_t i = 0; i < key.size(); ++i)
                if (i >= bc.key.size() || bc.key[i] != key[i]) dirty[i / kM2Group] = 1;
            if (bc.key.size() > key.size())                      // the class shrank: its last group lost rows
                dirty[ng - 1] = 1;
            if (!ar.put(dirty, &mj.dirty)) return arena_full();
        }
        bc.key.clear();                           // stale until the pack launch is queued (FirJob::bc)
        mj.bc = &bc;
        mj.key = std::move(key);
    }
    mj.dims.bank = bc.d;
    return RCF_OK;
}

}  // namespace

// the jobs of the class: matrix-core job (+ zero-history fix-ups behind it), vector job, discriminator job
int plan_class_jobs(rcf_t *h, BlockPlan &bp, ClassPlan &cp, int depth, std::pair<int, int> cls_key)
{
    if (cp.launches.empty()) return RCF_OK;
    const int D = cls_key.first, T = cls_key.second;
    Arena &ar = *bp.ar;
    FirJob job{};
    job.bank_src = cp.all_bank_src;
    job.dims.D = D; job.dims.T = T; job.dims.KT = choose_kt(D, T);
    job.dims.chans_per_wg = cp.shared_src ? 16 : 1;
    job.dims.max_n_k = cp.max_n;
    job.dims.ring_mask = h->ring_mask;
    job.dims.atan_tab = h->d_atan;
    ClassSplit sp = split_class(h, cp, depth, D, T);
    int rc;
    if (!sp.clean.empty()) {
        FirJob mj = job;
        if ((rc = plan_bank_matrix(h, ar, cls_key, sp.clean_ch, mj)) != RCF_OK) return rc;
        mj.dims.n_chans = (int)sp.clean.size();
        mj.dims.mfma = 1;
        mj.dims.chans_per_wg = 128;
        mj.dims.max_n_k = sp.n_common;
        mj.dims.src_len = (int64_t)(h->hist_cap + bp.n);
        const MfmaPlan plan = mfma_plan((int)sp.clean.size(), sp.n_common, T);
        mj.dims.mfma_nt = plan.nt;
        mj.dims.mfma_parts = plan.parts;
        mj.dims.partial = nullptr;
        if (plan.parts > 1) {                       // split-K: one slab of partial sums per part
            const size_t need = (size_t)plan.parts * sp.clean.size() * (size_t)sp.n_common;
            if ((rc = grow_buried(h, h->d_partial, h->partial_cap, need, need)) != RCF_OK) return rc;
            mj.dims.partial = h->d_partial;
        }
        if (!ar.put(sp.clean, &mj.dev)) return arena_full();
        bp.fir_by_depth[depth].push_back(mj);
    }
    if (!sp.fixups.empty()) {                       // queued behind the matrix-core launch: see split_class
        FirJob fj = job;
        fj.bc = nullptr;
        fj.repack = false;
        fj.dirty = nullptr;
        fj.dims.n_chans = (int)sp.fixups.size();
        fj.dims.max_n_k = 0;
        for (auto &F : sp.fixups) fj.dims.max_n_k = std::max(fj.dims.max_n_k, (int)F.n_k);
        fj.dims.small = 0;
        fj.dims.mfma = 0;
        fj.dims.chans_per_wg = 1;                   // per-channel n_k differ: one channel per workgroup
        if (!ar.put(sp.fixups, &fj.dev)) return arena_full();
        bp.fir_by_depth[depth].push_back(fj);
    }
    if (!sp.rest.empty()) {
        job.dims.n_chans = (int)sp.rest.size();
        job.dims.small = (!cp.shared_src && fir_small_outputs(D, T) > 0) ? 1 : 0;
        // a group's block: launches whose records are self-contained (every channel its own source view) are merged
        // with the same class of the other front-ends -- the records stay on the host until the group has them all
        if (bp.defer && job.dims.chans_per_wg == 1) job.host.swap(sp.rest);
        else if (!ar.put(sp.rest, &job.dev)) return arena_full();
        bp.fir_by_depth[depth].push_back(std::move(job));
    }
    if (!(job.dims.small && sp.clean.empty())) {   // the small-T kernel writes the discriminator ring itself
        DiscJob dj;
        dj.host.swap(cp.discs);
        dj.max_n = cp.max_n;
        if (!bp.defer && !dj.upload(ar)) return arena_full();
        bp.disc_jobs.push_back(std::move(dj));
    }
    return RCF_OK;
}

// filterbank taps (matrix + records) and the records that go out as one launch each
int plan_tail(rcf_t *h, BlockPlan &bp)
{
    Arena &ar = *bp.ar;
    PfbLaunch &pl = bp.pl;
    if (!bp.tap_list.empty() && bp.run_pfb) {
        const size_t pitch = (bp.tap_list.size() + 15) & ~size_t(15);      // slots, whole groups of 16
        // Slot order: first every aligned run of 16 bins that is tapped completely (tap_finalize reads those from the
        // bank's ring: PfbLaunch::tap_first), then the remaining taps, which go through the matrix.
        const int NB = pl.NB;
        auto &first = bp.tap_first_of_bin;
        first.assign((size_t)NB, -1);
        for (size_t i = 0; i < bp.tap_list.size(); ++i)
            if (first[bp.tap_list[i].bin] < 0) first[bp.tap_list[i].bin] = (int32_t)i;
        auto &ordered = bp.tap_ordered;
        ordered.clear();
        ordered.reserve(bp.tap_list.size());
        std::vector<int32_t> group_bin0;
        group_bin0.reserve(pitch / 16);
        for (int b0 = 0; b0 + 16 <= NB && pl.fm_mode != 2; b0 += 16) {     // (fm_mode 2: the bank writes no bins ring to read runs from)
            bool full = true;
            for (int j = 0; j < 16 && full; ++j) full = first[b0 + j] >= 0;
            if (!full) continue;
            for (int j = 0; j < 16; ++j) {
                ordered.push_back(bp.tap_list[first[b0 + j]]);
                bp.tap_list[first[b0 + j]].bin = -1;            // taken
            }
            group_bin0.push_back(b0);
        }
        pl.tap_first = (int32_t)ordered.size();
        for (const TapLaunch &t : bp.tap_list)
            if (t.bin >= 0) ordered.push_back(t);
        bp.tap_list.swap(ordered);
        group_bin0.resize(pitch / 16, -1);
        for (size_t i = 0; i < bp.tap_list.size(); ++i) bp.tap_bins[i] = bp.tap_list[i].bin;
        if (!ar.put(bp.tap_bins, &pl.tap_bins) || !ar.put(bp.tap_list, &bp.d_tap_list) || !ar.put(group_bin0, &bp.d_group_bin0))
            return arena_full();
        // the matrix holds the slots from tap_first on and nothing else (every bin of a 1600-bin bank tapped, 2^25-sample
        // blocks: no matrix at all instead of 537 MB of it)
        const size_t mat_pitch = pitch - (size_t)pl.tap_first;
        const size_t need = mat_pitch * (size_t)pl.n_frames;
        const int rc = grow_buried(h, h->d_tapmat, h->tapmat_cap, need, need);
        if (rc != RCF_OK) return rc;
        pl.tap_mat = h->d_tapmat;
        pl.tap_pitch = (int32_t)mat_pitch;
        pl.n_taps = (int32_t)bp.tap_list.size();
    }
    // (a group's block: the exact-rotator fills and the tail stages of all members go out as one launch each)
    if (!bp.defer && !bp.rot_fills.empty() && !ar.put(bp.rot_fills, &bp.d_rot_fills)) return arena_full();
    if (!bp.defer && !bp.tails.upload(ar)) return arena_full();
    if (!bp.audf.empty() && !ar.put(bp.audf, &bp.d_audf)) return arena_full();
    return RCF_OK;
}

// plan_channel() advances a channel's state as it goes, so a block must not be refused half way through the schedule
// (the channels planned before the refusal would have counted outputs nobody computed).  The one refusal that depends on
// the block is a ring too small for what the block yields: this pass walks the channels in dependency order WITHOUT
// touching them -- what the block gives each one is kept in `dry`, where a channel chained on it finds its source range --
// and reports it first.  It only runs when the cheap bound in plan_block() says a ring could overflow.
int check_block_capacity(rcf_t *h, const BlockPlan &bp)
{
    std::unordered_map<int, Range> dry;            // channel id -> produced (before, after) this block
    const auto in_dry = [&dry](const Chan &sc) {
        auto it = dry.find(sc.id);
        return it == dry.end() ? Range{sc.pos.produced, sc.pos.produced} : it->second;
    };
    for (int depth = 0; depth <= bp.max_depth; ++depth)
        for (auto &kv : h->chans) {
            const Chan &c = *kv.second;
            if (c.depth != depth) continue;
            SrcRange sr{};
            if (!block_source(h, bp, c, in_dry, &sr)) continue;
            Share s;
            const int rc = block_share(h, bp, c, sr.p0, sr.p1, &s);
            if (rc != RCF_OK) return rc;
            dry[c.id] = {c.pos.produced, s.cnt ? s.n_lo + s.cnt : c.pos.produced};
        }
    return RCF_OK;
}

void undo_block(rcf_t *h, BlockUndo &u)
{
    if (!u.armed) return;
    for (const BlockUndo::Saved &s : u.saved) s.c->pos = s.pos;
    if (h->pfb.open) h->pfb.produced = h->pfb.produced_before;
    h->blk_serial = u.serial_before;
    u.armed = false;
}

// Everything of one block up to (not including) its launches.  On failure the handle is as it was before the call; on
// success the channels' counters have advanced and `undo` can still take that back (a group whose LATER member fails).
int plan_block(rcf_t *h, size_t n, BlockPlan &bp, BlockUndo &undo)
{
    bp.S0 = h->total_in;
    bp.S1 = bp.S0 + (int64_t)n;
    bp.n = n;
    auto tp = std::chrono::steady_clock::now();
    int rc = plan_arena(h, bp);
    if (rc == RCF_OK) rc = plan_pfb(h, bp);
    if (rc != RCF_OK) return rc;
    RCF_PROF(0, "plan_arena+pfb", tp);
    {
        // no ring can overflow when even the fastest channel's outputs of this block plus the longest reach fit
        size_t worst = bp.min_d0 ? n / (size_t)bp.min_d0 + 2 : 0;
        if (bp.run_pfb) worst = std::max(worst, (size_t)bp.pl.n_frames + 1);
        if (worst + bp.max_reach > h->out_cap && (rc = check_block_capacity(h, bp)) != RCF_OK) {
            if (h->pfb.open) h->pfb.produced = h->pfb.produced_before;      // plan_pfb had counted the block's frames
            return rc;
        }
    }
    // Planning advances every channel's counters and rotator model (plan_channel) and can still fail after that -- a
    // bank matrix, split-K slab or tap matrix that cannot be allocated, an exhausted launch arena.  Nothing has been
    // queued at that point: put the counters back, so that they never claim outputs nobody computed (and the exact
    // rotator's device state stays in step with them).
    // (every channel is saved right before plan_channel() touches it: one pass over the channels instead of two)
    undo.saved.clear();
    undo.saved.reserve(h->chans.size());
    undo.serial_before = h->blk_serial;
    undo.armed = true;
    auto roll_back = [&](int code) { undo_block(h, undo); return code; };
    // channels, by depth then by (D, T) class (the handle's PlanCache holds the buckets)
    bp.fir_by_depth.resize(bp.max_depth + 1);
    bp.serial = ++h->blk_serial;
    const auto &by_depth = h->plan_cache.by_depth;
    RCF_PROF(1, "undo + buckets", tp);
    for (int depth = 0; depth <= bp.max_depth; ++depth) {
        const auto &classes = by_depth[(size_t)depth];
        for (const auto &cls : classes) {
            ClassPlan cp;
            cp.launches.reserve(cls.second.size());
            cp.launched.reserve(cls.second.size());
            cp.discs.reserve(cls.second.size());
            const size_t nc = cls.second.size();
            for (size_t ci = 0; ci < nc; ++ci) {
                Chan *c = cls.second[ci];
                if (ci + 6 < nc) {                    // (a thousand front-ends' channels do not fit the host's caches)
                    const char *nx = reinterpret_cast<const char *>(cls.second[ci + 6]);
                    __builtin_prefetch(nx); __builtin_prefetch(nx + 64); __builtin_prefetch(nx + 128); __builtin_prefetch(nx + 192);
                }
                undo.saved.push_back(BlockUndo::Saved{c, c->pos});
                if ((rc = plan_channel(h, bp, cp, c)) != RCF_OK) return roll_back(rc);
            }
            RCF_PROF(3, "plan_channel (class)", tp);
            if ((rc = plan_class_jobs(h, bp, cp, depth, cls.first)) != RCF_OK) return roll_back(rc);
            RCF_PROF(4, "plan_class_jobs", tp);
        }
    }
    if ((rc = plan_tail(h, bp)) != RCF_OK) return roll_back(rc);
    RCF_PROF(5, "plan_tail", tp);
    {
        // RCF_FAIL_PLAN_AT=<k>: the k-th block of a handle fails here as an exhausted launch arena would (tests of the
        // roll-back above: tests/test_gpu_round4.py)
        static const long fail_at = [] { const char *e = getenv("RCF_FAIL_PLAN_AT"); return e ? atol(e) : 0L; }();
        if (fail_at > 0 && (long)++h->plan_calls == fail_at) {
            set_error("injected planning failure (RCF_FAIL_PLAN_AT)");
            return roll_back(RCF_ENOMEM);
        }
    }
    return RCF_OK;
}

int process_block(rcf_t *h, size_t n)
{
    if (h->graveyard.size() > 512) drain_graveyard(h);     // bounded even if nobody ever syncs or reads
    BlockPlan bp;
    BlockUndo undo;
    int rc = plan_block(h, n, bp, undo);
    if (rc != RCF_OK) return rc;
    if ((rc = launch_plan(h, bp)) != RCF_OK) return rc;      // kernels may be queued: the handle's stream state is undefined now
    if ((rc = run_scan(h, bp)) != RCF_OK) return rc;
    return finish_block(h, bp);
}

}  // namespace rcfx
