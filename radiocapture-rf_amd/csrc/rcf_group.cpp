// rcf_group.cpp -- grouped launches over front-ends, and the native real-time pump that drives them.
//
// The reference's receiver holds every configured SDR source in one top block (rc_frontend/receiver.py:67-70,170-204;
// ten sources per host in configs/config_denver_dev_den817.py:25-118).  Here a source is an rcf_t with its own buffers
// and channels; run one by one, a real-time block (20 ms of 20 Msps) is a handful of ~5 us kernels per front-end and one
// MI355X is LAUNCH-bound at a few hundred of them while its memory system idles.  A group plans the blocks of G
// front-ends with the per-front-end planner (rcf_plan.cpp, unchanged arithmetic), concatenates what is concatenable and
// launches ONE kernel per stage:
//   group_prep_kernel          wire format -> cf32 for every member (pinned host memory read in place), history tails
//                              dual-written, the group's launch records host -> device        (ingest.hip)
//   pfb_group_kernel_* / pfb5_group_kernel / pfbm_group_kernel   the chunks of every member of one bank shape   (pfb.hip, pfb5.hip, pfbm.hip)
//   fir_small_kernel / fir_bank_kernel       stage-2 channels of all members of one (D, T) class (records concatenated)
//   tap_finalize_group_kernel  the tapped bins of every member                               (tapfin.hip)
//   disc / rot_fill, and the tail stages (TailStages, rcf_plan.h: fm_fir / agc / clock_mm / costas / fsk4 / slice / tsbk / edacs / osw / p25lc / squelch / capture)   records
//                              concatenated: the group's table is the members' tables appended
//   gather_rings_kernel        the read: new output of any channels of any members -> pinned host memory, one launch
// What is not concatenable (matrix-core banks with their per-handle tap slabs, voice chains, scans, banks that still see
// zero history) follows per member on the same stream, in dependency order.  The bits are those of the members run alone.
#include <tuple>

#include "rcf_group.h"

using namespace rcfx;


namespace {

using ShapeKey = std::tuple<int, int, int, int>;

struct MergedFir {
    FirLaunchDims dims{};
    std::vector<ChanLaunch> recs;
    const ChanLaunch *dev = nullptr;
};

// filterbanks of one shape in steady state: one launch where the shape has a grouped kernel (pfb_shape.h), one by one at the
// bucket's place where it has none
struct BankGroup { std::vector<size_t> idx; const PfbLaunch *d_pls = nullptr; GroupMap gm{}; bool grouped = false; };

// One group block on its way through the stages below, in the order group_process() calls them.
struct GroupBlock {
    rcf_group *g;
    const std::vector<GroupItem> &items;
    int fmt; float scale, offset;
    hipStream_t st;
    rcf_t *h0;                                 // merged launches are timed on the first member (rcf_timing_* of that handle)
    int a = 0;                                 // the group's arena in use, where this block's records start in it ...
    size_t base = 0;
    Arena ga{nullptr, nullptr, 0, 0};          // ... and the members' planners and the merge stages put them
    std::vector<const void *> dsrc;            // per item: its source as the device reads it (nullptr: resident)
    std::vector<std::unique_ptr<BlockPlan>> plans;
    std::vector<BlockUndo> undo;
    std::map<ShapeKey, BankGroup> banks;       // (bins, decimation, rows of the kernel, fused-discriminator mode)
    std::vector<size_t> bank_singles;
    std::vector<TapFinArgs> tap_args;
    const TapFinArgs *d_tap_args = nullptr;
    int tap_max_taps = 0, tap_max_rows = 0;
    std::vector<std::map<ShapeKey, MergedFir>> merged;   // per depth: (D, T, small, KT) -> the members' records of that class
    DiscJob disc;                              // the members' discriminator, tail-stage and rotator-fill records
    TailStages tails;
    std::vector<RotFill> rots;
    const RotFill *d_rots = nullptr;
    std::vector<PrepRec> prep;                 // the ingest launch's records, kPrepMaxRecs per launch
    std::vector<uint32_t> prep_tiles;
    const PrepRec *prep_mapped = nullptr;

    size_t size() const { return items.size(); }
    rcf_t *member(size_t i) const { return g->members[(size_t)items[i].m]; }
};

// room in the group's arena for every member's records and the group's own
int reserve_arena(GroupBlock &b)
{
    size_t need = 16384 + b.size() * (3 * sizeof(PrepRec) + sizeof(PfbLaunch) + sizeof(TapFinArgs) + 4 * sizeof(int32_t) + 512);
    for (size_t i = 0; i < b.size(); ++i) {
        rcf_t *h = b.member(i);
        flush_lagged(h);                                       // (a member that was fed on its own before: nothing lags inside a group)
        if (h->graveyard.size() > 512) drain_graveyard(h);
        need += arena_need_bound(h);
    }
    ArenaSet &as = b.g->arenas;
    if (as.reserve(need, b.st) != RCF_OK) return RCF_EHIP;
    b.a = as.cur;
    b.base = as.fill;
    b.ga = Arena{as.h[b.a], as.d[b.a], b.base, as.cap};
    return RCF_OK;
}

// where the device reads each source: pinned memory in place, pageable memory through a staging copy
int stage_sources(GroupBlock &b)
{
    const size_t bps = group_sample_bytes(b.fmt);
    b.dsrc.assign(b.size(), nullptr);
    for (size_t i = 0; i < b.size(); ++i) {
        const GroupItem &it = b.items[i];
        if (!it.src) continue;
        if (it.dsrc) { b.dsrc[i] = it.dsrc; continue; }
        void *dv = nullptr;
        if (hipHostGetDevicePointer(&dv, const_cast<void *>(it.src), 0) == hipSuccess && dv) { b.dsrc[i] = dv; continue; }
        (void)hipGetLastError();                               // (pageable memory: not an error)
        const size_t bytes = it.n * bps;
        void *&stage = b.g->d_stage[(size_t)it.m];
        if (b.g->stage_cap[(size_t)it.m] < bytes) {
            void *nd = nullptr;
            RCF_HIP(hipMalloc(&nd, bytes));
            if (stage) { RCF_HIP(hipStreamSynchronize(b.st)); (void)hipFree(stage); }
            stage = nd;
            b.g->stage_cap[(size_t)it.m] = bytes;
        }
        RCF_HIP(hipMemcpyAsync(stage, it.src, bytes, hipMemcpyHostToDevice, b.st));
        b.dsrc[i] = stage;
    }
    return RCF_OK;
}

// every member's block planned by the per-front-end planner into the group's arena.  (A refusal leaves the refused member as
// it was; group_process takes back the ones planned before it.)
int plan_members(GroupBlock &b)
{
    b.plans.resize(b.size());
    b.undo.resize(b.size());
    for (size_t i = 0; i < b.size(); ++i) {
        b.plans[i].reset(new BlockPlan);
        b.plans[i]->defer = true;
        b.plans[i]->ar = &b.ga;
        const int rc = plan_block(b.member(i), b.items[i].n, *b.plans[i], b.undo[i]);
        if (rc != RCF_OK) return rc;
    }
    return RCF_OK;
}

// filterbanks: members of one shape in steady state share a bucket; a bucket of one, and every bank that cannot join one,
// goes out alone after the buckets
int merge_banks(GroupBlock &b)
{
    for (size_t i = 0; i < b.size(); ++i) {
        BlockPlan &bp = *b.plans[i];
        if (!bp.run_pfb) continue;
        bp.pl.ev_start = bp.pl.ev_stop = nullptr;
        // (the grouped kernels have no masking form: plan_pfb's answer -- for a fused bank it covers the chunk before its
        // first frame, which its first workgroup recomputes; and such a bank joins in its look-back form only)
        if (bp.pfb_zero_history || (bp.pl.fm_ring && !bp.pl.fm_edge)) {
            b.bank_singles.push_back(i);
            continue;
        }
        const PfbShape &sh = bp.shape;
        BankGroup &bg = b.banks[std::make_tuple(sh.NB, sh.D, sh.Ppad, bp.pl.fm_ring ? bp.pl.fm_mode : 0)];
        bg.grouped = bp.pl.fm_ring ? sh.grouped_fused : sh.grouped;
        bg.idx.push_back(i);
    }
    for (auto it = b.banks.begin(); it != b.banks.end();) {
        BankGroup &bg = it->second;
        if (bg.idx.size() < 2) { b.bank_singles.push_back(bg.idx[0]); it = b.banks.erase(it); continue; }
        if (!bg.grouped) { ++it; continue; }
        const int F = b.plans[bg.idx[0]]->shape.chunk_frames;
        std::vector<PfbLaunch> pls;
        std::vector<int32_t> first;
        pls.reserve(bg.idx.size());
        first.reserve(bg.idx.size() + 1);
        int32_t total = 0, uniform = -1;
        for (size_t i : bg.idx) {
            const PfbLaunch &pl = b.plans[i]->pl;
            const int32_t nwg = (pl.n_frames + F - 1) / F;
            uniform = uniform < 0 ? nwg : (uniform == nwg ? uniform : 0);
            first.push_back(total);
            total += nwg;
            pls.push_back(pl);
        }
        first.push_back(total);
        if (!b.ga.put(pls, &bg.d_pls) || !b.ga.put(first, &bg.gm.wg_first)) return arena_full();
        bg.gm.n_fe = (int32_t)bg.idx.size();
        bg.gm.total_wg = total;
        bg.gm.uniform_nwg = uniform > 0 ? uniform : 0;
        ++it;
    }
    std::sort(b.bank_singles.begin(), b.bank_singles.end());
    return RCF_OK;
}

// the tapped bins of every member: one tap-finalize launch
int merge_taps(GroupBlock &b)
{
    for (auto &p : b.plans) {
        const BlockPlan &bp = *p;
        if (!bp.run_pfb || bp.pl.n_taps <= 0) continue;
        const PfbLaunch &pl = bp.pl;
        b.tap_args.push_back(TapFinArgs{bp.d_tap_list, pl.tap_mat, bp.d_group_bin0, pl.bins_ring, pl.n_lo - pl.n_abs0, pl.n_taps,
                                        pl.tap_pitch, pl.n_frames, pl.tap_first, pl.NB, 0});
        b.tap_max_taps = std::max(b.tap_max_taps, (int)pl.n_taps);
        b.tap_max_rows = std::max(b.tap_max_rows, (int)pl.n_frames);
    }
    if (!b.tap_args.empty() && !b.ga.put(b.tap_args, &b.d_tap_args)) return arena_full();
    return RCF_OK;
}

// FIR jobs whose records are self-contained: one launch per depth and (D, T) class
int merge_firs(GroupBlock &b)
{
    size_t depths = 1;
    for (auto &bp : b.plans) depths = std::max(depths, bp->fir_by_depth.size());
    b.merged.resize(depths);
    for (auto &bp : b.plans)
        for (size_t d = 0; d < bp->fir_by_depth.size(); ++d)
            for (FirJob &j : bp->fir_by_depth[d]) {
                if (j.host.empty()) continue;
                MergedFir &mf = b.merged[d][std::make_tuple(j.dims.D, j.dims.T, j.dims.small, j.dims.KT)];
                if (mf.recs.empty()) { mf.dims = j.dims; mf.dims.max_n_k = 0; mf.dims.atan_tab = b.h0->d_atan; }
                mf.dims.max_n_k = std::max(mf.dims.max_n_k, j.dims.max_n_k);
                mf.recs.insert(mf.recs.end(), j.host.begin(), j.host.end());
            }
    for (auto &lvl : b.merged)
        for (auto &kv : lvl) {
            kv.second.dims.n_chans = (int)kv.second.recs.size();
            if (!b.ga.put(kv.second.recs, &kv.second.dev)) return arena_full();
        }
    return RCF_OK;
}

// discriminators, tail stages (TailStages, rcf_plan.h), exact-rotator fills: the members' records one after the other
int merge_tails(GroupBlock &b)
{
    for (auto &bp : b.plans) {
        for (const DiscJob &dj : bp->disc_jobs) b.disc.append(dj);
        b.tails.append(bp->tails);
        b.rots.insert(b.rots.end(), bp->rot_fills.begin(), bp->rot_fills.end());
    }
    if (!b.disc.upload(b.ga) || !b.tails.upload(b.ga) || (!b.rots.empty() && !b.ga.put(b.rots, &b.d_rots))) return arena_full();
    return RCF_OK;
}

void push_copy_rec(GroupBlock &b, const void *src, float2 *dst, size_t n8)
{
    PrepRec c{};
    c.src = src;
    c.dst = dst;
    c.n = (uint32_t)n8;
    c.fmt = -1;
    b.prep.push_back(c);
}

// The ingest launch's records, last: per member its conversion and the history of its next block, then the one that uploads
// everything put into the arena so far.  Block sample k sits at buffer index H + k; the next block's history is buffer
// [n, n + H): sample k lands at other[H + k - n] once that is >= 0.
int build_prep(GroupBlock &b)
{
    const size_t bps = group_sample_bytes(b.fmt);
    b.prep.reserve(2 * b.size() + 1);
    for (size_t i = 0; i < b.size(); ++i) {
        rcf_t *h = b.member(i);
        const size_t n = b.items[i].n, H = h->hist_cap;
        float2 *curb = h->d_buf[h->cur], *oth = h->d_buf[h->cur ^ 1];
        if (b.dsrc[i]) {
            PrepRec r{};
            r.src = b.dsrc[i];
            r.dst = curb + H;
            r.n = (uint32_t)n;
            r.hist_from = n >= H ? (uint32_t)(n - H) : 0u;
            r.hist_dst = n >= H ? oth : oth + (H - n);
            r.fmt = b.fmt;
            r.scale = b.scale;
            r.offset = b.offset;
            const size_t item = b.fmt == RCF_FMT_CF32 ? 4 : bps / 2;    // bytes per raw value
            r.aligned = ((uintptr_t)r.src % (4 * item)) == 0 ? 1 : 0;
            r.dst_aligned = ((uintptr_t)r.dst % 16) == 0 ? 1 : 0;
            b.prep.push_back(r);
            if (n < H) push_copy_rec(b, curb + n, oth, H - n);          // the part of the history that is older than this block
        } else {
            push_copy_rec(b, curb + n, oth, H);                         // resident data: only the history moves
        }
        b.plans[i]->history_done = true;
    }
    unsigned char *h_dev = b.g->arenas.h_dev[b.a];                      // the pinned arena as the device sees it
    const UploadSpan up = arena_upload_span(b.base, b.ga.used);
    if (up.bytes) push_copy_rec(b, h_dev + up.from, reinterpret_cast<float2 *>(b.ga.d + up.from), up.bytes / 8);
    for (size_t at = 0; at < b.prep.size(); at += kPrepMaxRecs)
        b.prep_tiles.push_back(fill_prep_tiles(b.prep.data() + at, (int)std::min<size_t>(kPrepMaxRecs, b.prep.size() - at)));
    const PrepRec *d_prep = nullptr;
    if (!b.ga.put(b.prep, &d_prep)) return arena_full();
    // (the kernel reads ITS records where the host wrote them, not their device copy)
    b.prep_mapped = reinterpret_cast<const PrepRec *>(h_dev + (reinterpret_cast<const unsigned char *>(d_prep) - b.ga.d));
    b.g->arenas.fill = (b.ga.used + 63) & ~size_t(63);
    return RCF_OK;
}

void launch_prep(const GroupBlock &b)
{
    for (size_t at = 0, li = 0; at < b.prep.size(); at += kPrepMaxRecs, ++li)
        launch_group_prep(b.prep_mapped + at, (int)std::min<size_t>(kPrepMaxRecs, b.prep.size() - at), b.prep_tiles[li], b.st);
}

// one depth of FIRs: every member's own jobs, then the merged classes
void launch_fir_depth(GroupBlock &b, size_t d)
{
    for (size_t i = 0; i < b.size(); ++i) {
        BlockPlan &bp = *b.plans[i];
        if (d >= bp.fir_by_depth.size()) continue;
        for (FirJob &j : bp.fir_by_depth[d])
            if (j.host.empty())                                         // (the others were merged)
                launch_fir_job(b.member(i), j, d ? RCF_T_FIR_DERIVED : (j.dims.mfma ? RCF_T_FIR_MFMA : RCF_T_FIR), b.st);
    }
    for (auto &kv : b.merged[d]) {
        Timed t(b.h0, d ? RCF_T_FIR_DERIVED : RCF_T_FIR);
        launch_fir_bank(kv.second.dev, kv.second.dims, b.st);
    }
}

void launch_banks_alone(GroupBlock &b, const std::vector<size_t> &idx)
{
    for (size_t i : idx) {
        Timed t(b.member(i), RCF_T_PFB);
        launch_pfb(b.plans[i]->shape, b.plans[i]->pl, b.plans[i]->pfb_zero_history, b.st);
    }
}

// Everything behind the prep launch, in dependency order (launch_plan's, rcf_launch.cpp).  The first error is returned, and
// the launching goes on: finish_members has every member's bookkeeping to do either way.
int launch_block(GroupBlock &b, bool wait)
{
    rcf_t *h0 = b.h0;
    hipStream_t st = b.st;
    int rc = RCF_OK;
    if (wait && hipEventRecord(b.g->ingest_ev, st) != hipSuccess) { set_error("group: event record failed"); rc = RCF_EHIP; }
    if (b.d_rots) launch_rot_fill(b.d_rots, (int)b.rots.size(), h0->ring_mask, st);
    launch_fir_depth(b, 0);
    for (auto &kv : b.banks) {
        BankGroup &bg = kv.second;
        const BlockPlan &b0 = *b.plans[bg.idx[0]];
        if (bg.grouped) { Timed t(h0, RCF_T_PFB); launch_pfb_group(b0.shape, b0.pl, bg.d_pls, bg.gm, st); }
        else launch_banks_alone(b, bg.idx);
    }
    launch_banks_alone(b, b.bank_singles);
    for (size_t i = 0; i < b.size(); ++i) launch_member_pfb_squelch(b.member(i), *b.plans[i], st);
    if (b.d_tap_args) {
        Timed t(h0, RCF_T_TAPS);
        launch_tap_finalize_group(b.d_tap_args, (int)b.tap_args.size(), b.tap_max_taps, b.tap_max_rows, h0->ring_mask, h0->d_atan, st);
    }
    for (size_t d = 1; d < b.merged.size(); ++d) launch_fir_depth(b, d);
    launch_tail(h0, &b.disc, b.disc.dev ? 1 : 0, b.tails, st);
    for (size_t i = 0; i < b.size(); ++i) {
        launch_member_audio(b.member(i), *b.plans[i], st);
        const int rs = run_scan(b.member(i), *b.plans[i]);
        if (rs != RCF_OK && rc == RCF_OK) rc = rs;
    }
    if (rc == RCF_OK) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_error("group launch failed: %s", hipGetErrorString(e)); rc = RCF_EHIP; }
    }
    return rc;
}

// Every member's buffers flip and its counters advance: the prep kernel has written them whatever came of the launches
// after it, and after an error among those every member is faulted.  Not finish_block (rcf_launch.cpp): the history went
// out with the prep launch, and a member of a group records no buf_done event -- rcf_push_iq on it later orders its copy
// behind these reads through buf_dirty.
int finish_members(GroupBlock &b, int rc)
{
    for (size_t i = 0; i < b.size(); ++i) {
        rcf_t *h = b.member(i);
        h->buf_dirty[h->cur] = true;
        h->cur ^= 1;
        h->total_in = b.plans[i]->S1;
        if (rc == RCF_OK) continue;
        h->fault = rc;
        std::snprintf(h->fault_text, sizeof h->fault_text, "group block failed: %s", rcf_last_error());
    }
    return rc;
}

}  // namespace

// (declared in rcf_group.h: the pump calls it)
int rcfx::group_process(rcf_group *g, const std::vector<GroupItem> &items, int fmt, float scale, float offset, bool wait)
{
    if (items.empty()) return RCF_OK;
    auto tp = std::chrono::steady_clock::now();
    RCF_HIP(hipSetDevice(g->device));
    GroupBlock b{g, items, fmt, scale, offset, g->stream, g->members[0]};

    // Until the prep launch nothing is queued: a stage that fails returns its code, and what the planning advanced in the
    // members is taken back here, once.
    int rc = reserve_arena(b);
    if (rc == RCF_OK) { RCF_PROF(8, "group: arena reserve", tp); rc = stage_sources(b); }
    if (rc == RCF_OK) rc = plan_members(b);
    if (rc == RCF_OK) { RCF_PROF(9, "group: planning (all)", tp); rc = merge_banks(b); }
    if (rc == RCF_OK) rc = merge_taps(b);
    if (rc == RCF_OK) rc = merge_firs(b);
    if (rc == RCF_OK) rc = merge_tails(b);
    if (rc == RCF_OK) rc = build_prep(b);
    if (rc != RCF_OK) {
        for (size_t i = 0; i < b.undo.size(); ++i) undo_block(b.member(i), b.undo[i]);
        return rc;
    }
    RCF_PROF(10, "group: merging + records", tp);

    // From the prep launch on every listed member's counters have been advanced and its buffers written, and a failure
    // leaves queued work behind: no roll-back.  Errors are collected, every member is finished and -- after an error -- faulted.
    launch_prep(b);
    RCF_PROF(11, "group: prep launch", tp);
    rc = finish_members(b, launch_block(b, wait));
    if (rc != RCF_OK) return rc;
    RCF_PROF(12, "group: other launches", tp);
    if (wait) (void)hipEventSynchronize(g->ingest_ev);
    return RCF_OK;
}

// =================================================================== C ABI
extern "C" {

int rcf_group_open(rcf_t *const *handles, int n, rcf_group_t **out)
{
    if (!handles || n < 1 || !out) { set_error("bad group arguments"); return RCF_EINVAL; }
    for (int i = 0; i < n; ++i) {
        if (!handles[i]) { set_error("group member %d is NULL", i); return RCF_EINVAL; }
        for (int j = 0; j < i; ++j)
            if (handles[j] == handles[i]) { set_error("group member %d listed twice", i); return RCF_EINVAL; }
        if (handles[i]->device != handles[0]->device || handles[i]->out_cap != handles[0]->out_cap) {
            set_error("group members must share the device and the output capacity (member %d differs)", i);
            return RCF_EINVAL;
        }
        if (handles[i]->group) { set_error("group member %d already belongs to a group", i); return RCF_ESTATE; }
    }
    std::unique_ptr<rcf_group> g(new rcf_group);
    g->device = handles[0]->device;
    RCF_HIP(hipSetDevice(g->device));
    g->members.assign(handles, handles + n);
    g->d_stage.assign((size_t)n, nullptr);
    g->stage_cap.assign((size_t)n, 0);
    // everything that can fail comes first and touches no member's state: a failure below leaves the handles as they were
    // (no dangling group / stream pointers on them, rcf_close still works), the stream and the event are destroyed
    MemberLocks ml(g->members);
    for (rcf_t *h : g->members)
        if (h->group) { set_error("a group member already belongs to a group"); return RCF_ESTATE; }   // (checked again under its lock)
    int rc = RCF_OK;
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) rc = RCF_EHIP;
    if (rc == RCF_OK && hipEventCreateWithFlags(&g->ingest_ev, hipEventDisableTiming) != hipSuccess) rc = RCF_EHIP;
    for (rcf_t *h : g->members) {
        if (rc != RCF_OK) break;
        flush_lagged(h);
        if (hipStreamSynchronize(h->stream) != hipSuccess) rc = RCF_EHIP;   // whatever it queued on its own stream comes first
    }
    if (rc != RCF_OK) {
        set_error("group open: %s", hipGetErrorString(hipGetLastError()));
        if (g->ingest_ev) (void)hipEventDestroy(g->ingest_ev);
        if (g->stream) (void)hipStreamDestroy(g->stream);
        return rc;
    }
    for (rcf_t *h : g->members) {                          // (cannot fail)
        time_collect(h);
        h->own_stream = h->stream;
        h->stream = g->stream;
        h->group = g.get();
    }
    *out = g.release();
    return RCF_OK;
}

int rcf_group_close(rcf_group_t *g)
{
    if (!g) return RCF_EINVAL;
    if (g->pump) { set_error("stop the group's pump first"); return RCF_ESTATE; }
    (void)hipSetDevice(g->device);
    {
        std::lock_guard<std::mutex> gl(g->mu);
        MemberLocks ml(g->members);
        (void)hipStreamSynchronize(g->stream);
        for (rcf_t *h : g->members) {
            time_collect(h);
            free_graveyard_idle(h);
            h->stream = h->own_stream;
            h->own_stream = nullptr;
            h->group = nullptr;
        }
    }
    for (void *p : g->d_stage) if (p) (void)hipFree(p);
    g->host_stage.release();
    g->arenas.destroy();
    if (g->ingest_ev) (void)hipEventDestroy(g->ingest_ev);
    (void)hipStreamDestroy(g->stream);
    delete g;
    return RCF_OK;
}

int rcf_group_size(rcf_group_t *g) { return g ? (int)g->members.size() : RCF_EINVAL; }

static int group_call(rcf_group_t *g, const void *const *blocks, const size_t *n_samples, int fmt, float scale, float offset,
                      bool commit)
{
    if (!g || !n_samples || (!commit && !blocks)) { set_error("bad group push arguments"); return RCF_EINVAL; }
    if (!commit && group_sample_bytes(fmt) == 0) { set_error("unknown sample format %d", fmt); return RCF_EINVAL; }
    std::vector<GroupItem> items;
    for (size_t i = 0; i < g->members.size(); ++i) {
        const size_t n = n_samples[i];
        if (n == 0 || (!commit && !blocks[i])) continue;
        if (n > g->members[i]->block_cap) {
            set_error("member %zu: %zu samples exceed its block capacity %zu", i, n, g->members[i]->block_cap);
            return RCF_ECAP;
        }
        items.push_back(GroupItem{(int)i, n, commit ? nullptr : blocks[i], nullptr});
    }
    std::lock_guard<std::mutex> gl(g->mu);
    if (g->pump) { set_error("the group is fed by its pump"); return RCF_ESTATE; }
    MemberLocks ml(g->members);
    return group_process(g, items, fmt, scale, offset, !commit);
}

int rcf_group_push(rcf_group_t *g, const void *const *blocks, const size_t *n_samples, int fmt, float scale, float offset)
{
    return group_call(g, blocks, n_samples, fmt, scale, offset, false);
}

int rcf_group_commit(rcf_group_t *g, const size_t *n_samples)
{
    return group_call(g, nullptr, n_samples, RCF_FMT_CF32, 1.0f, 0.0f, true);
}

int rcf_group_sync(rcf_group_t *g)
{
    if (!g) return RCF_EINVAL;
    std::lock_guard<std::mutex> gl(g->mu);
    MemberLocks ml(g->members);
    RCF_HIP(hipSetDevice(g->device));
    for (rcf_t *h : g->members) flush_lagged(h);
    RCF_HIP(hipStreamSynchronize(g->stream));
    for (rcf_t *h : g->members) free_graveyard_idle(h);
    return RCF_OK;
}

int rcf_group_read_many(rcf_group_t *g, int what, const int *members, const int *chan_ids, int n, float gain, void *out,
                        size_t cap_each, int64_t *counts)
{
    if (!g || !members || !chan_ids || !out || !counts || n < 0 || row_kind(what) < 0) {
        set_error("bad batched read arguments");
        return RCF_EINVAL;
    }
    std::lock_guard<std::mutex> gl(g->mu);
    MemberLocks ml(g->members);
    RCF_HIP(hipSetDevice(g->device));
    for (rcf_t *h : g->members) flush_lagged(h);            // (a member that was fed on its own meanwhile)
    return read_many(g->host_stage, g->stream, g->members.data(), g->members.size(), members, chan_ids, n, what, gain, out, cap_each,
                     counts);
}

}  // extern "C"
