// rcf_plan.h -- the per-block schedule: what one commit of one front-end launches, built on the host first.  The stages
// behind the FIRs (symbol filters, AGCs, the three symbol loops, the slicers behind the loops, the TSBK, EDACS, OSW and P25 voice stages behind the slicers, the carrier detectors, the capture stages) are one table, TailStages: a block's plan and a group's
// block each hold one, and the planner, the group's merge and the launcher visit it through TailStages::each.
#pragma once
#include <chrono>

#include "rcf_state.h"

namespace rcfx {

struct Arena {
    unsigned char *h, *d;
    size_t used = 0, cap;
    template <class T>
    bool put(const std::vector<T> &v, const T **dev)
    {
        const size_t bytes = sizeof(T) * v.size();
        const size_t at = (used + 63) & ~size_t(63);
        if (at + bytes > cap) return false;
        std::memcpy(h + at, v.data(), bytes);
        *dev = reinterpret_cast<const T *>(d + at);
        used = at + bytes;
        return true;
    }
};
inline int arena_full() { set_error("launch arena exhausted"); return RCF_ENOMEM; }     // what a failed put() comes to

// A device buffer of the handle that has to hold `need` items: when it does not, one of `want` (>= need) is allocated in
// its place and the old one buried -- launches queued earlier may still read it.
template <class T> int grow_buried(rcf_t *h, T *&d, size_t &cap, size_t need, size_t want)
{
    if (need <= cap) return RCF_OK;
    T *nd = nullptr;
    RCF_HIP(hipMalloc(&nd, sizeof(T) * want));
    bury(h, d);
    d = nd;
    cap = want;
    return RCF_OK;
}

inline int choose_kt(int D, int T)
{
    int kt = (8192 - T) / D + 1;
    if (kt < 1) kt = 1;
    if (kt > 256) kt = 256;
    if (kt >= 8) kt &= ~7;
    return kt;
}

// ------------------------------------------------------------------ the per-block schedule
// Everything one commit schedules is built on the host first (a BlockPlan: launch records in the pinned arena, jobs per
// dependency depth), then uploaded with one copy and launched in dependency order.  process_block() is the sequence;
// the plan_*() functions below each build one part of it.
struct FirJob {
    FirLaunchDims dims; const ChanLaunch *dev; bool repack; const unsigned char *dirty;
    // bank-matrix cache entry to mark current once the pack launch has been queued (not before: an error
    // return in between must not leave a key that claims a matrix nobody built)
    rcf::BankCache *bc; std::vector<std::pair<int, uint64_t>> key;
    std::vector<ChanLaunch> host;      // BlockPlan::defer: records not yet in the arena (the group merges them first)
    bool bank_src = false;             // every channel of the job reads a bin of the filterbank (what the stage-2 lag may defer)
};

// The records of one stage in one block, all channels (a group's block: of all members) in one launch: on the host, and in
// the arena once uploaded (BlockPlan::defer: the group uploads what it merged)
template <class Rec> struct StageRecs {
    std::vector<Rec> host;
    const Rec *dev = nullptr;
    int max_n = 0;                     // the largest n_k
    int n() const { return (int)host.size(); }
    void add(const Rec &r) { host.push_back(r); max_n = std::max(max_n, (int)r.n_k); }
    void append(const StageRecs &o) { host.insert(host.end(), o.host.begin(), o.host.end()); max_n = std::max(max_n, o.max_n); }
    bool upload(Arena &ar) { return host.empty() || ar.put(host, &dev); }
};
typedef StageRecs<DiscLaunch> DiscJob;     // the discriminators of one (depth, D, T) class
struct AgcRecs : StageRecs<AgcLaunch> {
    int max_ns = 0;                    // the longest window
    void add(const AgcLaunch &r) { StageRecs::add(r); max_ns = std::max(max_ns, (int)r.nsamples); }
    void append(const AgcRecs &o) { StageRecs::append(o); max_ns = std::max(max_ns, o.max_ns); }
};

// The stages that follow the derived FIRs and the discriminators, in launch order.  each() is the one list of them: it
// calls f(timing class, launcher, the stage of every table given).  kNoTimingClass: the stage's launch is not timed
// (RCF_T_COUNT is the ABI's).
constexpr int kNoTimingClass = -1;
struct TailStages {
    StageRecs<FmFirLaunch> symf;       // symbol filters: they read the rings the discriminators wrote
    AgcRecs agcf;                      // feedforward AGCs
    StageRecs<ClockLaunch> clkf;       // symbol clocks, behind the discriminators
    StageRecs<CostasLaunch> gcf;       // Gardner / Costas loops, behind the AGCs: they read the AGC rings
    StageRecs<Fsk4Launch> f4f;         // C4FM loops, behind the symbol filters: they read the symbol-filter rings
    StageRecs<SliceLaunch> slf;        // slicers, behind the three loops: they read the loops' soft-symbol rings and counters
    StageRecs<TsbkLaunch> tsf;         // P25 trunking blocks, behind the slicers: they read the slicers' rings and counters
    StageRecs<EdacsLaunch> edf;        // EDACS control frames, behind the slicers likewise
    StageRecs<OswLaunch> osf;          // SmartNet OSWs, behind the slicers likewise
    StageRecs<P25lcLaunch> lcf;        // P25 voice data units, behind the slicers likewise
    StageRecs<SquelchLaunch> sqf;      // carrier detect: it reads the IQ rings the FIRs and the tap finalize wrote
    StageRecs<CaptureLaunch> capf;     // carrier-operated capture: it reads the same rings, this block's samples and `pre` before them
    template <class F, class... T> static void each(F &&f, T &...t)
    {
        f(RCF_T_DISC, launch_fm_fir, t.symf...);
        f(RCF_T_DISC, launch_agc, t.agcf...);
        f(RCF_T_CLOCK, launch_clock_mm, t.clkf...);
        f(RCF_T_COSTAS, launch_costas, t.gcf...);
        f(RCF_T_FSK4, launch_fsk4, t.f4f...);
        f(RCF_T_SLICE, launch_slice, t.slf...);
        f(RCF_T_SLICE, launch_tsbk, t.tsf...);
        f(RCF_T_SLICE, launch_edacs, t.edf...);
        f(RCF_T_SLICE, launch_osw, t.osf...);
        f(RCF_T_SLICE, launch_p25lc, t.lcf...);
        f(kNoTimingClass, launch_squelch, t.sqf...);
        f(kNoTimingClass, launch_capture, t.capf...);
    }
    template <class Rec> StageRecs<Rec> &of()      // the stage whose records are plain StageRecs<Rec>: found at compile time
    {
        StageRecs<Rec> *r = nullptr;
        each([&r](int, auto, auto &s) { if constexpr (std::is_same<StageRecs<Rec> &, decltype(s)>::value) r = &s; }, *this);
        return *r;
    }
    void append(const TailStages &o) { each([](int, auto, auto &mine, const auto &theirs) { mine.append(theirs); }, *this, o); }
    bool upload(Arena &ar)
    {
        bool ok = true;
        each([&](int, auto, auto &s) { ok = ok && s.upload(ar); }, *this);
        return ok;
    }
    bool any() const                   // a record of any stage in this block
    {
        bool v = false;
        each([&](int, auto, const auto &s) { v = v || !s.host.empty(); }, *this);
        return v;
    }
};

struct BlockPlan {
    int64_t S0 = 0, S1 = 0;            // the block's samples [S0, S1)
    size_t n = 0;

    // how far back every consumer of a ring reaches beyond the block's new samples (a block's writes must not
    // overwrite what the same block's readers still need): derived channels T - 1 + D of source output, the
    // discriminator one sample, the symbol filter its taps, the AGC N - 1 IQ samples, the symbol clock 7 of the
    // discriminator's (the Gardner / Costas loop and the C4FM loop none: their history is in their state records).  Every ring reaches back 1 (the discriminator); only sources of other channels and channels with a
    // symbol filter, an AGC or a symbol clock reach further -- the
    // map holds just those (with 131072 plain wideband channels it stays empty: a std::map entry per channel and block
    // was a tenth of the host's schedule time).
    const std::unordered_map<int, size_t> *reach_x = nullptr;   // source id (channel id / RCF_SRC_PFB_BIN0) -> samples (the handle's PlanCache)
    int max_depth = 0;
    int min_d0 = 0;                    // smallest decimation among the channels on the wideband stream (0: none)
    size_t max_reach = 1;              // largest consumer reach of any ring (see reach_x) / voice-chain filter
    size_t arena_need = 0;
    int a = 0;                         // arena in use, and where this commit's records start in it
    size_t arena_base = 0;
    Arena own_ar{nullptr, nullptr, 0, 0};
    Arena *ar = &own_ar;               // a member of a group plans into the group's arena instead
    uint64_t serial = 0;               // Chan::Pos::blk_before / blk_after of this block carry it
    std::vector<std::vector<FirJob>> fir_by_depth;
    std::vector<DiscJob> disc_jobs;
    TailStages tails;                  // symbol filters, AGCs, symbol loops: all channels of a stage in one launch
    std::vector<RotFill> rot_fills;    // exact rotator: one record per launched channel, one launch before the FIRs
    std::vector<TapLaunch> tap_list;   // filterbank taps: copied out by the bank's kernel, finished by tap_finalize
    std::vector<int32_t> tap_bins;
    std::vector<AudioLaunch> audf;     // analog voice chains, all channels in one set of launches
    int audf_max_n = 0;
    double audf_ratio = 0;
    int audf_num = 1, audf_den = 1;
    PfbLaunch pl{};
    bool run_pfb = false;
    bool run_pfb_squelch = false;      // the bank carries the carrier detector (rcf_pfb_squelch): two launches behind the bank's
    PfbShape shape;                    // run_pfb: the bank's shape, and whether this launch still reaches before its start
    bool pfb_zero_history = false;     // (plan_pfb; with the fused discriminator: of the launch and its halo chunk)
    const TapLaunch *d_tap_list = nullptr;
    const int32_t *d_group_bin0 = nullptr;   // per group of 16 tap slots: first bin of a run read straight from the ring, or -1
    std::vector<int32_t> tap_first_of_bin;
    std::vector<TapLaunch> tap_ordered;
    const RotFill *d_rot_fills = nullptr;
    const AudioLaunch *d_audf = nullptr;
    bool defer = false;                // a member of a group: mergeable records stay on the host (FirJob::host, disc_jobs, tails)
    bool history_done = false;         // launch_plan copied the history tail together with the launch records

    size_t reach(int id) const
    {
        if (!reach_x || reach_x->empty()) return 1;
        auto it = reach_x->find(id);
        return it == reach_x->end() ? (size_t)1 : std::max<size_t>(1, it->second);
    }
};

// channels of one (depth, D, T) class collected for launching
struct ClassPlan {
    std::vector<ChanLaunch> launches;
    std::vector<Chan *> launched;
    std::vector<DiscLaunch> discs;
    int max_n = 0;
    bool shared_src = true;
    bool all_bank_src = true;          // every launched channel's source is a filterbank bin
};

// what planning a block changed in the handle, so that it can be taken back while nothing has been queued
struct BlockUndo {
    struct Saved { Chan *c; Chan::Pos pos; };
    std::vector<Saved> saved;
    uint64_t serial_before = 0;
    bool armed = false;
};

// RCF_PLAN_PROF=1: host time per planning section -- total, calls, mean and the longest call -- printed at exit
// (tools/rt_probe.py runs with it)
struct PlanProf {
    static constexpr int N = 16;
    static bool on();
    static void add(int slot, const char *name, std::chrono::steady_clock::time_point &from);
};
#define RCF_PROF(slot, name, tp) do { if (PlanProf::on()) PlanProf::add(slot, name, tp); } while (0)

// rcf_plan.cpp
int plan_block(rcf_t *h, size_t n, BlockPlan &bp, BlockUndo &undo);
void undo_block(rcf_t *h, BlockUndo &undo);
size_t arena_need_bound(rcf_t *h);
const rcf_t::PlanCache &plan_cache(rcf_t *h);
int plan_arena(rcf_t *h, BlockPlan &bp);
int plan_pfb(rcf_t *h, BlockPlan &bp);
int plan_channel(rcf_t *h, BlockPlan &bp, ClassPlan &cp, Chan *c);
int plan_class_jobs(rcf_t *h, BlockPlan &bp, ClassPlan &cp, int depth, std::pair<int, int> cls_key);
int plan_tail(rcf_t *h, BlockPlan &bp);
int check_block_capacity(rcf_t *h, const BlockPlan &bp);
// rcf_launch.cpp
int launch_plan(rcf_t *h, BlockPlan &bp);
// ... and the steps a group block (rcf_group.cpp) launches the same way.  h: the handle whose timing, ring mask and
// arctangent table the launch uses -- the front-end itself, or the group's first member for what the group merged.
struct UploadSpan { size_t from, bytes; };             // the arena bytes [base, used) as the 64-byte blocks that hold them
UploadSpan arena_upload_span(size_t base, size_t used);
void launch_fir_job(rcf_t *h, FirJob &j, int timing_class, hipStream_t st);   // an unmerged FIR job, its repack first
// what follows the derived FIRs: one discriminator launch per job, then the uploaded stages of t
void launch_tail(rcf_t *h, const DiscJob *disc, size_t n_disc, const TailStages &t, hipStream_t st);
void launch_member_audio(rcf_t *h, const BlockPlan &bp, hipStream_t st);
void launch_member_pfb_squelch(rcf_t *h, const BlockPlan &bp, hipStream_t st);   // behind the bank's launch, single or grouped
int run_scan(rcf_t *h, const BlockPlan &bp);
int finish_block(rcf_t *h, const BlockPlan &bp);

}  // namespace rcfx
