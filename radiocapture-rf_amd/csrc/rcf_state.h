// rcf_state.h -- host-side state of librcf.so (the kernels never see it): the front-end handle with its channels,
// filterbank, scanner, slab pools and launch arenas, and the helpers the host modules share.
//   rcf_handle.cpp   open / close / sync, pools, wideband ingest        rcf_plan.cpp    the per-block schedule (host)
//   rcf_launch.cpp   the block's launches in dependency order           rcf_chan.cpp    channels: lifecycle, taps, queries
//   rcf_stage.cpp    a channel's optional stages: symbol filter, AGC,   rcf_read.cpp    a channel's streams (one descriptor, Stream)
//                    symbol loops, slicer, the frame decoders behind it                 and the one read path of every host read
//                    (one record, Slicer::Frames), voice chain (attach / off)
//   rcf_streams.h    the stream table and the readers' integer rules (no HIP: g++ alone compiles it)
//   rcf_bank.cpp     filterbank + scanner ABI                           rcf_timing.cpp  HIP-event timing
//   rcf_comm.cpp     RCCL peak-list exchange                            rcf_group.cpp   grouped launches over front-ends
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "rcf_internal.h"
#include "rcf_streams.h"

namespace rcfx {

static const double kTwoPi = 6.283185307179586476925286766559;

static inline int64_t ceil_div(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }
static inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// A fresh device allocation that is freed again unless somebody takes it: what an attach function allocates is its own
// until the finished record is swapped into the channel, so a call that fails half way leaks nothing and changes nothing.
template <class T> struct Fresh {
    T *p = nullptr;
    Fresh() = default;
    Fresh(const Fresh &) = delete;
    Fresh &operator=(const Fresh &) = delete;
    ~Fresh() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, sizeof(T) * n); }
    T *take() { T *r = p; p = nullptr; return r; }
};

static size_t pow2_at_least(size_t v)
{
    size_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// one number per attachment of a counted stage (a symbol loop, the voice chain): a reader that keeps a position of its own
// in the stage's stream -- the pump's counted slots -- sees by it that the stage was attached again (a ring's address may
// come back from the allocator; this does not)
inline uint64_t next_stage_serial()
{
    static std::atomic<uint64_t> n{0};
    return ++n;
}

struct Chan {
    // ---- what planning a block reads and writes, together at the front of the object: the four cache lines plan_block
    // prefetches (with a thousand front-ends x 256 channels the planner's time is the cache misses of this walk).  The
    // static_asserts behind the struct hold the condition.
    int id = -1;
    int src = -1;                 // -1 wideband; RCF_SRC_PFB_BIN0 + bin; else source channel id
    int D = 0, T = 0;
    int depth = 0;
    bool fm_only = false;         // rcf_chan_set_fm_only: tap_finalize writes the discriminator ring only (a tap's IQ ring keeps
                                  // just the launch's last output, for the next launch's first discriminator sample)
    bool is_tap = false;          // a bin of a frame-major filterbank open as a channel: the bank's kernel copies it
                                  // into the launch's tap matrix, tap_finalize_kernel fills the rings
    float2 *d_ctaps = nullptr;
    float2 *d_iq = nullptr;
    float *d_fm = nullptr;
    int64_t start_sample = 0;     // in source index space
    int64_t k_abs0 = 0;
    // exact rotator (rcf_set_rotator): phase ring + {phase, counter} state, one pool slice
    float2 *d_rot = nullptr;
    // rotator model
    double extra_dangle = 0, extra_dlogmag = 0;   // added to the increment's own angle / log magnitude (filterbank taps)
    double dangle = 0, dlogmag = 0;
    // Everything planning a block advances, and nothing else: plan_block saves it before plan_channel touches the channel,
    // undo_block puts it back -- one assignment each, so a field added here cannot be missed by either.
    struct Pos {
        long double angle0 = 0;   // rotator model at output n_seg0
        double logmag0 = 0;
        int64_t n_seg0 = 0;
        int64_t produced = 0;     // relative output count
        // output range [blk_before, blk_after) the block with serial blk_serial gave this channel (its derived channels'
        // input range)
        int64_t blk_before = 0, blk_after = 0;
        uint64_t blk_serial = 0;
    } pos;
    // ---- the optional stages behind the rings, one record each; null = the channel has no such stage.  What a second
    // call of the attaching function means:
    //   stage                                  ring on re-call       from         read cursor
    //   symbol filter (rcf_chan_fm_filter)     kept                  kept         kept          (new taps and gain only)
    //   AGC           (rcf_chan_agc)           kept                  `produced`   `produced`
    //   symbol loops  (rcf_chan_clock_mm,      new ring and state    `produced`   0
    //                  rcf_chan_costas, rcf_chan_fsk4: one record shape, Loop, and one attach path, rcf_stage.cpp)
    //   voice chain   (rcf_chan_audio_open)    new                   `produced`   0
    // rec: the stage's launch record with everything that does not change from block to block -- rings, state, bank, taps,
    // constants as the kernel takes them -- filled at attach and nowhere else; the planner copies it and sets (n_lo, n_k).
    // `from`: the first relative channel output the stage is defined for (a new GR block: zero history before it; a record
    // with an n_first carries the same value); `rd`: items handed to the stage's reader; reach(): how far behind a block's
    // first output the stage reads the channel's rings; release(): the device buffers go once the stream has passed them
    // (rcf_stage.cpp)
    struct Sym {                        // real FIR over gain * fm (the P25 symbol filter)
        FmFirLaunch rec{};              // owns sym_ring and taps
        int64_t from = 0, rd = 0;
        size_t reach() const { return (size_t)std::max(1, rec.ntaps); }
        void release(rcf_t *h);
    };
    struct Agc {                        // feedforward_agc_cc(nsamples, reference) over the IQ stream (P25 CQPSK front half)
        AgcLaunch rec{};                // owns agc_ring
        int64_t from = 0, rd = 0;
        size_t reach() const { return (size_t)std::max(1, rec.nsamples - 1); }     // the window reaches n - 1 samples behind
        void release(rcf_t *h);
    };
    // what the three symbol loops share.  One allocation, which starts at the record's output ring (Ring): soft-symbol ring
    // of out_cap floats | the state record (rec.st), in a slot of whole 256 bytes | the caller's bank, if any (attach_loop,
    // rcf_stage.cpp).  rec.taps: the interpolator bank the stage reads, the caller's or rcf::d_mmse
    template <class State_, class Rec_, float *Rec_::*Ring> struct Loop {
        typedef State_ State;
        Rec_ rec{};
        int64_t from = 0, rd = 0;
        const uint64_t serial = next_stage_serial();
        float *&ring() { return rec.*Ring; }
        size_t reach() const { return 0; }                               // the history is in the state record: no look-back
        // the record's two counters on the device, n_out then slips (ClockState keeps them behind `p`: moving them to the
        // front, where the other two have them, changes clock_mm_kernel's code)
        const void *counters() const
        {
            static_assert(offsetof(State, slips) == offsetof(State, n_out) + sizeof(int64_t), "n_out, then slips");
            return &rec.st->n_out;
        }
        void release(rcf_t *h);
    };
    // (kWhat: the loop's name in the ABI -- RCF_READ_CLOCK / COSTAS / FSK4 --, by which a slicer names its source)
    struct Clock : Loop<ClockState, ClockLaunch, &ClockLaunch::sym_ring> {   // clock_recovery_mm_ff over gain * fm (SmartNet / EDACS)
        static constexpr int kWhat = RCF_READ_CLOCK;
        size_t reach() const { return (size_t)kClockTaps - 1; }         // a symbol's window starts up to 7 samples behind
    };
    // Gardner / Costas symbol recovery over the AGC ring (P25 CQPSK back half)
    struct Costas : Loop<CostasState, CostasLaunch, &CostasLaunch::sym_ring> { static constexpr int kWhat = RCF_READ_COSTAS; };
    // the C4FM symbol loop over the symbol-filter ring (P25 C4FM back half)
    struct Fsk4 : Loop<Fsk4State, Fsk4Launch, &Fsk4Launch::out_ring> { static constexpr int kWhat = RCF_READ_FSK4; };
    struct Audio {                      // the analog voice chain
        // owns st, the rings (one allocation from a_ring on: a | l | h | o | c (cf32), out_cap samples each) and the taps
        // (one allocation from lpf on: lpf | hpf | rs (padded))
        AudioLaunch rec{};
        int64_t from = 0, rd = 0;       // rd: audio samples handed to the reader
        const uint64_t serial = next_stage_serial();
        size_t reach() const { return (size_t)std::max(std::max(rec.n_lpf, rec.n_hpf), rec.nt_rs); }   // in the chain's own rings
        void release(rcf_t *h);
    };
    std::unique_ptr<Sym> sym;
    std::unique_ptr<Agc> agc;
    std::unique_ptr<Clock> clock;
    std::unique_ptr<Costas> costas;
    std::unique_ptr<Fsk4> fsk4;
    // Hard decisions behind ONE of the symbol loops (rcf_chan_slicer): packed words and sync hits.  One allocation, which
    // starts at rec.word_ring: word ring of out_cap words | the state record, in a slot of 256 bytes | hit ring of hit_cap
    // items.  A second call: new rings and state, cursors 0.  The stage has no `from`: it starts at a SYMBOL of its source
    // (rec.src0), and goes when that loop goes or is attached again (rcf_stage.cpp)
    struct Slicer {
        SliceLaunch rec{};
        int source = 0;                 // RCF_READ_CLOCK / COSTAS / FSK4
        uint32_t hit_cap = 0;
        int64_t rd_words = 0, rd_hits = 0;
        uint64_t serial = 0;            // which attachment its two streams belong to (next_stage_serial, set where the stage is
                                        // attached: max_frames_launch below builds a Slicer per call); a frame decoder has its own
        // The frame decoders out of the slicer's two streams: P25 trunking blocks (rcf_chan_tsbk), EDACS control frames
        // (rcf_chan_edacs), SmartNet OSWs (rcf_chan_osw), P25 voice data units (rcf_chan_p25lc).  One record shape.  A decoder hangs off the slicer -- Chan stays
        // inside its prefetched lines -- and goes whenever the slicer goes.  One allocation, which starts at rec.rec_ring:
        // record ring of cap records of the stream's item_w words | the state record, in a slot of 256 bytes.  A second
        // call: new ring and state, cursor 0 (attach_frames, rcf_stage.cpp).  kKind: the decoder's stream (rcf_streams.h:
        // its words per record, and its refusal); kName: how the messages spell it
        template <class State_, class Launch_> struct Frames {
            typedef State_ State;
            typedef Launch_ Launch;
            Launch rec{};
            uint32_t cap = 0;
            int64_t rd = 0;
            uint64_t serial = 0;        // set by attach_frames
        };
        struct Tsbk : Frames<TsbkState, TsbkLaunch> { static constexpr int kKind = kTsbk; static constexpr const char *kName = "TSBK"; };
        struct Edacs : Frames<EdacsState, EdacsLaunch> { static constexpr int kKind = kEdacs; static constexpr const char *kName = "EDACS"; };
        struct Osw : Frames<OswState, OswLaunch> { static constexpr int kKind = kOsw; static constexpr const char *kName = "OSW"; };
        std::unique_ptr<Tsbk> tsbk;
        std::unique_ptr<Edacs> edacs;
        struct P25lc : Frames<P25lcState, P25lcLaunch> { static constexpr int kKind = kP25lc; static constexpr const char *kName = "P25 voice"; };
        std::unique_ptr<Osw> osw;
        std::unique_ptr<P25lc> p25lc;
        // The one list of them.  At most one is ever attached: what they ask of the slicer excludes each other (TSBK: 2
        // bits per symbol; EDACS: binary, a 48-bit sync word; OSW: binary, an 8-bit sync word matched exactly), and the two
        // that ask the same, TSBK and the P25 voice stage (rcf_chan_p25lc), refuse each other by name
        template <class F> void for_each_frames(F &&f) { f(tsbk); f(edacs); f(osw); f(p25lc); }
        template <class R> std::unique_ptr<R> &frames()                  // the list's holder of an R
        {
            std::unique_ptr<R> *r = nullptr;
            for_each_frames([&r](auto &f) { if constexpr (std::is_same<std::unique_ptr<R> &, decltype(f)>::value) r = &f; });
            return *r;
        }
        static size_t max_frames_launch()                                // the largest launch record of the list
        {
            size_t n = 0;
            Slicer{}.for_each_frames([&n](auto &f) { n = std::max(n, sizeof(f->rec)); });
            return n;
        }
        size_t reach() const { return 0; }                               // it reads the loop's ring, never the channel's
        void release(rcf_t *h);
    };
    // Carrier detect over the IQ stream (rcf_chan_squelch): simple_squelch_cc's level and what it opened.  It writes no ring
    // and has no reader: its state record (one allocation, rec.st) is the result.  A second call: a new state, `from` = `produced`
    struct Squelch {
        SquelchLaunch rec{};            // owns st
        int64_t from = 0;
        size_t reach() const { return 0; }                               // the level is in the state record: no look-back
        void release(rcf_t *h);
    };
    // Carrier-operated capture over the IQ stream (rcf_chan_capture): the detector as a gate.  One allocation, which starts at
    // rec.cap_ring: captured ring of cap samples | record ring of rec_cap records | the state record, in a slot of 256 bytes.
    // A second call: new rings and state, cursors 0, `from` = `produced`
    struct Capture {
        CaptureLaunch rec{};            // owns cap_ring (rec_ring and st lie behind it)
        int64_t from = 0;
        uint32_t cap = 0, rec_cap = 0;
        int64_t rd = 0, rd_rec = 0;     // items handed to the two streams' readers
        const uint64_t serial = next_stage_serial();
        size_t reach() const { return (size_t)std::max(1, rec.pre); }    // the writer re-reads the IQ ring `pre` samples back
        void release(rcf_t *h);
    };
    std::unique_ptr<Audio> audio;
    std::unique_ptr<Slicer> slicer;
    std::unique_ptr<Squelch> squelch;
    std::unique_ptr<Capture> capture;
    // (the two plain readers' cursors: planning a block never looks at them, so they stand behind the stage holders it does
    // look at, which fill the fourth prefetched line to its end)
    int64_t rd_iq = 0, rd_fm = 0;
    // the one list of them: f(the stage's holder -- null when the channel has no such stage --, the bytes of its launch
    // record, whether its reach() is into rings of its own instead of the channel's)
    template <class F> void for_each_stage(F &&f)
    {
        f(sym, sizeof(FmFirLaunch), false); f(agc, sizeof(AgcLaunch), false); f(clock, sizeof(ClockLaunch), false);
        f(costas, sizeof(CostasLaunch), false); f(fsk4, sizeof(Fsk4Launch), false); f(audio, sizeof(AudioLaunch), true);
        f(slicer, sizeof(SliceLaunch) + Slicer::max_frames_launch() + 64, false);    // (with the frame decoder it may carry)
        f(squelch, sizeof(SquelchLaunch), false);
        f(capture, sizeof(CaptureLaunch), false);
    }
    // ---- the rest
    float incr[2] = {1.f, 0.f};   // exact rotator: what GNU Radio iterates
    uint64_t many_stamp = 0;      // the host_read call that last listed this channel (batched reads: one reader per stream)
    double src_rate = 0, offset_hz = 0;
    uint64_t taps_version = 0;    // bumped whenever d_ctaps changes (bank-matrix cache key)
    std::vector<float> proto;     // prototype taps (host)
};
// (offsetof of a class with non-trivial members: conditionally supported, and both compilers of this tree support it)
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Winvalid-offsetof"
static_assert(offsetof(Chan, pos) + sizeof(Chan::Pos) <= 192, "what plan_channel advances: inside the first three cache lines");
static_assert(offsetof(Chan, capture) + sizeof(std::unique_ptr<Chan::Capture>) <= 256, "what plan_channel reads: inside the four prefetched lines");
#pragma GCC diagnostic pop

struct Pfb {
    bool open = false;
    PfbShape shape;                // the bank's row of the shape table (pfb_shape.h), resolved once by rcf_pfb_open
    int NB = 0, D = 0, T = 0, P = 0;   // bins, decimation, prototype taps, taps per branch (= shape.NB, .D, .P)
    std::vector<float> proto;      // prototype taps (host): rcf_pfb_tap_open's GNU-Radio phase model needs them
    float *d_ptaps = nullptr;
    float2 *d_tw = nullptr;
    float2 *d_bins = nullptr;
    std::vector<int64_t> rd;       // per-bin read cursors
    int64_t start_sample = 0, n_abs0 = 0, produced = 0;
    int64_t produced_before = 0;   // value of `produced` before the current commit (for derived channels)
    // the discriminator fused into a frame-major bank (rcf_pfb_fm_enable): d_fm[(i & ring_mask) NB + k], i = frame - n_abs0
    int fm_mode = 0;               // 0 off, 1 beside the bins ring, 2 instead of it
    int fm_gr_phase = 0;
    float *d_fm = nullptr;
    float2 *d_fm_inc = nullptr;    // [NB] per-bin rotator increment as a phasor
    int64_t fm_from = 0;           // first relative frame the discriminator ring holds
    int64_t fm_until = 0;          // (fm_mode == 0) the frame the discriminator was switched off at
    // look-back form (pfb5_fmlb_kernel): edge rows + flags the chunks' workgroups hand their last frames over through
    unsigned long long *d_fm_edge = nullptr, *d_fm_flag = nullptr;
    int *d_fm_err = nullptr;
    int fm_slots = 0;
    int fm_local = 0;              // the hand-over stays in one XCD's L2 (pfb5_xcd_map_ok said so)
    uint64_t fm_serial = 0;        // launches so far (the flags' tags)
    std::vector<int64_t> rd_fm;    // per-bin read cursors
    // carrier detect on every bin (rcf_pfb_squelch): one state allocation of bins_pad = NB rounded up to 64 items per array,
    // level x 2 | n_open | last_open | thr | mask (PfbSquelchLaunch), and the z scratch of the largest launch the handle accepts
    struct Squelch {
        bool on = false;
        double alpha = 0, a_pow_s = 0;
        double *d_state = nullptr, *d_z = nullptr;
        size_t bins_pad = 0;
        int cur = 0;               // which level array holds the levels as of everything queued (a launch flips it)
        int64_t from = 0;          // first relative frame it saw, or will see
        int64_t until = 0;         // (off) the frame it was switched off at
        double *level(int which) const { return d_state + (size_t)which * bins_pad; }
        int64_t *n_open() const { return reinterpret_cast<int64_t *>(d_state + 2 * bins_pad); }
        int64_t *last_open() const { return reinterpret_cast<int64_t *>(d_state + 3 * bins_pad); }
        double *thr() const { return d_state + 4 * bins_pad; }
        uint32_t *mask() const { return reinterpret_cast<uint32_t *>(d_state + 5 * bins_pad); }
        size_t state_doubles() const { return 5 * bins_pad + bins_pad / 64; }
    } sq;
};

struct Scan {
    bool armed = false, done = false;
    int N = 0, n_frames = 0, L = 0, R = 0, chunk = 0;
    int frames_done = 0;
    int64_t start_sample = 0;
    float *d_window = nullptr, *d_vring = nullptr, *d_sum = nullptr, *d_out = nullptr;
    float2 *d_tw = nullptr, *d_scratch = nullptr;
    int64_t *d_peaks = nullptr;
    void *d_peak_ws = nullptr;
};

}  // namespace rcfx

namespace rcfx {
// Launch-parameter arenas: two pinned host buffers with device twins.  The records of successive blocks are APPENDED to the
// current one; only when it is full is an event recorded (every hipEventRecord costs ~6 us of queue gap: rocprof trace
// of the timed configuration) and the other one taken, once the kernels that read it have finished.
struct ArenaSet {
    size_t cap = 8u << 20;
    unsigned char *h[2] = {nullptr, nullptr};
    unsigned char *h_dev[2] = {nullptr, nullptr};     // the same pinned memory as the device sees it
    unsigned char *d[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    int cur = 0;
    size_t fill = 0;              // bytes of the current arena taken by earlier commits
    int create();                 // RCF_EHIP also when the pinned arenas cannot be mapped for the device (h_dev)
    void destroy();               // the stream that read them is idle
    int reserve(size_t need, hipStream_t stream);   // room for `need` more bytes in arena `cur` from `fill` on
};

// Pinned host memory that host_read's gather kernel reads its records from and writes the rows into, across PCIe (one per
// front-end, one per group).  Grows by powers of two from 64 KiB.
struct PinnedStage {
    unsigned char *h = nullptr, *d = nullptr;     // host address / the same memory as the device sees it
    size_t cap = 0;
    int ensure(size_t need, hipStream_t stream);  // RCF_ENOMEM when no mapped pinned memory of that size can be had
    void release() { if (h) (void)hipHostFree(h); h = d = nullptr; cap = 0; }
};
}  // namespace rcfx

using rcfx::Chan;
using rcfx::Pfb;
using rcfx::Scan;

struct rcf {
    int device = 0;
    int fault = 0;                 // sticky: a group block failed after its launches had been queued (set_dev refuses from then on)
    char fault_text[160] = "";
    double fs = 0, fc = 0;
    size_t block_cap = 0, hist_cap = 0, out_cap = 0;
    uint64_t blk_serial = 0;       // process_block count (Chan::blk_serial)
    uint64_t ring_mask = 0;
    hipStream_t stream = nullptr;
    float2 *d_buf[2] = {nullptr, nullptr};
    int cur = 0;
    int64_t total_in = 0;
    double shift_hz = 0;          // accumulated rcf_source_shift
    float *d_atan = nullptr;
    float *d_level = nullptr;     // rcf_chan_fm_level result
    float *d_mmse = nullptr;      // rcf_design_mmse_interpolator(8, 128, 0.25): the default bank of the symbol clocks, the Gardner / Costas and the C4FM loops, built at first use
    void *d_raw = nullptr;        // wire-format staging (rcf_push_raw), block_cap * 4 bytes, lazily allocated
    // launch-parameter arenas (pinned host + device), double buffered
    rcfx::ArenaSet arenas;
    // Stage-2 lag (rcf_launch.cpp): the small-T FIR + discriminator launch of the last block has NOT been queued -- it rides
    // in the next block's filterbank launch (S2Rider), or goes out on its own as soon as anybody could look at its outputs
    // (every entry point that touches the stream flushes it: set_dev).  RCF_S2_LAG=0 / rcf_set_stage2_lag(h, 0): off.
    struct Lag {
        bool pending = false;
        rcfx::FirLaunchDims dims{};
        const rcfx::ChanLaunch *dev = nullptr;
        int64_t frames = 0;           // bank frames of the block it belongs to (ring room: the next block must not overwrite them)
    } lag;
    bool lag_enabled = true;
    // a handle that belongs to a group (rcf_group_open) runs on the group's stream; its own comes back at rcf_group_close
    struct rcf_group *group = nullptr;
    hipStream_t own_stream = nullptr;
    std::map<int, std::unique_ptr<Chan>> chans;
    uint64_t chans_epoch = 0;     // bumped whenever a channel is opened or closed or gains / loses a symbol filter, AGC,
                                  // symbol clock, Gardner / Costas loop, C4FM loop or voice chain (cached Chan pointers: the pump's; the cached arena need below)
    // What planning a block needs to know about the channel SET (not their counters), valid while epoch == chans_epoch:
    // the summary plan_arena() used to rebuild from a walk over every channel, and the (depth, D, T) classes plan_block()
    // used to re-bucket -- three passes of pointer chasing per block (20 us of a 30 us plan for a front-end with 256
    // tapped bins once a thousand front-ends no longer fit the host's caches, RCF_PLAN_PROF).
    struct PlanCache {
        uint64_t epoch = ~0ull;
        std::unordered_map<int, size_t> reach_x;
        int max_depth = 0, min_d0 = 0;
        size_t max_reach = 1, arena_need = 0;
        typedef std::pair<std::pair<int, int>, std::vector<Chan *>> ClassBucket;
        std::vector<std::vector<ClassBucket>> by_depth;     // classes sorted by (D, T); channels in id order
    } plan_cache;
    int next_id = 1;
    Pfb pfb;
    Scan scan;
    // bank matrices of the matrix-core FIR path, one per (D, T) class, rebuilt when membership or taps change
    struct BankCache { std::vector<std::pair<int, uint64_t>> key; float *d = nullptr; size_t cap = 0; };
    std::map<std::pair<int, int>, BankCache> banks;
    uint64_t taps_clock = 0;
    // device buffers to release once the stream is idle: (pointer, pool slice bytes; 0 = plain hipFree)
    std::vector<std::pair<void *, size_t>> graveyard;
    // Channel buffers (rings, composite taps) come from slabs cut into equal slices, one pool per slice size:
    // opening a channel is a free-list pop instead of three hipMalloc + two memsets, closing one returns the
    // slices once the stream has passed them (create / release is what the reference's own self-test times,
    // frontend_connector.py:242-251)
    struct SlicePool { std::vector<void *> slabs, free_; };
    std::map<size_t, SlicePool> pools;
    std::map<int, std::vector<float>> proto_cache;   // channel_rate -> low_pass_2 prototype (rcf_chan_open)
    // H2D of block n+1 runs on its own stream while block n's kernels run (push_iq / push_raw)
    hipStream_t copy_stream = nullptr;
    hipEvent_t buf_done[2] = {nullptr, nullptr};   // the kernels that read d_buf[i] have finished
    hipEvent_t copy_ev = nullptr, raw_done = nullptr;
    bool buf_done_set[2] = {false, false};
    bool buf_dirty[2] = {false, false};   // kernels that read d_buf[i] were queued after buf_done[i] was last recorded
    bool eager_buf_done = false;          // a handle that is fed by rcf_push_iq records buf_done after every block (the
                                          // next block's copy overlaps this block's kernels); one fed in place
                                          // (rcf_ingest_ptr / rcf_commit) has no copy to order and records nothing
    bool raw_done_set = false;
    // RCCL communicator for the peak-list all-gather (rcf_comm_init); librccl is dlopen'ed on first use
    void *comm = nullptr;
    int comm_rank = 0, comm_size = 1;
    int64_t *d_gather = nullptr;
    size_t gather_cap = 0;
    rcfx::PinnedStage host_stage; // the handle's host reads (host_read, rcf_pfb_read_bin)
    // optional per-kernel-class HIP-event timing (rcf_timing_*)
    bool timing = false;
    unsigned timing_mask = ~0u;
    bool exact_rot = false;       // rcf_set_rotator / RCF_ROTATOR=exact: channels iterate GNU Radio's float32 rotator
    int decim_rule = RCF_DECIM_EXACT;   // rcf_set_decim_rule / RCF_DECIM_FLOOR=1
    uint64_t plan_calls = 0;            // blocks planned so far (RCF_FAIL_PLAN_AT)
    float2 *d_tapmat = nullptr;   // filterbank taps: the current launch's compact tap matrix (PfbLaunch::tap_mat)
    size_t tapmat_cap = 0;        // in float2
    float2 *d_partial = nullptr;  // split-K slabs of the matrix-core bank
    size_t partial_cap = 0;       // in float2
    struct TimeRec { int what; hipEvent_t a, b; };
    std::vector<TimeRec> time_pending;
    std::vector<hipEvent_t> time_pool;
    unsigned timing_stride = 1;   // rcf_timing_stride: events around every n-th launch of a class only
    unsigned time_seen[RCF_T_COUNT] = {0};
    double time_ms[RCF_T_COUNT] = {0};
    int64_t time_n[RCF_T_COUNT] = {0};
    std::mutex mu;
};

namespace rcfx {

// ---------------------------------------------------------------- rcf_handle.cpp
int set_dev(rcf_t *h);               // hipSetDevice + flush_lagged: what every entry point that touches the stream calls
int set_dev_ingest(rcf_t *h);        // hipSetDevice only: push / commit decide themselves what becomes of a lagging launch
void flush_lagged(rcf_t *h);         // rcf_launch.cpp
void bury(rcf_t *h, void *p, size_t slice = 0);
void free_graveyard_idle(rcf_t *h);      // the stream is known to be idle (the caller just synchronised it)
void drain_graveyard(rcf_t *h);
size_t slice_round(size_t bytes);
void *pool_get(rcf_t *h, size_t bytes);  // one slice of `bytes` (a multiple of 256) from the handle's pools

// ---------------------------------------------------------------- rcf_timing.cpp
hipEvent_t time_event(rcf_t *h);
void time_collect(rcf_t *h);

struct Timed {   // RAII: brackets the launches issued in its scope with two events on the stream
    rcf_t *h; int what; hipEvent_t a = nullptr;
    Timed(rcf_t *h_, int what_) : h(h_), what(what_)
    {
        if (h->timing && (h->timing_mask >> what & 1u) && (h->time_seen[what]++ % h->timing_stride) == h->timing_stride - 1) {   // the LAST of each group: never the first launch after a sync
            a = time_event(h);
            (void)hipEventRecord(a, h->stream);
        }
    }
    ~Timed()
    {
        if (!a) return;
        hipEvent_t b = time_event(h);
        (void)hipEventRecord(b, h->stream);
        h->time_pending.push_back({what, a, b});
    }
};

// The filterbank's launch is timed with the events ATTACHED to its dispatch (PfbLaunch::ev_start / ev_stop) instead of a
// bracket of two event records: one barrier packet less inside the measured interval (bracket 102.9 us, attached
// 101.1-102.2 on one box; rocprofv3's kernel trace reads another 2.5-5 us less).  RCF_TIMING_BRACKET=1 keeps the bracket.
struct TimedAttached {
    rcf_t *h; int what; PfbLaunch &pl; hipEvent_t a = nullptr, b = nullptr; bool bracket = false;
    TimedAttached(rcf_t *h_, int what_, PfbLaunch &pl_) : h(h_), what(what_), pl(pl_)
    {
        static const bool use_bracket = [] { const char *e = getenv("RCF_TIMING_BRACKET"); return e && atoi(e) != 0; }();
        pl.ev_start = pl.ev_stop = nullptr;
        if (h->timing && (h->timing_mask >> what & 1u) && (h->time_seen[what]++ % h->timing_stride) == h->timing_stride - 1) {
            a = time_event(h);
            bracket = use_bracket;
            if (bracket) { (void)hipEventRecord(a, h->stream); }
            else { b = time_event(h); pl.ev_start = a; pl.ev_stop = b; }
        }
    }
    ~TimedAttached()
    {
        pl.ev_start = pl.ev_stop = nullptr;
        if (!a) return;
        if (bracket) { b = time_event(h); (void)hipEventRecord(b, h->stream); }
        h->time_pending.push_back({what, a, b});
    }
};

// ---------------------------------------------------------------- rcf_chan.cpp
#define FIND_CHAN(h, id, c)                                                 \
    auto it_ = (h)->chans.find(id);                                         \
    if (it_ == (h)->chans.end()) { set_error("no such channel %d", id); return RCF_ENOCHAN; } \
    Chan *c = it_->second.get()

// source description for one commit
struct SrcRange {
    StreamView view;
    int64_t p0, p1;      // new samples [p0, p1) in the source's index space
};
bool source_range(rcf_t *h, int src, int64_t S0, int64_t S1, SrcRange *out);
int upload_composite(rcf_t *h, Chan *c);
double pfb_tap_gr_dangle(const rcf_t *h, int bin);
int pfb_fm_upload_increments(rcf_t *h);
// tap: a frame-major bank's tap (rcf_pfb_tap_open), copied by the bank's kernel -- the one bin consumer mode 2 keeps
int new_channel(rcf_t *h, int src, int D, const float *taps, int T, double offset_hz, int *chan_id, bool tap = false);
void free_channel(rcf_t *h, Chan *c);                 // c's device buffers go once the stream has passed them; the caller erases c
// a stage goes (switched off, replaced, or with its channel): release() its buffers, then the record
template <class R> void drop_stage(rcf_t *h, std::unique_ptr<R> &r) { if (r) { r->release(h); r.reset(); } }
template <class S, class R, float *R::*Ring> void Chan::Loop<S, R, Ring>::release(rcf_t *h) { bury(h, ring()); ring() = nullptr; rec.st = nullptr; rec.taps = nullptr; }   // one allocation

// ---------------------------------------------------------------- rcf_read.cpp
// ---- the one read path.  A stream is a device ring of `cap` items (a power of two) of item_w 4-byte words: item i at word
// (i & (cap - 1)) * stride_w of ring when stride_w > 1 (one bin of a frame-major ring of floats), else at
// (i & (cap - 1)) * item_w.  A plain stream's end the host knows: the ring holds the cap items before `newest`, a reader at
// *cursor may take up to `end`.  A counted stream -- counter != nullptr: a symbol loop's, the voice chain's, the slicer's, the TSBK, EDACS, OSW and P25 voice stages' --
// ends at ceil(*counter * interp / decim) of a DEVICE counter, which the counted gather reads itself (CountedRec,
// rcf_internal.h); serial: which attachment of the stage this is (a re-attached stage starts a new stream)
struct Stream {
    rcf_t *h = nullptr;
    const void *ring = nullptr;
    uint32_t item_w = 1, stride_w = 0;
    uint32_t cap = 0;                  // the handle's out_cap, or the ring's own (the slicer's hit ring, the frame decoders' records')
    int64_t *cursor = nullptr;
    int64_t end = 0, newest = 0;       // plain
    const int64_t *counter = nullptr;  // counted
    uint32_t interp = 1, decim = 1;
    uint64_t serial = 0;
};
// The channel's side of the stream table (rcf_streams.h): c's stream `kind`, or RCF_ESTATE with the row's refusal (IQ of a
// discriminator-only tap, a stage the channel does not carry).  Never touches the device.
int chan_stream(rcf_t *h, Chan *c, int kind, Stream *s);
// the front `bytes` of a stage's device state record: one asynchronous copy behind everything queued, one synchronisation
int stage_state(rcf_t *h, const void *d_state, void *st, size_t bytes);
// The round trip of a counted stream: its end as of everything queued, and in two[] the counter and the word behind it
// (the loops' {n_out, slips}, the voice chain's {n_a, n_prev}).  The produced / state queries' and rcf_pump_start's; no
// read needs it
int stream_count(rcf_t *h, const Stream &s, int64_t *end, int64_t two[2]);

// the gather record of the n items of s from *s.cursor on into the destination described by dst_* (GatherRec); float items
// leave multiplied by gain unless it is 1
inline GatherRec gather_rec(const Stream &s, int64_t n, uint32_t dst_w, uint32_t dst_pos_w, uint32_t dst_mask_w, float gain)
{
    return GatherRec{static_cast<const uint32_t *>(s.ring), (uint32_t)(((uint64_t)*s.cursor & (s.cap - 1u)) * s.item_w),
                     (uint32_t)n * s.item_w, s.cap * s.item_w - 1u, dst_w, dst_pos_w, dst_mask_w, gain,
                     gain != 1.0f ? 1u : 0u, s.stride_w};
}

// one entry of a host read: a stream, the row its items go to and at most how many.  s.ring == nullptr: nothing to read
// (*count holds the entry's error code already)
struct ReadEntry {
    Stream s;
    Chan *c = nullptr;            // batched reads: a channel listed twice in one call is refused (RCF_EINVAL)
    float gain = 1.0f;
    void *out = nullptr;
    int64_t max = 0;
    int64_t *count = nullptr;     // out: items read, or the entry's error code
};
// Every entry's new items in one gather launch (gather_rings; gather_counted for counted entries, which reserve
// min(max, cap) items of staging each and learn their counts and cursors from the launch's result words) into `stage`
// and one synchronisation of `stream`; then the rows are copied out, the cursors advanced and the graveyards of the idle
// handles (those on `stream`) released.  RCF_ECAP: the words do not fit the records' 32 bits; RCF_ENOMEM: no staging.
int host_read(PinnedStage &stage, hipStream_t stream, rcf_t *const *idle, size_t n_idle, ReadEntry *es, size_t n);
// a single reader: host_read of one entry on h's own stream and staging; the items read, or an error code
int64_t read_one(rcf_t *h, const Stream &s, float gain, void *out, size_t max_items);
// rcf_chan_read_many (hs = the handle, ms = nullptr) and rcf_group_read_many (hs = the members): entry i is channel
// chan_ids[i] of hs[ms[i]] as `what` (the caller has checked it with read_kind; RCF_READ_FM x gain) into row i of out;
// counts[i] its items or its error
int read_many(PinnedStage &stage, hipStream_t stream, rcf_t *const *hs, size_t n_hs, const int *ms, const int *chan_ids, int n,
              int what, float gain, void *out, size_t cap_each, int64_t *counts);

// ---------------------------------------------------------------- rcf_bank.cpp
void pfb_release(rcf_t *h);          // the bank's device buffers go once the stream has passed them; the bank is closed
// Bin `bin` of the bank's fused discriminator ring (rcf_pfb_fm_enable) as a stream for a reader at *cursor: frame-major
// floats, read with a stride of NB words; it ends at `produced`, or at the frame the discriminator was switched off at.
// false: no such ring or bin.  The two readers differ, and each keeps its way: rcf_pfb_read_fm (pump = false) measures a
// reader's lag from `produced` and relies on rcf_pfb_fm_enable to move rd_fm past frames that were never demodulated; the
// pump (pump = true) measures it from the stream's end and raises its own cursor to fm_from
bool pfb_fm_stream(rcf_t *h, int bin, int64_t *cursor, bool pump, Stream *s);

// ---------------------------------------------------------------- rcf_plan.cpp / rcf_launch.cpp
int process_block(rcf_t *h, size_t n);

// ---------------------------------------------------------------- rcf_comm.cpp
void comm_destroy(rcf_t *h);

}  // namespace rcfx
