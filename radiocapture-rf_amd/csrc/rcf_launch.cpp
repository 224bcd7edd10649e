// rcf_launch.cpp -- one front-end's block: upload the launch records, launch in dependency order, scan, history.
#include "rcf_plan.h"

namespace rcfx {

void flush_lagged(rcf_t *h)
{
    if (!h->lag.pending) return;
    h->lag.pending = false;
    Timed t(h, RCF_T_FIR_DERIVED);
    launch_fir_bank(h->lag.dev, h->lag.dims, h->stream);
}

// ---- the steps one front-end's block and a group block (rcf_group.cpp) launch the same way
UploadSpan arena_upload_span(size_t base, size_t used)
{
    const size_t from = base & ~size_t(63);
    return UploadSpan{from, used > base ? ((used + 63) & ~size_t(63)) - from : 0};
}

void launch_fir_job(rcf_t *h, FirJob &j, int timing_class, hipStream_t st)
{
    if (j.repack) {
        launch_fir_pack(j.dev, j.dims.n_chans, j.dims.T, const_cast<float *>(j.dims.bank), j.dirty, st);
        if (j.bc) j.bc->key = std::move(j.key);
    }
    Timed t(h, timing_class);
    launch_fir_bank(j.dev, j.dims, st);
}

// a stage's launch by its launcher's signature: (records, count, largest n_k, ring mask, stream), the AGC's with its longest window
template <class Rec>
static void launch_stage(const StageRecs<Rec> &s, void (*launch)(const Rec *, int, int, uint64_t, hipStream_t), uint64_t ring_mask, hipStream_t st)
{
    launch(s.dev, s.n(), s.max_n, ring_mask, st);
}
static void launch_stage(const AgcRecs &s, void (*launch)(const AgcLaunch *, int, int, int, uint64_t, hipStream_t), uint64_t ring_mask, hipStream_t st)
{
    launch(s.dev, s.n(), s.max_n, s.max_ns, ring_mask, st);
}

void launch_tail(rcf_t *h, const DiscJob *disc, size_t n_disc, const TailStages &t, hipStream_t st)
{
    for (size_t i = 0; i < n_disc; ++i) {
        Timed tm(h, RCF_T_DISC);
        launch_discriminator(disc[i].dev, disc[i].n(), disc[i].max_n, h->ring_mask, h->d_atan, st);
    }
    TailStages::each([&](int timing_class, auto launch, const auto &s) {
        if (!s.dev) return;
        if (timing_class == kNoTimingClass) { launch_stage(s, launch, h->ring_mask, st); return; }
        Timed tm(h, timing_class);
        launch_stage(s, launch, h->ring_mask, st);
    }, t);
}

void launch_member_audio(rcf_t *h, const BlockPlan &bp, hipStream_t st)
{
    if (!bp.d_audf) return;
    Timed t(h, RCF_T_AUDIO);
    launch_audio(bp.d_audf, (int)bp.audf.size(), bp.audf_max_n, bp.audf_num, bp.audf_den, h->ring_mask, h->d_atan, st);
}

// The carrier detector of every bin (rcf_pfb_squelch) over the frames the bank's launch of this block wrote.  The record is a
// kernel argument, built here: which of the state's two level arrays holds the levels is a fact of the LAUNCH order (a
// planned block that is taken back never gets here).
void launch_member_pfb_squelch(rcf_t *h, const BlockPlan &bp, hipStream_t st)
{
    if (!bp.run_pfb_squelch) return;
    Pfb::Squelch &q = h->pfb.sq;
    const PfbLaunch &pl = bp.pl;
    PfbSquelchLaunch p{};
    p.bins_ring = pl.bins_ring;
    p.level_in = q.level(q.cur);
    p.level_out = q.level(q.cur ^ 1);
    p.n_open = q.n_open(); p.last_open = q.last_open(); p.thr = q.thr(); p.mask = q.mask();
    p.z = q.d_z;
    p.ring_mask = pl.ring_mask;
    p.tile_pitch = pl.tile_pitch;
    p.i_lo = pl.n_lo - pl.n_abs0;
    p.alpha = q.alpha; p.a_pow_s = q.a_pow_s;
    p.n_frames = pl.n_frames; p.n_bins = pl.NB; p.frame_major = pl.frame_major;
    launch_pfb_squelch(p, st);
    q.cur ^= 1;
}

// upload all launch parameters in one copy, then launch in dependency order
int launch_plan(rcf_t *h, BlockPlan &bp)
{
    hipStream_t st = h->stream;
    PfbLaunch &pl = bp.pl;
    // ---- stage-2 lag.  The previous block's small-T launch, if it is still pending, rides in THIS block's filterbank launch
    // when that launch is the kernel that can carry it and the bank's ring has room for both blocks' frames; otherwise it
    // goes out now, ahead of everything of this block.
    const size_t pfb_reach = bp.reach(RCF_SRC_PFB_BIN0);
    const bool carry = bp.run_pfb && bp.shape.carries_s2 && !bp.pfb_zero_history;
    if (h->lag.pending && !(carry && (size_t)(pl.n_frames + h->lag.frames) + pfb_reach <= h->out_cap)) flush_lagged(h);
    S2Rider sr{};
    if (h->lag.pending) {
        const FirLaunchDims &ld = h->lag.dims;
        sr.chans = h->lag.dev;
        sr.atan_tab = ld.atan_tab;
        sr.ring_mask = ld.ring_mask;
        sr.D = ld.D; sr.T = ld.T; sr.KB = fir_small_outputs_rider(ld.D, ld.T);
        sr.n_chans = ld.n_chans;
        sr.n_tiles = (ld.max_n_k + sr.KB - 1) / sr.KB;
        sr.n_wgs = (sr.n_chans * sr.n_tiles + 7) & ~7;

        h->lag.pending = false;
    }
    // ... and this block's own: ONE small-T job on the bank's bins, nothing that consumes its outputs within the block (a
    // record of any tail stage, a voice chain: they read rings the lagged launch has not written)
    FirJob *lag_job = nullptr;
    if (h->lag_enabled && carry && bp.fir_by_depth.size() == 2 && bp.fir_by_depth[1].size() == 1 && bp.fir_by_depth[1][0].dims.small &&
        bp.fir_by_depth[1][0].dev && bp.fir_by_depth[1][0].bank_src && !bp.tails.any() && !bp.d_audf &&
        (size_t)pl.n_frames * 2 + pfb_reach <= h->out_cap)
        lag_job = &bp.fir_by_depth[1][0];
    {
        // the block's launch records host -> device, and -- in the same launch -- its history tail behind the OTHER input
        // buffer's block (nothing in this block reads that place, and the kernels that did read it are earlier in
        // the stream): one small launch per block instead of two
        const UploadSpan up = arena_upload_span(bp.arena_base, bp.ar->used);
        unsigned char *dst = bp.ar->d + up.from, *src = h->arenas.h_dev[bp.a] + up.from;
        // ... or none at all: when the filterbank's launch is the first of the block that needs neither (no direct
        // channels, no exact-rotator fill before it, no tap matrix whose slot list the bank itself reads from the
        // arena), its first workgroups do both copies on the way in (PfbLaunch::rider_*)
        const bool ride = bp.run_pfb && !bp.d_rot_fills &&
                          (bp.fir_by_depth.empty() || bp.fir_by_depth[0].empty()) && pl.n_taps == pl.tap_first &&
                          up.bytes / 8 < (1u << 31) && h->hist_cap < (1u << 28) && bp.shape.takes_rider;
        if (ride) {
            pl.rider_dst[0] = reinterpret_cast<unsigned long long *>(dst);
            pl.rider_src[0] = reinterpret_cast<const unsigned long long *>(src);
            pl.rider_n8[0] = (uint32_t)((up.bytes + 7) / 8);
            pl.rider_dst[1] = reinterpret_cast<unsigned long long *>(h->d_buf[h->cur ^ 1]);
            pl.rider_src[1] = reinterpret_cast<const unsigned long long *>(h->d_buf[h->cur] + bp.n);
            pl.rider_n8[1] = (uint32_t)(sizeof(float2) * h->hist_cap / 8);
        } else {
            Timed t(h, RCF_T_HISTORY);
            launch_copy8x2(dst, src, up.bytes, h->d_buf[h->cur ^ 1], h->d_buf[h->cur] + bp.n, sizeof(float2) * h->hist_cap, st);
        }
        bp.history_done = true;
        if (up.bytes) h->arenas.fill = (bp.ar->used + 63) & ~size_t(63);
    }
    if (bp.d_rot_fills) launch_rot_fill(bp.d_rot_fills, (int)bp.rot_fills.size(), h->ring_mask, st);
    if (!bp.fir_by_depth.empty())
        for (auto &j : bp.fir_by_depth[0]) launch_fir_job(h, j, j.dims.mfma ? RCF_T_FIR_MFMA : RCF_T_FIR, st);
    if (bp.run_pfb) { TimedAttached t(h, RCF_T_PFB, pl); launch_pfb(bp.shape, pl, bp.pfb_zero_history, st, sr.n_wgs ? &sr : nullptr); }
    launch_member_pfb_squelch(h, bp, st);
    if (bp.run_pfb && pl.n_taps > 0) {
        Timed t(h, RCF_T_TAPS);
        launch_tap_finalize(bp.d_tap_list, pl.n_taps, pl.tap_mat, pl.tap_pitch, pl.n_frames, pl.n_lo - pl.n_abs0,
                            h->ring_mask, h->d_atan, bp.d_group_bin0, pl.tap_first, pl.bins_ring, pl.NB, st);
    }
    for (size_t d = 1; d < bp.fir_by_depth.size(); ++d)
        for (auto &j : bp.fir_by_depth[d]) {
            if (&j == lag_job) {                            // not queued: it rides in the next block's filterbank launch
                h->lag.pending = true;
                h->lag.dims = j.dims;
                h->lag.dev = j.dev;
                h->lag.frames = pl.n_frames;
                continue;
            }
            Timed t(h, RCF_T_FIR_DERIVED);
            launch_fir_bank(j.dev, j.dims, st);
        }
    launch_tail(h, bp.disc_jobs.data(), bp.disc_jobs.size(), bp.tails, st);
    launch_member_audio(h, bp, st);
    return RCF_OK;
}

// the scan's share of the block: every frame that is complete now
int run_scan(rcf_t *h, const BlockPlan &bp)
{
    hipStream_t st = h->stream;
    const int64_t S0 = bp.S0, S1 = bp.S1;

    Scan &sc = h->scan;
    if (sc.armed && !sc.done) {
        int64_t avail = (S1 - sc.start_sample) / sc.N;
        if (avail > sc.n_frames) avail = sc.n_frames;
        while (sc.frames_done < avail) {
            const int cnt = (int)std::min<int64_t>(sc.chunk, avail - sc.frames_done);
            ScanLaunch sl{};
            sl.src.base = h->d_buf[h->cur];
            sl.src.mask = ~0ull;
            sl.src.origin = S0 - (int64_t)h->hist_cap;
            sl.src.stride = 1;
            sl.s0 = sc.start_sample + (int64_t)sc.frames_done * sc.N;
            sl.window = sc.d_window;
            sl.tw = sc.d_tw;
            sl.vring = sc.d_vring;
            sl.N = sc.N; sl.R = sc.R;
            sl.f0 = sc.frames_done; sl.n_frames = cnt;
            sl.scratch = sc.d_scratch;
            { Timed t(h, RCF_T_SCAN_FFT); launch_scan_fft(sl, st); }
            {
                Timed t(h, RCF_T_SCAN_MOVSUM);
                launch_scan_movsum(sc.d_vring, sc.N, sc.R, sc.L, sc.frames_done, cnt, sc.n_frames - 1, sc.d_sum,
                                   sc.d_out, st);
            }
            sc.frames_done += cnt;
        }
        if (sc.frames_done >= sc.n_frames) sc.done = true;
    }
    return RCF_OK;
}

// history for the next block, flip buffers
int finish_block(rcf_t *h, const BlockPlan &bp)
{
    hipStream_t st = h->stream;
    const size_t n = bp.n;
    const int64_t S1 = bp.S1;

    const int other = h->cur ^ 1;
    if (!bp.history_done) {
        Timed t(h, RCF_T_HISTORY);
        launch_copy8(h->d_buf[other], h->d_buf[h->cur] + n, sizeof(float2) * h->hist_cap, st);
    }
    if (h->eager_buf_done) {
        RCF_HIP(hipEventRecord(h->buf_done[h->cur], st));    // everything that reads this buffer is queued
        h->buf_done_set[h->cur] = true;
        h->buf_dirty[h->cur] = false;
    } else {
        h->buf_dirty[h->cur] = true;
    }
    h->cur = other;
    h->total_in = S1;
    RCF_HIP(hipGetLastError());
    return RCF_OK;
}

}  // namespace rcfx
