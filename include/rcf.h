/*
 * rcf.h -- C ABI of librcf.so: the MI355X-native wideband channelizer, NBFM discriminator and FFT
 * peak scanner that replaces the GNU Radio hot path of MattMills/radiocapture-rf.
 *
 * The reference has no FFI of its own (it is pure Python on top of GNU Radio 3.8 blocks); this ABI is
 * the boundary a maintainer binds with ctypes (INTEGRATION.md shows the stub).  Every entry point
 * names the reference interface it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; device pointers are passed as void* / float*.
 *   - IQ is interleaved little-endian float32 re,im ("cf32", GNU Radio gr_complex), 8 bytes/sample.
 *   - every function returns RCF_OK (0) or a negative RCF_E* code and never throws; the text of the
 *     last failure on the calling thread is rcf_last_error().
 *   - one rcf_t is bound to one HIP device and one HIP stream; calls on one handle are serialised by
 *     an internal mutex (mirrors receiver.access_lock, rc_frontend/receiver.py:48).
 *   - there is NO CPU fallback: without a gfx950 device rcf_open() fails with RCF_EHIP.
 */
#ifndef RCF_H
#define RCF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rcf rcf_t;

#define RCF_OK        0
#define RCF_EINVAL   -1   /* bad argument */
#define RCF_ENOMEM   -2   /* host or device allocation failed */
#define RCF_EHIP     -3   /* HIP runtime error / no device */
#define RCF_ENOCHAN  -4   /* unknown channel id */
#define RCF_ECAP     -5   /* block larger than the configured capacity */
#define RCF_ESTATE   -6   /* call not valid in the current state */
#define RCF_EAGAIN   -7   /* result not ready yet */
#define RCF_ERANGE   -8   /* offset outside the source's band / non-integral decimation */

/* window types: numeric values follow gnuradio.filter.firdes.WIN_* */
#define RCF_WIN_HAMMING          0
#define RCF_WIN_BLACKMAN         2
#define RCF_WIN_KAISER           4   /* takes beta */
#define RCF_WIN_BLACKMAN_HARRIS  5

/* ------------------------------------------------------------------ library / device */
const char *rcf_version(void);
const char *rcf_last_error(void);
/* number of visible HIP devices (0 when none / no driver); never fails */
int rcf_device_count(void);
/* PCI address of HIP device `device` ("0000:75:00.0") into out[cap]: what maps a HIP ordinal to its sysfs node
 * (/sys/bus/pci/devices/<addr>/numa_node, local_cpulist) -- a box may show more cards in sysfs than HIP may use.
 * RCF_EINVAL: no such device / cap too small. */
int rcf_device_pci_bus_id(int device, char *out, size_t cap);

/* ------------------------------------------------------------------ filter design (host) */
/* gnuradio.filter.firdes.low_pass_2(gain, fs, fc, tw, att_dB, window) as called at
 * rc_frontend/channel.py:33 and p25_control_demod.py:106.  Writes the float32 taps; returns the tap
 * count, or -(needed count) when cap is too small (call with taps=NULL, cap=0 to size). */
int rcf_design_low_pass_2(double gain, double fs, double fc, double tw, double att_db, int window,
                          float *taps, int cap);
/* gnuradio.fft.window.{hamming,blackman,blackmanharris}(n) (fft_vector.py:38) */
int rcf_design_window(int window, int n, float *w);
/* firdes.low_pass / firdes.high_pass (gain, fs, cutoff, transition, window, beta): tap count from the window's
 * max_attenuation (Hamming 53, Blackman 74, Blackman-harris 92, Kaiser beta/0.1102+8.7).  Used by the analog
 * voice chain: firdes.high_pass(1, rate, 300, 30, WIN_HAMMING, 6.76) (logging_receiver.py:215) and the
 * rational resampler's Kaiser low-pass.  Same return convention as rcf_design_low_pass_2. */
#define RCF_FIR_LOW_PASS   0
#define RCF_FIR_HIGH_PASS  1
int rcf_design_firdes(int kind, double gain, double fs, double fc, double tw, int window, double beta,
                      float *taps, int cap);
/* gr-filter optfir.low_pass(gain, Fs, freq1, freq2, passband_ripple_db, stopband_atten_db): remezord() length
 * estimate + Parks-McClellan exchange (pm_remez, grid density 16, 2 extra taps) -- the audio low-pass inside
 * analog.fm_demod_cf (logging_receiver.py:214).  Same return convention as rcf_design_low_pass_2. */
int rcf_design_optfir_low_pass(double gain, double fs, double freq1, double freq2, double passband_ripple_db,
                               double stopband_atten_db, float *taps, int cap);
/* analog.fm_deemph(fs, tau) (gr-analog fm_emph.py): bilinear 1-pole/1-zero section -> iir_filter_ffd taps */
int rcf_design_fm_deemph(double fs, double tau, double btaps[2], double ataps[2]);
/* rational_resampler_fff(interpolation, decimation, taps=None, fractional_bw=None) (logging_receiver.py:216-221):
 * reduces by the gcd and designs firdes.low_pass(I, I, mid, width, WIN_KAISER, 7.0) with fractional_bw 0.4.
 * Writes the reduced ratio; same return convention for the taps. */
int rcf_design_resampler(int interpolation, int decimation, int *interp_out, int *decim_out, float *taps, int cap);
/* The MMSE fractional-delay interpolator bank of rcf_chan_clock_mm: nsteps + 1 rows of ntaps floats, row-major; row s, for
 * mu = s / nsteps, is the least-squares solution R h = r of minimising
 *     int_{-bw}^{bw} | sum_j h_j e^{-i 2 pi f j} - e^{-i 2 pi f (ntaps / 2 - mu)} |^2 df
 *     R[j][l] = 2 bw sinc(2 bw (j - l)),  r[j] = 2 bw sinc(2 bw (j - ntaps / 2 + mu)),  sinc(x) = sin(pi x) / (pi x)
 * solved in extended precision and rounded to float; rows 0 and nsteps are the unit rows e_{ntaps/2} and e_{ntaps/2 - 1}.
 * (8, 128, 0.25) has the shape, indexing and objective of GNU Radio's interpolator_taps.h, which a numerical minimiser
 * produced and which is printed to 6 digits: the two tables are not the same numbers, and how far apart they are has not
 * been measured.  ntaps even, 2 .. 64; nsteps 1 .. 4096; 0 < bw <= 0.5.  Same return convention as rcf_design_low_pass_2. */
int rcf_design_mmse_interpolator(int ntaps, int nsteps, double bw, float *taps, int cap);
/* rc_frontend/channel.py:31-33: decim = int(fs/cr)/2 (must be integral -> else RCF_ERANGE) and the
 * tap count of low_pass_2(1.0, fs, cr/2, cr/2, 20.0, WIN_HAMMING). */
int rcf_channel_params(double samp_rate, int channel_rate, int *decim, int *ntaps);
/* The same with the rule for a non-integral int(fs/cr)/2 spelled out.  rc_frontend/channel.py:31 was written for
 * Python 2, where int / int floors: the author's deployment (configs/config_denver_massive_p25.py:20,31: 10 666 666 sps,
 * receiver_split2 = False) ran 12.5 kHz channels at decim = 853 // 2 = 426, output rate 10 666 666 / 426 = 25 039 S/s.
 * Under Python 3 the same line hands GNU Radio 426.5 and the channel cannot be built.
 *   RCF_DECIM_EXACT (default)  reject (RCF_ERANGE) unless int(fs/cr) is even       -- Python 3 behaviour made explicit
 *   RCF_DECIM_FLOOR            decim = int(fs/cr) // 2                              -- what the Python 2 deployment ran
 * out_rate (may be NULL) = fs / decim: NOT 2 cr in the floored case; consumers read it from rcf_chan_info. */
#define RCF_DECIM_EXACT 0
#define RCF_DECIM_FLOOR 1
int rcf_channel_params_ex(double samp_rate, int channel_rate, int decim_rule, int *decim, int *ntaps, double *out_rate);

/* ------------------------------------------------------------------ front-end lifecycle */
/*
 * One rcf_t == one SDR source of the reference's receiver (rc_frontend/receiver.py:170-204): it owns
 * the HBM-resident wideband buffer that replaces the per-subscriber ZMQ copies of
 * `zeromq.pub_sink('ipc:///tmp/rx_source_<id>')` (receiver.py:201-202).
 *   block_capacity : max samples per push/commit            (0 -> 1<<22)
 *   hist_capacity  : samples of history kept before a block (0 -> 1<<16; must cover T-1, the PFB
 *                    prototype length and the scan FFT length)
 *   out_capacity   : per-channel output ring, samples, rounded up to a power of two (0 -> 1<<16)
 */
int rcf_open(int device, double samp_rate, double center_freq, rcf_t **out);
int rcf_open_ex(int device, double samp_rate, double center_freq, size_t block_capacity,
                size_t hist_capacity, size_t out_capacity, rcf_t **out);
int rcf_close(rcf_t *h);
/* How the channels' rotators run (freq_xlating_fir_filter_ccc's gr::blocks::rotator, rc_frontend/channel.py:35).
 * exact = 0 (default): GNU Radio's float32 increment in closed form (float64 model) -- any block size at full speed;
 *   the IQ stream is GNU Radio's up to a slowly turning common phase (7.7e-6 .. 4.3e-4 rad after 10^6 outputs),
 *   discriminator and magnitudes are not affected.
 * exact != 0: GNU Radio's own recurrence, phase *= incr in float32 with the renormalisation every 512 calls, iterated
 *   per channel on the device before each block's FIR launches: the IQ stream then carries GNU Radio's phase output for
 *   output at any stream length.  Sequential by nature (measured ~30 ns per output per block -- 0.15 ms for a 5243-output block, whatever the
 *   channel count: channels run side by side): meant for real-time
 *   block sizes.  Plain channels only -- filterbank bin taps keep the closed form (their rotator also carries the
 *   bank's own phases).  Must be called before the first channel is opened (RCF_ESTATE otherwise); the environment
 *   variable RCF_ROTATOR=exact sets it at rcf_open. */
int rcf_set_rotator(rcf_t *h, int exact);
/* Stage-2 lag (default on; RCF_S2_LAG=0 at rcf_open or on = 0 here: off).  On a handle whose block is a power-of-two
 * filterbank plus short stage-2 channels on its bins (rcf_pfb_chan_open: BASELINE configs[1]), the stage-2 launch of block
 * n is not queued behind block n's filterbank launch -- a latency-bound tail of ~19 us behind a bandwidth-bound 100 us
 * kernel -- but rides, as the first workgroups, in block n + 1's filterbank launch; every call that could observe its
 * outputs (reads, rcf_sync, channel control, timing reads, a block that cannot carry it) queues it on its own first.
 * Results are the same bits either way. */
int rcf_set_stage2_lag(rcf_t *h, int on);
/* The decimation rule rcf_chan_open / rcf_pfb_chan_open apply on this handle (rcf_channel_params_ex); default
 * RCF_DECIM_EXACT, or RCF_DECIM_FLOOR when the environment variable RCF_DECIM_FLOOR=1 is set at rcf_open. */
int rcf_set_decim_rule(rcf_t *h, int decim_rule);
/* wait until everything queued on the handle's stream has finished */
int rcf_sync(rcf_t *h);
/* the handle's hipStream_t, for callers that time the kernels with HIP events */
void *rcf_stream(rcf_t *h);
int rcf_device(rcf_t *h);

/* ------------------------------------------------------------------ measurement */
/* Per-kernel-class timing with HIP events recorded on the handle's own stream around each launch
 * (torch.cuda.Event would only see torch's stream).  Used by bench.py for roofline.achieved. */
#define RCF_T_FIR          0   /* direct xlating-FIR bank on the wideband stream, vector-FMA kernel */
#define RCF_T_PFB          1   /* polyphase filterbank kernel */
#define RCF_T_FIR_DERIVED  2   /* stage-2 / pre-filter FIRs on narrowband rings */
#define RCF_T_DISC         3   /* discriminator */
#define RCF_T_SCAN_FFT     4   /* scan FFT + log-magnitude */
#define RCF_T_SCAN_MOVSUM  5   /* scan running sum */
#define RCF_T_HISTORY      6   /* history carry-over copy */
#define RCF_T_FIR_MFMA     7   /* the same bank on the FP32 matrix cores (>= 8 channels on one source) */
#define RCF_T_AUDIO        8   /* analog voice chain (squelch/demod/de-emphasis walk, FIRs, resampler) */
#define RCF_T_TAPS         9   /* filterbank taps: tap matrix -> channel rings, rotator + discriminator fused */
#define RCF_T_CLOCK        10  /* symbol clocks (rcf_chan_clock_mm): one launch per block for every clocked channel */
#define RCF_T_COSTAS       11  /* Gardner / Costas loops (rcf_chan_costas): one launch per block for every channel with the stage */
#define RCF_T_FSK4         12  /* C4FM symbol loops (rcf_chan_fsk4): one launch per block for every channel with the stage */
#define RCF_T_SLICE        13  /* hard decisions (rcf_chan_slicer): one launch per block for every channel with the stage; and the
                                * launch of the TSBK stages behind them (rcf_chan_tsbk), one more per block with such a stage,
                                * and likewise that of the EDACS stages (rcf_chan_edacs) and of the OSW stages (rcf_chan_osw) */
#define RCF_T_COUNT        14
/* on = 0: off; 1: every class; otherwise a mask with bit (class + 1) set for each class to time -- every timed
 * launch costs two event records on the stream (~10 us of gap), so a throughput run times only what it reports.  The
 * filterbank's launch carries its two events attached to the dispatch (one barrier packet less inside the measured
 * interval; ~4 us per timed launch); RCF_TIMING_BRACKET=1 brackets it like the other classes. */
int rcf_timing_enable(rcf_t *h, int on);
/* events around every `every`-th launch of a timed class only (default 1 = every launch).  An event record is a
 * barrier packet: ~6 us of queue gap each on MI355X, two per timed launch -- at a 0.13 ms step that is 9 % of the
 * throughput being measured; a stride keeps the per-launch durations live and the stream nearly undisturbed. */
int rcf_timing_stride(rcf_t *h, int every);
/* accumulated milliseconds and launch count of one class since the last reset (syncs the stream) */
int rcf_timing_read(rcf_t *h, int what, double *total_ms, int64_t *launches, int reset);

/* ------------------------------------------------------------------ wideband ingest */
/* Host buffer in: copies n_samples H2D behind the history and runs every consumer (channels, PFB,
 * armed scan) over the new block.  Replaces the source -> pub_sink broadcast (receiver.py:201-202)
 * and every channel's sub_source (rc_frontend/channel.py:29).  Pageable or large blocks are copied on a second stream
 * (the copy of block n + 1 overlaps the kernels of block n); a block of <= 4 MiB in pinned memory (rcf_host_alloc) is
 * fetched by a kernel on the compute stream straight out of host memory -- no second stream, no cross-stream waits:
 * what a real-time block wants.  Returns once the caller's buffer has been read. */
int rcf_push_iq(rcf_t *h, const float *iq_interleaved, size_t n_samples);
/* Zero-copy ingest: *dev_ptr is where the producer (SDR DMA, generator kernel, hipMemcpy) must put
 * the next block (device memory, room for *max_samples); rcf_commit(n) then processes the n samples
 * found there.  rcf_commit without rewriting the region re-processes the resident data as the next
 * n samples of the stream (used by bench.py: inputs already resident in HBM). */
int rcf_ingest_ptr(rcf_t *h, float **dev_ptr, size_t *max_samples);
/* copy n_samples host samples to offset `at` (samples) of the pending block without processing them:
 * for drivers that deliver a block in pieces, and for pre-loading resident data */
int rcf_ingest_write(rcf_t *h, const float *iq_interleaved, size_t n_samples, size_t at);
int rcf_commit(rcf_t *h, size_t n_samples);
/* Wire-format ingest: the host hands over the SDR's native samples (2 or 4 bytes per complex sample
 * instead of 8 over PCIe) and the conversion the reference leaves to gr-osmosdr / gr-uhd on the host
 * (rc_frontend/receiver.py:74-98,170-191) runs on the GPU: x = (float(raw) - offset) * scale per
 * component, then the block is processed like rcf_push_iq.  rtl-sdr: RCF_FMT_U8, offset 127.4,
 * scale 1/128; sc16 (USRP wire, bladeRF Q11): RCF_FMT_S16, offset 0, scale 1/32768 or 1/2048.
 * A block of up to 4 MiB in pinned memory (rcf_host_alloc) is converted straight out of host memory -- one launch, no
 * staging copy: the shape of a real-time SDR block; larger ones go through a staged copy that overlaps the previous
 * block's kernels.  Either way the call returns once
 * the caller's buffer has been read. */
#define RCF_FMT_CF32 0   /* float32 I,Q interleaved (rcf_group_push only: rcf_push_iq is the single-front-end form) */
#define RCF_FMT_U8   1   /* unsigned 8-bit I,Q interleaved */
#define RCF_FMT_S8   2   /* signed 8-bit I,Q interleaved */
#define RCF_FMT_S16  3   /* signed 16-bit little-endian I,Q interleaved */
int rcf_push_raw(rcf_t *h, const void *iq_raw, size_t n_samples, int fmt, float scale, float offset);
/* total samples ingested so far */
int64_t rcf_samples_in(rcf_t *h);
/* Page-locked host memory for push buffers: a pinned buffer is DMA'd in place, and rcf_push_iq / rcf_push_raw copy
 * block n+1 on a separate stream while block n's kernels run (the reference's SDR driver thread filling the next
 * buffer while GNU Radio's scheduler works on the current one).  Pageable buffers work too, staged by the runtime. */
void *rcf_host_alloc(size_t bytes);
void rcf_host_free(void *p);

/* ------------------------------------------------------------------ direct ("xlat") channels */
/*
 * rcf_chan_open == channel.channel(parent_zmq_address, port, channel_rate, samp_rate, offset)
 * (rc_frontend/channel.py:18-38): decim = int(fs/cr)/2, taps = low_pass_2(1.0, fs, cr/2, cr/2, 20,
 * HAMMING), freq_xlating_fir_filter_ccc(decim, taps, offset, fs) with GNU Radio's float32 tap-phase
 * and rotator arithmetic.  Output rate fs/decim = 2*channel_rate.  The channel starts at the next
 * ingested sample with zero history (GR semantics).
 */
int rcf_chan_open(rcf_t *h, int channel_rate, double offset_hz, int *chan_id);
/* generic form: any decimation / prototype taps (e.g. the P25 69-tap pre-filter with decim 1,
 * p25_control_demod.py:106-108).  src_chan < 0: input is the wideband stream; otherwise the output of
 * PFB bin `src_chan - RCF_SRC_PFB_BIN0` (see rcf_pfb_chan_open) or of direct channel `src_chan`. */
int rcf_chan_open_taps(rcf_t *h, int src_chan, int decim, const float *taps, int ntaps,
                       double offset_hz, int *chan_id);
/* channel.set_offset (rc_frontend/channel.py:61-63): retune, keeping rotator phase and FIR history */
int rcf_chan_set_offset(rcf_t *h, int chan_id, double offset_hz);
/* channel.destroy (rc_frontend/channel.py:64-67) */
int rcf_chan_close(rcf_t *h, int chan_id);
int rcf_chan_info(rcf_t *h, int chan_id, int *decim, int *ntaps, double *out_rate, double *offset_hz);
/* samples produced so far / not yet read */
int64_t rcf_chan_produced(rcf_t *h, int chan_id);
/* index, in the channel's SOURCE stream (wideband samples for rcf_chan_open; frames of the bank / outputs of the parent
 * for chained channels and taps), of the first sample the channel sees -- everything before it counts as zero (GNU
 * Radio's zero history, the state a freshly started channel.py flowgraph is in).  The reference's data wire carries no
 * timestamps; with this a consumer can place output n at source sample start + n * decim. */
int64_t rcf_chan_start(rcf_t *h, int chan_id);
/* Non-blocking reads (return the sample count, 0 if nothing is ready, <0 on error).  read_iq is the
 * payload of the channel's zeromq.pub_sink (rc_frontend/channel.py:36); read_fm is
 * analog.quadrature_demod_cf(gain) applied to that stream (p25_control_demod.py:120-121,
 * moto_control_demod.py:105, edacs_control_demod.py:84, logging_receiver.py:233-234).  The two
 * cursors are independent.  A reader that falls more than out_capacity behind loses the oldest
 * samples (as a PUB socket at its HWM does). */
int64_t rcf_chan_read_iq(rcf_t *h, int chan_id, float *out_interleaved, size_t max_samples);
int64_t rcf_chan_read_fm(rcf_t *h, int chan_id, float gain, float *out, size_t max_samples);
/* The same reads for MANY channels behind one stream synchronisation -- what an egress pump that serves hundreds of
 * channel.py:36 PUB sockets needs per pass (a single-channel read costs a device round trip each).  what: RCF_READ_IQ
 * (out = float2[n_chans][cap_each]), RCF_READ_FM (out = float[n_chans][cap_each], scaled by gain) or RCF_READ_AGC
 * (out = float2[n_chans][cap_each], the AGC ring of rcf_chan_agc); counts[i] = samples copied for chan_ids[i] (0: nothing
 * new; RCF_ENOCHAN: no such channel, RCF_EINVAL: a channel listed a second time -- it has one reader position per stream;
 * RCF_ESTATE: the channel has no such stream -- IQ of a discriminator-only tap, AGC of a channel without one; the others
 * are still served).  `out` may be pinned memory (rcf_host_alloc): the copies then overlap each other.
 *   The streams of a channel's stages are batched the same way: RCF_READ_SYM .. RCF_READ_AUDIO, out =
 * float[n_chans][cap_each], gain ignored, RCF_ESTATE for a channel without that stage.  How many soft symbols or audio
 * samples a stage has produced only the device knows, so the gather reads the stage's counter itself: still one launch
 * and one synchronisation for the whole call.  The reader position is the one rcf_chan_read_sym / _clock / _costas /
 * _fsk4 / _audio use: batched and single reads of one channel interleave without loss or repeat.  Values 3 .. 15 of
 * `what` are not streams (RCF_EINVAL). */
#define RCF_READ_IQ 0
#define RCF_READ_FM 1
#define RCF_READ_AGC 2    /* cf32 rows from the AGC ring (rcf_chan_agc); the pump delivers it too */
#define RCF_READ_SYM     16   /* float32, symbol-filter ring (rcf_chan_fm_filter) */
#define RCF_READ_CLOCK   17   /* float32 soft symbols of rcf_chan_clock_mm */
#define RCF_READ_COSTAS  18   /* float32 soft symbols of rcf_chan_costas */
#define RCF_READ_FSK4    19   /* float32 soft symbols of rcf_chan_fsk4 */
#define RCF_READ_AUDIO   20   /* float32 audio of the voice chain */
/* The two streams of rcf_chan_slicer, batched the same way: out = uint32[n_chans][cap_each], gain ignored, RCF_ESTATE for a
 * channel without the stage; the reader positions are those of rcf_chan_read_hard / rcf_chan_read_sync.  They are not float
 * streams: rcf_pump_start and rcf_pump_subscribe refuse them (RCF_EINVAL), the real-time pump delivers them through
 * rcf_pump_subscribe_hard. */
#define RCF_HARD_BITS    32   /* uint32 words of packed decisions */
#define RCF_HARD_SYNC    33   /* uint32 sync hits, (distance << 26) | (k & 0x3ffffff) */
int rcf_chan_read_many(rcf_t *h, int what, const int *chan_ids, int n_chans, float gain, void *out, size_t cap_each,
                       int64_t *counts);
/* P25 C4FM front half after the discriminator (p25_control_demod.py:129-133, logging_receiver.py:240-244):
 * filter.fir_filter_fff(1, taps) over quadrature_demod_cf(gain) -- e.g. the 5-tap boxcar symbol filter
 * (1/sps,)*sps.  Enabled per channel; applies from the next block on; output read with rcf_chan_read_sym
 * at the channel's rate (the sequential symbol-timing loop behind it, op25 fsk4_demod_ff, is rcf_chan_fsk4, below; a
 * second call -- new taps -- keeps that stage running). */
int rcf_chan_fm_filter(rcf_t *h, int chan_id, float gain, const float *taps, int ntaps);
int64_t rcf_chan_read_sym(rcf_t *h, int chan_id, float *out, size_t max_samples);
/* P25 CQPSK front half after the pre-filter (p25_control_demod.py:146-149,182-183; logging_receiver.py:278-332 runs the
 * same chain on every call of a CQPSK system): analog.feedforward_agc_cc(nsamples, reference) on the channel's IQ
 * (p25_control_demod.py:149, logging_receiver.py:281) -- the multiply_const_cc(1.0) on either side is the identity.  With
 * x[m] = 0 before the stage's first input, N = nsamples, R = reference:
 *     env(z) = float(|re| > |im| ? (double)|re| + 0.4 (double)|im| : (double)|im| + 0.4 (double)|re|)
 *     out[n] = (R / max(1e-4f, max env(x[n-N+1 .. n]))) * x[n-N+1]          (float division, float products)
 * i.e. the input delayed by N - 1 samples, scaled by a gain that looks N - 1 samples ahead; the first N - 1 outputs are 0.
 * Bit-identical to GNU Radio's naive loop restated in float (every step is exactly rounded).  nsamples = 0 switches it off.
 * Starts, with zero history, at the channel's next output (again on every call); applies from the next block on, on every
 * channel kind (direct, chained, stage-2, filterbank tap); a retune keeps it, closing the channel releases it.  The
 * sequential loops behind it (op25 gardner_costas_cc, diff_phasor_cc) are rcf_chan_costas, below.
 * RCF_EINVAL: nsamples outside 0 .. 4096 or a non-finite reference; RCF_ENOCHAN: no such channel; RCF_ESTATE: a
 * discriminator-only tap (rcf_chan_set_fm_only: no IQ; switching that on is refused while an AGC reads the channel);
 * RCF_ECAP: out_capacity < 2 nsamples -- and at a block that yields more outputs than the ring holds beside the N - 1
 * samples of look-back (nothing is queued then).  nsamples = 0 on a channel that carries rcf_chan_costas: RCF_ESTATE (that
 * stage reads the AGC ring and must be switched off first; calling again with a window is allowed). */
int rcf_chan_agc(rcf_t *h, int chan_id, int nsamples, float reference);
/* unread AGC outputs (cf32), oldest first, at the channel's rate; RCF_ESTATE without an AGC */
int64_t rcf_chan_read_agc(rcf_t *h, int chan_id, float *out_interleaved, size_t max_samples);
/* device pointer of the AGC's cf32 ring and its capacity (zero-copy, like rcf_chan_rings): output n lives at index
 * n & (capacity-1), n counted as rcf_chan_produced counts the channel's outputs */
int rcf_chan_agc_ring(rcf_t *h, int chan_id, void **agc_ring, size_t *capacity);
/* The SmartNet and EDACS control demodulators behind the discriminator (moto_control_demod.py:105-132,
 * edacs_control_demod.py:82-112):
 *     quadrature_demod_cf(5) -> clock_recovery_mm_ff(rate / symbol_rate, 1.4395919, 0.5, 0.05, 0.005) -> binary_slicer_fb
 * digital.clock_recovery_mm_ff(omega, gain_omega, mu, gain_mu, omega_relative_limit) (moto_control_demod.py:113,
 * edacs_control_demod.py:85), the Mueller and Mueller symbol clock, as a per-channel stage on the GPU.  Per channel, all
 * state in float: mu, omega, last (initially 0) and the 64-bit input position p.  The input is u[m] = gain * fm[m], fm the
 * channel's unit-gain discriminator stream (one float product, the one rcf_chan_read_fm(gain) delivers), u[m] = 0 before
 * the stage's first input (the block's history of 8 taps, zero at the start); counted from that input p starts at -7.
 * T is the interpolator bank, 129 rows of 8 floats.  With omega_mid = omega and omega_lim = omega_mid *
 * omega_relative_limit rounded to float once, symbol k is produced as soon as u[p .. p + 7] all exist:
 *     imu  = (int)rintf(mu * 128.0f)
 *     y    = sum over j = 0 .. 7, in that order, from 0, of  T[imu][7 - j] * u[p + j]
 *     mm   = slice(last) * y - slice(y) * last                         slice(x) = x < 0 ? -1.0f : 1.0f
 *     last = y
 *     omega = omega + gain_omega * mm
 *     omega = omega_mid + 0.5f * (fabsf((omega - omega_mid) + omega_lim) - fabsf((omega - omega_mid) - omega_lim))
 *     mu   = mu + omega + gain_mu * mm                                 (left to right)
 *     step = (int)floorf(mu);  mu = mu - floorf(mu);  p += step        (a step beyond the int range saturates)
 *     out[k] = y;  bit k = y >= 0
 * every product and sum rounded to float on its own (no fused multiply-add).  Two guards keep the loop bounded on any
 * input, where GNU Radio reads out of bounds or asserts: a step < 1 advances p by 1; a mu or omega that is not finite after
 * the update puts the state back to (mu, omega_mid, last = 0) of the call and advances p by (int)ceilf(omega_mid).  Both
 * count in `slips`; neither happens on a signal a locked loop sees.  The outputs depend on the input stream only, never on
 * how it was cut into blocks: a symbol whose window crosses a block boundary comes with the block that completes it.
 * Against GNU Radio itself the stage is "parity unpinned" (DESIGN.md 2): its 8-tap sum is a volk dot product of unknown
 * order, its build may contract, and its table is not this one unless the caller passes it.
 * p == NULL switches the stage off.  It starts, with zero history, at the channel's next output (again on every call:
 * symbol 0 is the first of the call); applies from the next block on, on every channel kind (direct, chained, stage-2,
 * filterbank tap, discriminator-only taps included: it reads the discriminator ring, not the IQ); a retune keeps it,
 * closing the channel releases it.  The slicer and the packing are rcf_chan_slicer, below (which this
 * call detaches: its source starts again at symbol 0); packet framing stays with the consumer.
 * RCF_EINVAL: a non-finite parameter, omega * (1 - omega_relative_limit) < 2 (GNU Radio's documented domain), omega > 4096,
 * mu outside 0 .. 1; RCF_ENOCHAN: no such channel; RCF_ECAP: out_capacity < 16 -- and at a block that yields more outputs
 * than the ring holds beside the 7 samples of look-back (nothing is queued then). */
typedef struct rcf_clock_mm_params {
    float gain;                 /* quadrature_demod_cf gain in front (5 in both demods) */
    float omega, gain_omega, mu, gain_mu, omega_relative_limit;
    int reserved_;
    const float *interp_taps;   /* 129 x 8, row-major; NULL = rcf_design_mmse_interpolator(8, 128, 0.25) */
} rcf_clock_mm_params_t;
int rcf_chan_clock_mm(rcf_t *h, int chan_id, const rcf_clock_mm_params_t *p);
/* soft symbols produced since the stage was (last) enabled, and how often its guards fired; syncs the stream, like
 * rcf_chan_audio_produced.  RCF_ESTATE without the stage (here and in the two calls below) */
int rcf_chan_clock_produced(rcf_t *h, int chan_id, int64_t *n_symbols, int64_t *n_slips);
/* unread soft symbols (float32), oldest first; the bit of a symbol is (out[i] >= 0) */
int64_t rcf_chan_read_clock(rcf_t *h, int chan_id, float *out, size_t max_symbols);
/* device pointer of the soft-symbol ring and its capacity (zero-copy, like rcf_chan_rings): symbol k lives at index
 * k & (capacity-1); rcf_chan_clock_produced gives the count */
int rcf_chan_clock_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity);
/* The back half of the P25 CQPSK (LSM / simulcast) demodulators behind the AGC (p25_control_demod.py:150-183,
 * logging_receiver.py:282-332):
 *     repeater.gardner_costas_cc(omega, gain_mu, gain_omega, alpha, beta, fmax, -fmax) -> digital.diff_phasor_cc
 *         -> blocks.complex_to_arg -> multiply_const_ff(4 / pi)           [-> op25.fsk4_slicer_fb([-2, 0, 2, 4]) at the consumer]
 * as a per-channel stage on the GPU that reads the channel's AGC ring (rcf_chan_agc) and writes float32 soft symbols
 * (+-1, +-3 on a locked signal).  op25's source is not part of the reference tree, so this comment DEFINES the stage: it
 * restates the published gardner_costas_cc algorithm and is "parity unpinned"  against any particular op25
 * build -- unpinned against op25.
 * State per channel, all float: mu, omega, phase, freq, the complex `last`, the last 32 derotated samples, and 64-bit
 * counts of symbols and slips.  Constants: th = (float)(pi / 4), r = (float)0.70710678118654752, 2 pi as float,
 * omega_mid = omega, L = max(2 ceil(omega), floor(omega / 2) + 9) (12 at 25000 / 4800 as in op25, 11 at 25000 / 6000; the lower
 * bound keeps both interpolator windows inside samples that exist).  Initially mu = omega = omega_mid, phase = freq = 0,
 * last = 0, all 32 samples 0.  T is the interpolator bank of rcf_chan_clock_mm, 129 rows of 8 floats.  Every product and
 * sum is rounded to float on its own (no fused multiply-add); a complex product (a + jb)(c + jd) is (ac - bd) + j(ad + bc),
 * four products and two sums; |v| = sqrtf(re re + im im), correctly rounded; cosf, sinf and atan2f are the precise
 * functions; clamp(v, +-l) = v < -l ? -l : v > l ? l : v (a NaN passes).  For every AGC output x[m] from the stage's
 * start on:
 *   1. phase = phase + freq;  if phase > 2 pi: phase -= 2 pi;  if phase < -2 pi: phase += 2 pi
 *   2. a = phase + th;  push (cosf(a) + j sinf(a)) * x[m]        (W[0] oldest .. W[L-1] newest of the last L pushed)
 *   3. mu = mu - 1;  if mu > 1: next input
 *   4. half = omega * 0.5f;  hs = (int)floorf(half);  hm = (mu + half) - (float)hs;  if hm > 1: hm -= 1, hs += 1
 *      hs = min(hs, L - 8)                                        (never taken at P25's parameters: the window stays in W)
 *      I(v, m) = sum over j = 0 .. 7, in that order, from 0, of  T[clamp((int)rintf(m * 128.0f), 0, 128)][7 - j] * v[j]
 *                                                                 (real and imaginary part apart)
 *      mid = I(W[0 .. 7], mu);  y = I(W[hs .. hs + 7], hm)
 *      e = (last.re - y.re) * mid.re + (last.im - y.im) * mid.im;  a NaN counts as 0;  e = clamp(e, +-1)
 *      d = y * conj(last) = (y.re last.re + y.im last.im) + j (y.im last.re - y.re last.im);  last = y
 *      omega = omega + (gain_omega * e) * |y|;  omega = omega_mid + clamp(omega - omega_mid, +-omega_limit)
 *      mu = (mu + omega) + gain_mu * e
 *      z = d * (r + j r);  pe = |z.re| > |z.im| ? (z.re > 0 ? -z.im : z.im) : (z.im > 0 ? z.re : -z.re)
 *      freq = freq + (beta * pe) * |z|;  phase = (phase + freq) + (alpha * pe) * |z|, wrapped once as in 1
 *      freq = clamp(freq, +-max_freq)
 *      out[k] = atan2f(d.im, d.re) * (float)(4 / pi)
 * One guard, counted in n_slips: if after step 4 mu, omega, phase, freq or last is not finite, or mu <= 1, the state goes
 * back to the initial one (the 32 samples stay).  It does not fire on a signal.  At most one symbol per input; the outputs
 * depend on the input stream only, never on how it was cut into blocks.  freq is the carrier loop's estimate in radians
 * per channel sample, of the sign opposite to the carrier's offset: what a drift reporter needs.
 * p == NULL switches the stage off.  It starts, with zero history, at the channel's next output (again on every call: a
 * fresh ring and state, symbol 0 is the first of the call); applies from the next block on, on every channel kind that can
 * carry an AGC; a retune keeps it, closing the channel releases it.  The slicer is rcf_chan_slicer, below (which
 * this call detaches: its source starts again at symbol 0); the framing stays with the consumer.
 * RCF_EINVAL: a parameter that is not finite, omega outside 2 .. 16, omega - omega_limit - gain_mu < 2 (so that mu > 1
 * after every symbol), a negative omega_limit or max_freq, max_freq >= pi; RCF_ENOCHAN: no such channel; RCF_ESTATE: the
 * channel has no AGC; RCF_ECAP: out_capacity < 64. */
typedef struct rcf_costas_params {
    float omega;                /* channel samples per symbol: 25000 / 4800 (phase 1) or 25000 / 6000 (phase 2) */
    float gain_mu, gain_omega;  /* 0.025, 0.1 gain_mu^2 (p25_control_demod.py:152-153) */
    float alpha, beta;          /* 0.04, 0.125 alpha^2 */
    float max_freq;             /* 2 pi 1200 / rate; the reference passes +fmax and -fmax */
    float omega_limit;          /* 0.005 in op25: omega stays within omega_mid +- omega_limit */
    int reserved_;
    const float *interp_taps;   /* 129 x 8, row-major; NULL = rcf_design_mmse_interpolator(8, 128, 0.25) */
} rcf_costas_params_t;
int rcf_chan_costas(rcf_t *h, int chan_id, const rcf_costas_params_t *p);
/* the loop's state as of the last block; syncs the stream, like rcf_chan_clock_produced.  RCF_ESTATE without the stage
 * (here and in the two calls below) */
typedef struct rcf_costas_state {
    int64_t n_symbols, n_slips; /* soft symbols produced since the stage was (last) attached, times the guard fired */
    float mu, omega, freq, phase;
} rcf_costas_state_t;
int rcf_chan_costas_state(rcf_t *h, int chan_id, rcf_costas_state_t *out);
/* unread soft symbols (float32), oldest first */
int64_t rcf_chan_read_costas(rcf_t *h, int chan_id, float *out, size_t max_symbols);
/* device pointer of the soft-symbol ring and its capacity (zero-copy, like rcf_chan_rings): symbol k lives at index
 * k & (capacity-1); rcf_chan_costas_state gives the count */
int rcf_chan_costas_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity);
/* The back half of the P25 C4FM demodulators behind the symbol filter (p25_control_demod.py:118-135,
 * logging_receiver.py:231-251):
 *     op25.fsk4_demod_ff(autotuneq, sample_rate, symbol_rate)            [-> op25.fsk4_slicer_fb([-2, 0, 2, 4]) at the consumer]
 * as a per-channel stage on the GPU that reads the channel's symbol-filter ring (rcf_chan_fm_filter) and writes float32
 * soft symbols at the symbol rate (+-1, +-3 on a locked signal).  op25's source is not part of the reference tree, so this
 * comment DEFINES the stage: it restates the published fsk4_demod_ff tracking loop and is "parity unpinned" 
 * against any particular op25 build -- unpinned against op25.
 * All state is double, as in op25.  Every product, sum and quotient is rounded on its own (no fused multiply-add); a
 * division is the IEEE division.  time = symbol_rate / sample_rate (one double division).  T is the interpolator bank of
 * rcf_chan_clock_mm, 129 rows of 8 floats.  State per channel: clock = 0, spread = 2, fine = 0, coarse = 0, the last 8
 * inputs h[0 .. 7] (float, all 0 at the start, h[7] the newest), and 64-bit counts of symbols and slips.  For every
 * symbol-filter output u[m] from the stage's start on:
 *   1. clock = clock + time;  h[0 .. 6] = h[1 .. 7];  h[7] = u[m]
 *   2. if not (clock > 1): next input
 *   3. clock = clock - 1
 *      v = floor(0.5 + 128 * (clock / time));  imu = v < 0 ? 0 : v > 127 ? 127 : (int)v      (a NaN gives 0)
 *      a = sum over j = 0 .. 7, in that order, from 0.0, of (double)(T[imu][j] * h[j])       (float product, double sum;
 *                                                                                             the taps are NOT reversed)
 *      b = the same sum with row imu + 1
 *      a = a - fine;  b = b - fine
 *      out[k] = (float)((2 * a) / spread)
 *      if      a < -spread:  e = a + 1.5 * spread;  spread = spread - (e * 0.5) * k_spread
 *      else if a < 0:        e = a + 0.5 * spread;  spread = spread - e * k_spread
 *      else if a < spread:   e = a - 0.5 * spread;  spread = spread + e * k_spread
 *      else:                 e = a - 1.5 * spread;  spread = spread + (e * 0.5) * k_spread    (a NaN lands here)
 *      clock  = b < a ? clock + e * k_timing : clock - e * k_timing
 *      spread = spread < spread_min ? spread_min : spread;  spread = spread > spread_max ? spread_max : spread   (a NaN passes)
 *      coarse = coarse + (fine - coarse) * k_coarse
 *      fine   = fine + e * k_fine
 * One guard, counted in n_slips: if after step 3 clock, spread, fine or coarse is not finite, or clock is outside
 * -1 .. 2, the four go back to their initial values (the 8 inputs stay).  op25 has no such guard -- there a NaN stops the
 * loop for good.  It does not fire on a signal.  At most one symbol per input; the outputs depend on the input stream
 * only, never on how it was cut into blocks.
 * coarse is what op25 posts to its autotune queue: the slow average of the level offset, in units of the discriminator's
 * output, where one level step is symbol_deviation Hz at the gain of p25_control_demod.py:120 (rcf.p25.fm_gain).  It has
 * the sign of the carrier's offset and is the value adjust_channel_offset (p25_control_demod.py:205-212) would scale.
 * p == NULL switches the stage off.  It starts, with zero history, at the channel's next output (again on every call: a
 * fresh ring and state, symbol 0 is the first of the call); applies from the next block on, on every channel kind that can
 * carry a symbol filter (direct, chained, stage-2, filterbank tap -- a discriminator-only tap too: the stage reads no
 * IQ); a retune keeps it, a second rcf_chan_fm_filter call keeps it, closing the channel releases it.  The slicer is
 * rcf_chan_slicer, below (which this call detaches: its source starts again at symbol 0); the framing stays with the consumer.
 * RCF_EINVAL: a parameter that is not finite, sample_rate / symbol_rate outside 2 .. 4096, spread_min or spread_max not
 * 0 < spread_min <= 2 <= spread_max; RCF_ENOCHAN: no such channel; RCF_ESTATE: the channel has no symbol filter;
 * RCF_ECAP: out_capacity < 16. */
typedef struct rcf_fsk4_params {
    double sample_rate, symbol_rate;    /* the channel's rate and 4800 (phase 1) or 6000 (phase 2): time = symbol_rate / sample_rate */
    double k_spread, k_timing;          /* 0.01, 0.025 in op25 */
    double k_fine, k_coarse;            /* 0.125, 0.00125 */
    double spread_min, spread_max;      /* 1.6, 2.4: the distance of two levels stays within 20 % of the nominal 2 */
    const float *interp_taps;           /* 129 x 8, row-major; NULL = rcf_design_mmse_interpolator(8, 128, 0.25) */
    int reserved_;
} rcf_fsk4_params_t;
int rcf_chan_fsk4(rcf_t *h, int chan_id, const rcf_fsk4_params_t *p);
/* the loop's state as of the last block; syncs the stream, like rcf_chan_costas_state.  RCF_ESTATE without the stage
 * (here and in the two calls below) */
typedef struct rcf_fsk4_state {
    int64_t n_symbols, n_slips; /* soft symbols produced since the stage was (last) attached, times the guard fired */
    double clock, spread, fine, coarse;
} rcf_fsk4_state_t;
int rcf_chan_fsk4_state(rcf_t *h, int chan_id, rcf_fsk4_state_t *out);
/* unread soft symbols (float32), oldest first */
int64_t rcf_chan_read_fsk4(rcf_t *h, int chan_id, float *out, size_t max_symbols);
/* device pointer of the soft-symbol ring and its capacity (zero-copy, like rcf_chan_rings): symbol k lives at index
 * k & (capacity-1); rcf_chan_fsk4_state gives the count */
int rcf_chan_fsk4_ring(rcf_t *h, int chan_id, void **sym_ring, size_t *capacity);
/* Hard decisions behind a symbol loop: the step that follows the soft symbols in every demodulator chain of the reference,
 *     op25.fsk4_slicer_fb([-2, 0, 2, 4])                                   (p25_control_demod.py:167-168, logging_receiver.py:250-251,307-308)
 *     digital.binary_slicer_fb -> blocks.unpacked_to_packed_bb(1, GR_MSB_FIRST)   (moto_control_demod.py:114-115, edacs_control_demod.py:86-90)
 * and the consumers' search for the frame-sync word (p25_control_demod.py:337 5575f5ff77ff, moto_control_demod.py:216
 * 10101100, edacs_control_demod.py:523 its 48-bit word), as one more optional stage per channel on the GPU.  It reads the
 * soft-symbol ring of ONE of the channel's symbol loops and writes two streams: packed decisions and sync hits.  All of it is
 * integer work on the loop's float32 outputs: the streams are exactly what the rules below give for the soft symbols the
 * loop's own reader delivers.
 * Decision d[k] of soft symbol s[k]:
 *     RCF_SLICE_BINARY   d = s >= 0 ? 1 : 0                                                       (a NaN gives 0)
 *     RCF_SLICE_FSK4     d = s < levels[0] ? 3 : s < levels[1] ? 2 : s < levels[2] ? 0 : 1        (a NaN gives 1; levels[3] decides nothing, as in op25)
 * k counts from the stage's start: the loop's n_symbols at the moment of the call (which reads that counter and so
 * synchronises the stream, as rcf_chan_fsk4_state does).
 * Bit stream: per symbol the 1 or 2 bits of d (bps), the higher one first; bits fill bytes from the top place down --
 * unpacked_to_packed_bb(bps, GR_MSB_FIRST) -- and bytes fill 32-bit words in memory order: byte j of the stream is byte
 * j & 3 of word j >> 2 (little-endian), so a uint8 view of the word ring is GNU Radio's byte stream and a frame-aligned P25
 * stream shows 55 75 f5 ff 77 ff as it stands.  The stream's items are whole words, 32 / bps symbols each; the unfinished
 * word stays in the stage's state and leaves when it is full (at most 15 dibits, 3.3 ms at 4800 baud, late).
 * Sync hits: L = sync_bits / bps.  For every k >= L - 1, dist = popcount((window ^ sync_word) & (2^sync_bits - 1)), window =
 * the last sync_bits bits of the bit stream ending with symbol k, the oldest bit highest.  If dist <= sync_max_errors one
 * item is appended to the hit ring: uint32 = (dist << 26) | (k & 0x3ffffff), k the LAST symbol of the window; items are in
 * increasing k.  A reader widens k against n_symbols: the largest value <= n_symbols - 1 with those low 26 bits.  Neither
 * stream depends on how the input was cut into blocks.  The word ring has out_capacity words, the hit ring hit_capacity
 * items; a reader that falls more than a ring behind loses the oldest.
 * Both polarities (sync_both = 1; edacs_control_demod.py:401-408 accepts its frame sync inverted): an item is appended as
 * well when dist >= sync_bits - sync_max_errors, i.e. when the window is within sync_max_errors of the inverted word.  The
 * item carries dist as it is: a reader takes dist > sync_bits / 2 as "inverted, at distance sync_bits - dist".  With
 * sync_both = 0 nothing of this applies.
 * p == NULL switches the stage off.  It applies from the next block on, on every channel kind its source loop supports; a
 * retune keeps it, calling again starts it afresh (new rings and state, k = 0 at the loop's next symbol), closing the
 * channel releases it.  Switching the source loop off, or attaching it again (a fresh ring, symbol 0), DETACHES the slicer:
 * it must be attached again behind the new loop.  A channel has at most one slicer.
 * RCF_EINVAL: an unknown source or mode, levels that are not finite or not non-decreasing (RCF_SLICE_FSK4), sync_bits not 0
 * or 8 .. 64 and a multiple of the bits per symbol, sync_max_errors outside 0 .. sync_bits - 1 (0 without a search),
 * hit_capacity not 0 or a power of two >= 16 (at most 2^26), sync_both not 0 or 1, or 1 with 2 sync_max_errors >= sync_bits
 * (the two polarities' ranges of dist would meet); RCF_ENOCHAN: no such channel; RCF_ESTATE: the channel does not
 * carry the named loop; RCF_ECAP: out_capacity < 64. */
#define RCF_SLICE_BINARY 1
#define RCF_SLICE_FSK4   2
typedef struct rcf_slicer_params {
    int source;            /* RCF_READ_CLOCK, RCF_READ_COSTAS or RCF_READ_FSK4: the loop whose soft symbols are sliced */
    int mode;              /* RCF_SLICE_BINARY (1 bit per symbol) / RCF_SLICE_FSK4 (2 bits per symbol) */
    float levels[4];       /* RCF_SLICE_FSK4 only: -2, 0, 2, 4 in the reference */
    uint64_t sync_word;    /* the low sync_bits bits, first-received bit highest */
    int sync_bits;         /* 0: no search; else 8 .. 64 and a multiple of the bits per symbol */
    int sync_max_errors;   /* a hit is a Hamming distance <= this, 0 .. sync_bits - 1 (63 at most) */
    int hit_capacity;      /* items of the hit ring, a power of two >= 16; 0 = 256 */
    int sync_both;         /* 0: the word as given; 1: its inverse is searched as well (see above) */
} rcf_slicer_params_t;
int rcf_chan_slicer(rcf_t *h, int chan_id, const rcf_slicer_params_t *p);
/* the stage's counters as of the last block; syncs the stream.  RCF_ESTATE without the stage (here and in the calls below) */
typedef struct rcf_slicer_state {
    int64_t n_symbols, n_words, n_hits;   /* symbols sliced, whole words written, hits appended since the stage was (last) attached */
} rcf_slicer_state_t;
int rcf_chan_slicer_state(rcf_t *h, int chan_id, rcf_slicer_state_t *out);
/* unread words of packed decisions / unread sync hits, oldest first (one round trip each) */
int64_t rcf_chan_read_hard(rcf_t *h, int chan_id, uint32_t *out, size_t max_words);
int64_t rcf_chan_read_sync(rcf_t *h, int chan_id, uint32_t *out, size_t max_hits);
/* device pointers of the word ring and the hit ring and their capacities (zero-copy, like rcf_chan_fsk4_ring): word i lives
 * at index i & (word_capacity - 1), hit i at i & (hit_capacity - 1); rcf_chan_slicer_state gives the counts.  Any of the
 * four may be NULL. */
int rcf_chan_slicer_rings(rcf_t *h, int chan_id, void **word_ring, size_t *word_capacity, void **hit_ring, size_t *hit_capacity);
/* P25 trunking blocks behind a slicer: what the reference's consumer does per frame of a control channel in Python
 * (p25_control_demod.py:337-364, p25_general.procTSDU / subprocTSBK / procStatus / data_deinterleave / trellis_1_2_decode /
 * crc16), as one more optional stage per channel on the GPU.  It reads the slicer's own two streams and writes a third, the
 * counted stream RCF_HARD_TSBK of 32-byte records: a consumer of a control channel takes the 12-octet TSBKs instead of every
 * word of the dibit stream.  All of it is integer work: the records are exactly what the rules below give for the words and
 * hits the slicer's readers deliver.  (The reference reads NAC and DUID uncorrected and so does rcf_chan_tsbk; BCH
 * correction of the NID is the option of rcf_chan_tsbk_ex below.  No other data unit than the TSDU, no parsing of a TSBK's
 * fields.)
 * Frames.  A hit item gives k, the last dibit of the sync word (widened against n_symbols as above); the frame starts at
 * dibit s = k - 23.  Hits are taken in order; a hit is ACCEPTED if k >= k_last_accepted + 24 (buf.find(sync, fsoffset + 6)),
 * the first one the stage considers always.  An accepted hit is DECIDED in the first block after which the slicer's whole
 * words hold the dibits up to s + 384, 16 n_words >= s + 384: the 360 dibits of the longest TSDU and the 24 of a sync word
 * that may begin inside them -- so every hit that can shorten the frame is in the hit ring by then and the stream does not
 * depend on how the input was cut into blocks.  frame_dibits = min(360, s_next - s), s_next the frame start of the next
 * accepted hit if there is one by then.  Dibit r of the frame is stream dibit s + r; info dibit j sits at r = j + j / 35
 * (every 36th dibit is a status symbol).
 * NID: info bits 48 .. 111; nac = info bits 48 .. 59, duid = info bits 60 .. 63.
 * Blocks are decoded only when duid == 7.  Block b (0, 1, 2) is the info dibits 56 + 98 b .. 153 + 98 b and is decoded if its
 * last dibit lies inside the frame, r(153 + 98 b) < frame_dibits (for frames of 180, 288 and 360 dibits the reference's
 * `while len(bitframe) >= 196`).
 * Deinterleave: code word t = 0 .. 47 is the block's dibits i + j, i + j + 1 with i = 2 (t / 4), j = (0, 26, 50, 74)[t % 4];
 * code word 48 is the dibits 24, 25.
 * Trellis: state 0 at the start; per code word c (4 bits) the new state is the candidate d whose word W[state][d] has the
 * most bits equal to c, the lowest d of equals; W = {2 C 1 F, E 0 D 3, 9 7 A 4, 5 B 6 8}.  The output is the first 48
 * states = 96 bits; n_inexact counts the code words (0 .. 49) with no candidate equal to c.
 * CRC: register 0, every one of the 96 bits shifted in, xor 0x1021 when bit 16 falls out; the block is good iff the register
 * ends at 0xffff.
 * Records, 8 uint32 each, in increasing k, then b:
 *     word 0    bits 0-1 b (3: a frame record without a block), bit 2 CRC bad, bit 3 next_bit, bits 4-9 n_inexact,
 *               bits 10-15 the hit's distance, bits 16-19 duid, bits 20-31 nac
 *     word 1    the low 32 bits of the widened k
 *     word 2-4  the 96 decoded bits, the first bit highest, bytes in memory order (the word ring's rule: a uint8 view is the
 *               12 octets); 0 in a frame record
 *     word 5-6  the NID's 64 bits, same rule
 *     word 7    bits 0-15 frame_dibits; bits 16-20 RCF_NID_BCH's, bits 21-29 RCF_TRELLIS_VITERBI's (below); else zero
 * next_bit is the info bit that follows the block's last one if it lies inside the frame, else 0 (procTSDU stops behind a
 * block that is followed by a 1).  A frame record goes out for an accepted frame with duid != 7 or with no whole block.
 * Lost: hits that left the hit ring before they were examined, and frames whose first word the word ring had overwritten
 * when they were decided, are skipped and counted (n_lost); a lost frame still counts as accepted.
 * p == NULL switches the stage off.  It applies from the next block on and considers only hits appended after the call (hit
 * index >= the slicer's n_hits at that moment: the call reads that counter and so synchronises the stream); calling again
 * starts it afresh.  It goes when the slicer goes: slicer attached again or switched off, its source loop attached again or
 * switched off, channel closed.
 * RCF_ESTATE: the channel has no slicer in RCF_SLICE_FSK4 mode that searches a 48-bit sync word, or that slicer searches both
 * polarities (sync_both = 1), or it carries the P25 voice stage (rcf_chan_p25lc); RCF_EINVAL: capacity not 0 or a power of
 * two >= 16 (at most 2^20); RCF_ENOCHAN: no such channel.
 * The NID (RCF_NID_BCH; rcf_chan_tsbk_ex here, rcf_chan_p25lc_ex for the voice stage).  The NID's first 63 bits are a word
 * of the binary BCH(63,16,23) code, t = 11: code bit i (0 .. 62) is info bit 48 + i of the frame -- bits 0 .. 11 the nac,
 * bits 12 .. 15 the duid -- and the coefficient of x^(62 - i), data first, in rs64.py's msg order.  The code is the binary
 * subfield subcode of RS(63,41,23) over GF(64) with x^6 + x + 1, alpha = 2 and the roots alpha^1 .. alpha^22 -- rs64.Codec(23)
 * on 63 symbols that are all 0 or 1 --; its generator, the lcm of those roots' minimal polynomials, is octal
 * 6331141367235453.  Info bit 111, the NID's 64th bit, takes no part (as the (24,12) Golay word's 24th bit without the
 * erasure option).  With the option the result is the code word within 11 bits of the received 63 if there is one -- it is
 * unique, d being 23 --: nac and duid are its first 16 bits and nid_fix is the number of bits it changes, 0 .. 11.  If there
 * is none, nac and duid stand as received and nid_fix = 15.  The decoder is complete inside the bound.  The decoded duid is
 * the one the stage acts on: "blocks are decoded only when duid == 7" here, the unit's kind in the voice stage.  The record's
 * nac and duid carry the decoded values; a TSBK record's words 5-6 keep the 64 bits as received, so a consumer sees both.
 * TSBK record: word 7 bits 16-19 nid_fix, bit 20 set (the NID went through the decoder).  Voice record: word 7 bits 28-31
 * nid_fix, word 0 bit 9 set.  Without the option (RCF_NID_RAW) all of these bits are 0.  The option is fixed for a stage's
 * life; calling an attach again starts the stage afresh with that call's value, so the records stay independent of how the
 * input is cut.  rcf_chan_tsbk(h, c, p) is rcf_chan_tsbk_ex(h, c, p, RCF_NID_RAW): one attach path.  RCF_EINVAL as well: nid
 * neither RCF_NID_RAW nor RCF_NID_BCH.
 * The trellis (RCF_TRELLIS_VITERBI; rcf_chan_tsbk_opt).  The paragraph "Trellis" above is the reference's walk: it decides
 * code word by code word and never looks back, so one wrong bit that leaves two candidates of a row tied at three equal
 * bits (0x2 / 0x1 and 0xC / 0xF of row 0 are 2 bits apart) can take the wrong one, and every later state follows from it.
 * With the option a block is decoded as a whole, by maximum likelihood for hard decisions.  A block is the same 49 code
 * words c_0 .. c_48.  A path is a state sequence s_0 .. s_48 with s_-1 = 0 and s_48 = 0: the encoder's flushing dibit
 * (the reference ignores the 49th code word; this rule uses it).  A path's cost is the sum over t of
 * popcount(W[s_(t-1)][s_t] xor c_t), with the W above.  The result is the path of least cost, among equal costs the
 * lexicographically smallest (s_0, s_1, ...); the output is s_0 .. s_47 = 96 bits as above.  Sequentially:
 * beta_48[s] = popcount(W[s][0] xor c_48); for t = 47 .. 0, beta_t[s] = min over d of popcount(W[s][d] xor c_t) +
 * beta_(t+1)[d]; then forward from state 0, at step t the lowest d that minimises popcount(W[s][d] xor c_t) + beta_(t+1)[d]
 * (at t = 48: d = 0).  Costs stay <= 4 x 49 = 196: small-integer work, no rounding.  The free distance of W's trellis is
 * 5, so every pattern of at most 2 wrong bits in a block's 196 is corrected.  If the reference's walk finds a candidate
 * equal to c at all 49 code words, both rules give the same 96 bits: that path costs 0, and a path of cost 0 is unique
 * because the four words of a row of W differ.
 * Records with the option: n_inexact (word 0 bits 4-9) counts the code words (0 .. 49) that differ from the chosen path's
 * word -- the meaning above, on the new path --; word 7 bits 21-28 hold the path's cost (0 .. 196) and bit 29 is set (the
 * block went through this decoder); in a frame record (b = 3) bits 21-29 are 0.  CRC bad, next_bit, the octets and all else
 * follow from the decoded bits by the rules above.  With RCF_TRELLIS_GREEDY all of these bits are 0 and the records are
 * those of rcf_chan_tsbk_ex bit for bit.  Like nid the option is fixed for a stage's life; attaching again starts the stage
 * afresh with that call's value.  It applies to the TSBK stage only (the voice stage has no trellis).
 * rcf_chan_tsbk_ex(h, c, p, nid) is rcf_chan_tsbk_opt(h, c, p, nid, RCF_TRELLIS_GREEDY): one attach path.  RCF_EINVAL as
 * well: trellis neither RCF_TRELLIS_GREEDY nor RCF_TRELLIS_VITERBI.  With p == NULL (the stage switched off) neither nid nor
 * trellis is looked at: the call returns what rcf_chan_tsbk(h, c, NULL) returns. */
typedef struct rcf_tsbk_params {
    int capacity;          /* records of the ring, a power of two >= 16; 0 = 256 */
    int reserved_[3];
} rcf_tsbk_params_t;
int rcf_chan_tsbk(rcf_t *h, int chan_id, const rcf_tsbk_params_t *p);
#define RCF_NID_RAW 0u   /* nac and duid as received (the reference's reading) */
#define RCF_NID_BCH 1u   /* the NID's BCH(63,16,23) word decoded first: the rule above */
int rcf_chan_tsbk_ex(rcf_t *h, int chan_id, const rcf_tsbk_params_t *p, uint32_t nid);
/* the NID decoder's counters of the channel's TSBK or voice stage as of the last block; syncs the stream: frames whose NID
 * went through the decoder, of them with nid_fix 1 .. 11, the sum of those nid_fix values, frames with nid_fix = 15.  All 0
 * for a stage attached with RCF_NID_RAW.  RCF_ESTATE: the channel has neither stage */
typedef struct rcf_nid_state { int64_t n_decoded, n_fixed, n_bits, n_bad; } rcf_nid_state_t;
int rcf_chan_nid_state(rcf_t *h, int chan_id, rcf_nid_state_t *out);
#define RCF_TRELLIS_GREEDY  0u   /* the reference's walk: the paragraph "Trellis" */
#define RCF_TRELLIS_VITERBI 1u   /* the least-cost path that ends in state 0: the paragraph "The trellis" */
int rcf_chan_tsbk_opt(rcf_t *h, int chan_id, const rcf_tsbk_params_t *p, uint32_t nid, uint32_t trellis);
/* the trellis decoder's counters of the channel's TSBK stage as of the last block; syncs the stream: blocks that went through
 * the decoder, of them with cost 0, the sum of the costs, the sum of the n_inexact values.  All 0 for a stage attached with
 * RCF_TRELLIS_GREEDY.  RCF_ESTATE: the channel has no TSBK stage */
typedef struct rcf_trellis_state { int64_t n_decoded, n_clean, n_bits, n_words; } rcf_trellis_state_t;
int rcf_chan_trellis_state(rcf_t *h, int chan_id, rcf_trellis_state_t *out);
/* the stage's counters as of the last block; syncs the stream.  RCF_ESTATE without the stage (here and in the calls below) */
typedef struct rcf_tsbk_state {
    int64_t n_records, n_frames, n_blocks, n_crc_bad, n_lost;   /* records written, frames accepted (decided or lost), blocks decoded, of them with a bad CRC, hits and frames lost */
} rcf_tsbk_state_t;
int rcf_chan_tsbk_state(rcf_t *h, int chan_id, rcf_tsbk_state_t *out);
/* unread records, oldest first: out = uint32[max_records][8] (one round trip); RCF_HARD_TSBK names the stream to
 * rcf_chan_read_many and rcf_group_read_many (out = uint32[n_chans][cap_each][8]); the pump delivers it
 * through rcf_pump_subscribe_hard */
#define RCF_HARD_TSBK    48
int64_t rcf_chan_read_tsbk(rcf_t *h, int chan_id, uint32_t *out, size_t max_records);
/* device pointer of the record ring and its capacity in records (zero-copy): record i lives at word 8 (i & (capacity - 1)) */
int rcf_chan_tsbk_ring(rcf_t *h, int chan_id, void **rec_ring, size_t *capacity);
/* EDACS control frames behind a slicer: what the reference's consumer does per 288-bit frame of a control channel in Python
 * strings (edacs_control_demod.py: get_next_frame 396-430, packet_framer 373-395, bch_decode 451-518, message_election
 * 172-189), as one more optional stage per channel on the GPU.  It applies to a slicer in RCF_SLICE_BINARY mode that searches
 * a 48-bit sync word, with sync_both 0 or 1.  It reads the slicer's own two streams and writes a third, the counted stream
 * RCF_HARD_EDACS of 32-byte records, one per frame: a consumer takes the two elected 40-bit messages instead of every word
 * of the bit stream.  All of it is integer work: the records are exactly what the rules below give for the words and hits the
 * slicer's readers deliver.  (No parsing of a message's fields.)
 * Frames.  A hit item gives k, the last bit of the sync word (widened against n_symbols as above); the frame starts at bit
 * s = k - 47 and its 240 data bits are the stream bits s + 48 .. s + 287.  Hits are taken in order; a hit is ACCEPTED if
 * k >= k_last_accepted + 288 (buf = buf[find + 288:]), the first one the stage considers always.  An accepted hit is DECIDED
 * in the first block after which the slicer's whole words hold the frame, 32 n_words >= s + 288.  A frame is never shortened,
 * so later hits cannot matter and the records do not depend on how the input was cut into blocks.  A hit is INVERTED if the
 * slicer searches both polarities and the item's dist > 24; all 240 bits of an inverted frame are inverted first.
 * Copies.  Copy c (0 .. 5) is the frame's data bits 40 c .. 40 c + 39; the copies 1 and 4 are inverted (packet_framer).
 * BCH(48,36) over GF(64), alpha^6 = alpha + 1 (the reference's _GF_ALPHA / _GF_IDX).  Per copy the received polynomial has
 * coefficient j = copy bit 39 - j for j = 0 .. 39 and 0 for j = 40 .. 62 (eight zero colour bits stand in front of the copy).
 * S_i = xor over the set j of alpha^(i j mod 63), i = 1, 3 (S2 and S4 are S1^2 and S1^4 and decide nothing).
 *     S1 = 0, S3 = 0      the copy stands
 *     S1 = 0, S3 != 0     the copy stands as well, uncorrected and valid: the reference's fall-through (76 of 3000 words with
 *                         three errors come back as received), reproduced here
 *     S1 != 0, S3 = S1^3  one error at position p = log S1
 *     otherwise           aux = S1^3 ^ S3, e1 = (log S1^2 - log aux) mod 63, e2 = (log S1 - log aux) mod 63; the positions are
 *                         i % 63 for every i in 1 .. 63 with 1 ^ alpha^((e1 + i) % 63) ^ alpha^((e2 + 2 i) % 63) = 0; the copy
 *                         FAILS unless exactly two positions result
 * The copy FAILS if any position is > 47.  Positions 40 .. 47 (the colour bits) are accepted and change none of the 40 bits;
 * a position p in 0 .. 39 flips copy bit 39 - p.
 * Election (message_election), per message -- m1 of the copies 0 .. 2, m2 of the copies 3 .. 5 -- over the corrected copies:
 * none decoded: no message; exactly one decoded: that one; otherwise the first value that two decoded copies share, else no
 * message.  With esk != 0 the first four bits of an elected message are or-ed with 0xA.
 * Records, 8 uint32 each, in increasing k:
 *     word 0    bit 0 inverted, bit 1 m1 present, bit 2 m2 present, bits 4-9 the hit's distance from the polarity it matched,
 *               bits 10-21 two bits per copy (copy c in the bits 10 + 2 c): 0 clean or stands, 1 one position, 2 two
 *               positions, 3 failed
 *     word 1    the low 32 bits of the widened k
 *     word 2-3  the 40 bits of m1, the first bit highest, bytes in memory order (the word ring's rule: a uint8 view is the
 *               5 octets), the rest 0; all 0 when absent
 *     word 4-5  m2 likewise
 *     word 6-7  0
 * Lost: hits that left the hit ring before they were examined, and frames whose first word the word ring had overwritten
 * when they were decided, are skipped and counted (n_lost); a lost frame still counts as accepted.
 * Departure: get_next_frame searches its whole string buffer for the inverted word first and only then for the upright one;
 * the stage takes the hits in stream order.  On a stream of one polarity the two agree.
 * p == NULL switches the stage off.  It applies from the next block on and considers only hits appended after the call (hit
 * index >= the slicer's n_hits at that moment: the call reads that counter and so synchronises the stream); calling again
 * starts it afresh.  It goes when the slicer goes: slicer attached again or switched off, its source loop attached again or
 * switched off, channel closed.  A slicer carries this stage or the TSBK stage, by its mode.
 * RCF_ESTATE: the channel has no slicer in RCF_SLICE_BINARY mode that searches a 48-bit sync word; RCF_EINVAL: capacity not
 * 0 or a power of two >= 16 (at most 2^20); RCF_ENOCHAN: no such channel. */
typedef struct rcf_edacs_params {
    int capacity;          /* records of the ring, a power of two >= 16; 0 = 256 */
    int esk;               /* != 0: extended addressing, the first four bits of every elected message |= 0xA */
    int reserved_[2];
} rcf_edacs_params_t;
int rcf_chan_edacs(rcf_t *h, int chan_id, const rcf_edacs_params_t *p);
/* the stage's counters as of the last block; syncs the stream.  RCF_ESTATE without the stage (here and in the calls below) */
typedef struct rcf_edacs_state {
    int64_t n_records, n_frames, n_msgs, n_msgs_none, n_lost;   /* records written, frames accepted (decided or lost), messages elected, messages without a result, hits and frames lost */
} rcf_edacs_state_t;
int rcf_chan_edacs_state(rcf_t *h, int chan_id, rcf_edacs_state_t *out);
/* unread records, oldest first: out = uint32[max_records][8] (one round trip); RCF_HARD_EDACS names the stream to
 * rcf_chan_read_many and rcf_group_read_many (out = uint32[n_chans][cap_each][8]); the pump delivers it
 * through rcf_pump_subscribe_hard */
#define RCF_HARD_EDACS   49
int64_t rcf_chan_read_edacs(rcf_t *h, int chan_id, uint32_t *out, size_t max_records);
/* device pointer of the record ring and its capacity in records (zero-copy): record i lives at word 8 (i & (capacity - 1)) */
int rcf_chan_edacs_ring(rcf_t *h, int chan_id, void **rec_ring, size_t *capacity);
/* SmartNet outbound signalling words (OSWs) behind a slicer: what the reference's consumer does per 84-bit frame of a control
 * channel in Python strings (moto_control_demod.py: receive_engine 212-331 -- the framing with its lock counter 252-281 and
 * 521-525, deinterleave 198-203, the parity syndrome and its correction 284-320, the two xor masks 325-330), as one more
 * optional stage per channel on the GPU.  It applies to a slicer in RCF_SLICE_BINARY mode that searches an 8-bit sync word
 * (10101100 there) with sync_max_errors = 0 and sync_both = 0.  It reads the slicer's own two streams and writes a third, the
 * counted stream RCF_HARD_OSW of 32-byte records, one per frame.  All of it is integer work: the records are exactly what
 * the rules below give for the words and hits the slicer's readers deliver, however the input was cut into blocks.
 * Notation.  Bits are the slicer's bit stream; a hit item gives k, the last bit of the sync word (widened against n_symbols
 * as above), and the hit STARTS at h = k - 7.  W = 32 n_words.  State: the cursor pos, a bit index, initially the slicer's
 * n_symbols at the call; locked, an int32, initially 0, which can go negative (it stops at the least int32); is_locked.
 * Only hits appended after the call and with h >= pos are considered.
 * One step at pos:
 *   A. locked >= 4, or locked == 3 and a hit starts at pos: the frame is at pos.  Decided in the first block with
 *      W >= pos + 84.  rel = 0 with a hit at pos; without one only rel != 0 matters (260-263) and the record carries 65535.
 *   B. anything else: h0 = the first hit with h >= pos (the stage waits for one), h1 = the first hit with h >= h0 + 8.
 *      Decided in the first block with W >= h0 + 92: by then every hit that starts in h0 + 8 .. h0 + 84 is there.  With
 *      locked <= 2 the candidate is accepted iff h1 - h0 == 84 (260); otherwise pos = h0 + 8 (525) and n_rejects += 1.  With
 *      locked == 3 it is accepted regardless.  rel = h0 - pos.
 *   Accepted: (1) rel != 0: locked -= 1, else locked += 1 if locked < 5;  (2) is_locked = locked >= 5;  (3) n_frames += 1;
 *      (4) with locked > 2 now, the packet is the bits pos + 8 .. pos + 83 and pos += 84;  (5) otherwise the packet is the bits
 *      h0 + 8 .. h0 + 83 and pos = h0 + 84.
 * Packet b[0 .. 75]: out[4 x + j] = b[x + 19 j], x = 0 .. 18, j = 0 .. 3 (deinterleave); data[i] = out[2 i], parity[i] =
 * out[2 i + 1], i = 0 .. 37; psyn[i] = parity[i] ^ data[i] ^ data[i - 1] with data[-1] = 0.  If any psyn bit is set:
 * n_bad += 1 and data[x] ^= psyn[x] & psyn[x + 1] for x = 0 .. 36 (psyn itself is not modified, bit 37 is never corrected);
 * else, if rel != 0, locked += 1 (320).  lid = data[0 .. 15] ^ 0xcc38, individual = data[16], cmd = data[17 .. 26] ^ 0xd5,
 * the first bit highest; the bits 27 .. 37 are delivered and not interpreted (the reference does not check them).
 * Records, 8 uint32 each, in increasing position:
 *     word 0    bit 0 sync at the cursor (rel == 0), bit 1 syndrome nonzero, bit 2 is_locked, bit 3 individual, bits 4-9 the
 *               number of data bits flipped, bits 10-15 the number of set psyn bits, bits 16-31 min(rel, 65535)
 *     word 1    the low 32 bits of the packet's sync position (the packet's first bit - 8)
 *     word 2    lid | cmd << 16
 *     word 3-4  the 38 corrected data bits, the first bit highest, bytes in memory order (the word ring's rule), the rest 0
 *     word 5-6  the 38 psyn bits likewise
 *     word 7    locked after the step, as int32
 * n_frames and n_bad are the reference's packets and packets_bad, which its quality_check reads.
 * Lost: hits that left the hit ring before they were examined are counted (n_lost); an accepted frame whose sync position's
 * word the word ring had overwritten when it was decided is counted (n_lost) and nothing else of its step applies.  After a
 * loss pos moves to the first retained hit at or behind it -- behind a lost frame: at or behind the oldest retained word --
 * if the block knows one, else (a lost frame) to the oldest retained word.
 * Departures.  The reference decides against whatever its string buffer holds -- more than 228 bits, one message more per
 * loop, all of it dropped when no sync word is in it -- so its output depends on how the stream arrives.  The stage equals
 * the reference with the whole stream in view, waits where the reference would see find() == -1, and has no 229-bit
 * minimum.  sync_loops, the retune (tune_next_control, which also zeroes locked) and the no-flow rule are control-plane policy
 * and stay with the consumer: one that retunes calls rcf_chan_osw again.  (No naming of cmd: dual, last_cmd, the type
 * table, the channel grants.)
 * p == NULL switches the stage off.  It applies from the next block on and considers only hits appended after the call (the
 * call reads the slicer's counters and so synchronises the stream); calling again starts it afresh, locked = 0 and a new
 * ring.  It goes when the slicer goes: slicer attached again or switched off, its source loop attached again or switched
 * off, channel closed.  A slicer carries at most one of the TSBK, EDACS and OSW stages: what it searches decides which.
 * RCF_ESTATE: the channel has no slicer in RCF_SLICE_BINARY mode that searches an 8-bit sync word with sync_max_errors = 0
 * and sync_both = 0; RCF_EINVAL: capacity not 0 or a power of two >= 16 (at most 2^20); RCF_ENOCHAN: no such channel. */
typedef struct rcf_osw_params {
    int capacity;          /* records of the ring, a power of two >= 16; 0 = 256 */
    int reserved_[3];
} rcf_osw_params_t;
int rcf_chan_osw(rcf_t *h, int chan_id, const rcf_osw_params_t *p);
/* the stage's counters as of the last block; syncs the stream.  RCF_ESTATE without the stage (here and in the calls below) */
typedef struct rcf_osw_state {
    int64_t n_records, n_frames, n_bad, n_rejects, n_lost;   /* records written, frames accepted (packets), of them with a nonzero syndrome (packets_bad), candidates rejected, hits and frames lost */
    int32_t locked, is_locked;                               /* the lock counter; is_locked as of the last accepted frame */
} rcf_osw_state_t;
int rcf_chan_osw_state(rcf_t *h, int chan_id, rcf_osw_state_t *out);
/* unread records, oldest first: out = uint32[max_records][8] (one round trip); RCF_HARD_OSW names the stream to
 * rcf_chan_read_many and rcf_group_read_many (out = uint32[n_chans][cap_each][8]); the pump delivers it
 * through rcf_pump_subscribe_hard */
#define RCF_HARD_OSW     51   /* (50 stays unassigned: the readers refuse it as an unknown stream) */
int64_t rcf_chan_read_osw(rcf_t *h, int chan_id, uint32_t *out, size_t max_records);
/* device pointer of the record ring and its capacity in records (zero-copy): record i lives at word 8 (i & (capacity - 1)) */
int rcf_chan_osw_ring(rcf_t *h, int chan_id, void **rec_ring, size_t *capacity);
/* P25 voice data units behind a slicer: what the reference's consumer does per frame of a voice channel in Python
 * (logging_receiver.py p25_sensor 381-473 and p25_control_demod.py 365-385: p25_general.procHDU / procLDU1 / procTLC /
 * subprocLC / procStatus, with the codecs of hamming.py, golay.py and rs64.py that stand beside p25_general's stubs), as one
 * more optional stage per channel on the GPU: the voice-channel counterpart of rcf_chan_tsbk.  It reads the slicer's own two
 * streams and writes a third, the counted stream RCF_HARD_P25LC of 32-byte records, one per frame: a consumer of a voice
 * channel takes NAC, DUID and the decoded link control instead of every word of the dibit stream.  All of it is integer
 * work: the records are exactly what the rules below give for the words and hits the slicer's readers deliver.  Optional,
 * through rcf_chan_p25lc_opt: LDU2's encryption sync (RCF_P25LC_ES) and inner words given up as erasures of the Reed-Solomon
 * decoder (RCF_P25LC_ERASURES); without an option every record is what the rules give without the paragraphs "LDU2" and
 * "Erasures".  BCH correction of the NID is rcf_chan_p25lc_ex's option RCF_NID_BCH, by the rule "The NID" at rcf_chan_tsbk_ex.
 * (No decoding of the LSD's (16,8,5) code, no IMBE.)
 * Frames.  Hits, the widening of k, the accept rule (k >= k_last_accepted + 24), the start at hit index >= the slicer's
 * n_hits at the call, the lost rule and "info dibit j sits at frame dibit r = j + j / 35" are rcf_chan_tsbk's.  The frame
 * starts at dibit s = k - 23; frame_dibits = min(864, s_next - s), s_next the frame start of the next accepted hit if there
 * is one by then.  An accepted hit is DECIDED in the first block with 16 n_words >= s + 888: the 864 dibits of an LDU and
 * the 24 of a sync word that may begin inside them -- so the records do not depend on how the input was cut into blocks.
 * NID: nac = info bits 48 .. 59, duid = info bits 60 .. 63 (info bit 0 is the sync word's first bit), uncorrected unless the
 * stage was attached with RCF_NID_BCH: then they are the decoded ones, and the decoded duid names the unit.
 * Units.  A unit is decoded only if its last needed frame dibit lies inside the frame (r < frame_dibits):
 *     duid 0x0  HDU   36 words of 18 bits, word w = info bits 112 + 18 w .. + 17; last dibit 389; inner code shortened Golay
 *                     (18,6,8), outer code RS(36,20,17); payload 20 hexbits = 15 octets (MI 72, MFID 8, ALGID 8, KID 16, TGID 16)
 *     duid 0x5  LDU1  24 words of 10 bits, word w = info bits 112 + B[w / 4] + 10 (w % 4) .. + 9, B = (288, 472, 656, 840,
 *                     1024, 1208) (procLDU1's slices); inner code Hamming (10,6,3), outer code RS(24,12,13); payload the
 *                     hexbits 0 .. 11 = 9 octets; the 32 raw LSD bits are info bits 1504 .. 1535; last dibit 788
 *     duid 0xF  TLC   12 words of 24 bits, word w = info bits 112 + 24 w .. + 23; last dibit 204; inner code extended Golay
 *                     (24,12,8), two hexbits per word, outer code RS(24,12,13); payload 9 octets
 * Every other duid (3, 7, 0xA -- LDU2, whose duid the consumer's activity rule needs --, 0xC, unknown) and a decodable duid
 * whose frame is too short gives a frame record without payload.
 * Modes.  correct = 0: p25_general's own reading, bit for bit: the payload is the first 6 (12 for the (24,12) words) bits of
 * every inner word, then the first 72 (HDU: 120) of those bits; nothing is corrected and all counts are 0.  correct = 1: the
 * decoders below.
 * Hamming (10,6,3), the first bit highest: the syndrome's four bits are the parities of the word under 0b1110011000,
 * 0b1101010100, 0b1011100010, 0b0111100001.  Syndrome 0: the word is good.  Syndrome equal to entry i of (1110, 1101, 1011,
 * 0111, 0011, 1100, 1000, 0100, 0010, 0001): bit i counted from the first is flipped and the word counts as FIXED.
 * Anything else: the word counts as BAD and its data bits are taken as read.
 * Golay, generator 0xC75: the result is the 12 data bits (the first 12) of the (23,12,7) code word nearest to the word's
 * first 23 bits -- unique and at most 3 bits away, the code being perfect; the 24th bit takes no part (golay.py searches on
 * msg >> 1).  The word counts as FIXED if any of the 23 bits changed.  An (18,6) word is extended by six leading zero data
 * bits; if the nearest code word's six leading data bits are not all zero the word counts as BAD and its data are taken as
 * read.  This decoder is complete; the reference's error-trapping search returns None on about half a percent of the
 * patterns of up to three errors.
 * RS(n, k, d) over GF(64), primitive polynomial x^6 + x + 1, alpha = 2, generator roots alpha^1 .. alpha^(d - 1), symbols
 * in the order of rs64.py's msg (data first, parity behind: symbol i is the coefficient of x^(n - 1 - i)), t = (d - 1) / 2.
 * The result is the code word of the shortened code within t symbols of the inner-decoded word if there is one -- it is
 * unique --, n_rs the number of symbols it changes; otherwise rs_bad is set, n_rs is 0 and the payload is the inner-decoded
 * data symbols as they stand.  No erasures without RCF_P25LC_ERASURES.
 * LDU2 (RCF_P25LC_ES).  Duid 0xA with frame_dibits > 788 is a unit of kind 4: 24 words of 10 bits at the LDU1's positions,
 * inner code Hamming (10,6,3) as above, outer code RS(24,16,9), t = 4, in the field, root order and symbol order of the other
 * two; payload the hexbits 0 .. 15 = 12 octets (MI 72, ALGID 8, KID 16); the 32 raw LSD bits where the LDU1 has them.  It
 * counts in n_decoded and n_rs_bad.  correct = 0: the first 6 bits of every word, then the first 96 of those --
 * rs_24_16_9_decode(hamming_10_6_3_decode(lc)) of p25_general over procLDU1's slices (its procLDU2 is empty).
 * Erasures (RCF_P25LC_ERASURES, correct = 1; all four units).  The erased set E is the symbols of the inner words that count
 * as BAD: one symbol per Hamming or (18,6) word, both symbols of a (24,12) word.  So that a (24,12) word can be BAD, its 24th
 * bit takes part under this option only: if the nearest (23,12) code word is 3 bits away and the received 24th bit is not the
 * overall parity of that code word (golay.py's encode appends it), four errors are detected, the word counts as BAD and its
 * data are taken as read.  The result is the code word of the shortened code that agrees with the inner-decoded word outside E
 * in all but v symbols with 2 v + |E| <= d - 1 if there is one -- it is unique --, n_rs the number of symbols it changes,
 * erased ones included (up to 16); otherwise, or if |E| > d - 1, rs_bad is set, n_rs is 0 and the data stand.  |E| is n_bad,
 * 2 n_bad for a TLC.  rs64.py's decode with its `erasures` list answers None on many patterns inside this bound and is right
 * wherever it answers; this decoder is complete.
 * Records, 8 uint32 each, in increasing k:
 *     word 0    bits 0-1 and bit 3 kind (0 HDU, 1 LDU1, 2 TLC, 3 a frame record; bit 3: 4 LDU2, with RCF_P25LC_ES only),
 *               bit 2 rs_bad, bits 4-7 n_rs's low four bits and bit 8 its fifth (set with RCF_P25LC_ERASURES only), bit 9
 *               set with RCF_NID_BCH only, bits 10-15 the hit's distance, bits 16-19 duid, bits 20-31 nac (the last three where TSBK has them)
 *     word 1    the low 32 bits of the widened k
 *     word 2-5  the payload's octets, the first bit highest, bytes in memory order (the word ring's rule), zero padded; 0
 *               in a frame record
 *     word 6    the 32 raw LSD bits, same rule (LDU1, LDU2), else 0
 *     word 7    bits 0-15 frame_dibits, bits 16-21 inner words fixed, bits 22-27 inner words bad, bits 28-31 nid_fix (RCF_NID_BCH; else zero)
 * p == NULL switches the stage off.  It applies from the next block on and considers only hits appended after the call;
 * calling again starts it afresh.  It goes when the slicer goes: slicer attached again or switched off, its source loop
 * attached again or switched off, channel closed.  A slicer carries this stage or the TSBK stage, never both: each of the two
 * calls is refused while the other stage is attached.
 * RCF_ESTATE: the channel has no slicer in RCF_SLICE_FSK4 mode that searches a 48-bit sync word, that slicer searches both
 * polarities (sync_both = 1), or it carries the TSBK stage; RCF_EINVAL: capacity not 0 or a power of two >= 16 (at most
 * 2^20), correct not 0 or 1, an unknown option bit, RCF_P25LC_ERASURES with correct = 0; RCF_ENOCHAN: no such channel.
 * rcf_chan_p25lc(h, c, p) is rcf_chan_p25lc_opt(h, c, p, 0): one attach path, and calling either again starts the stage
 * afresh with the options of that call.  rcf_chan_p25lc_opt(h, c, p, o) in turn is rcf_chan_p25lc_ex(h, c, p, o, RCF_NID_RAW);
 * RCF_EINVAL as well: nid neither RCF_NID_RAW nor RCF_NID_BCH. */
typedef struct rcf_p25lc_params {
    int capacity;          /* records of the ring, a power of two >= 16; 0 = 256 */
    int correct;           /* 0: the reference's p25_general reading (systematic bits, nothing corrected); 1: the decoders above */
    int reserved_[2];
} rcf_p25lc_params_t;
int rcf_chan_p25lc(rcf_t *h, int chan_id, const rcf_p25lc_params_t *p);
#define RCF_P25LC_ES        1u   /* decode LDU2's encryption sync */
#define RCF_P25LC_ERASURES  2u   /* inner words given up become Reed-Solomon erasures (needs correct = 1) */
int rcf_chan_p25lc_opt(rcf_t *h, int chan_id, const rcf_p25lc_params_t *p, uint32_t options);
int rcf_chan_p25lc_ex(rcf_t *h, int chan_id, const rcf_p25lc_params_t *p, uint32_t options, uint32_t nid);
/* the stage's counters as of the last block; syncs the stream.  RCF_ESTATE without the stage (here and in the calls below) */
typedef struct rcf_p25lc_state {
    int64_t n_records, n_frames, n_decoded, n_rs_bad, n_lost;   /* records written, frames accepted (decided or lost), units decoded (HDU, LDU1, TLC), of them with rs_bad, hits and frames lost */
} rcf_p25lc_state_t;
int rcf_chan_p25lc_state(rcf_t *h, int chan_id, rcf_p25lc_state_t *out);
/* unread records, oldest first: out = uint32[max_records][8] (one round trip); RCF_HARD_P25LC names the stream to
 * rcf_chan_read_many and rcf_group_read_many (out = uint32[n_chans][cap_each][8]); the pump delivers it
 * through rcf_pump_subscribe_hard */
#define RCF_HARD_P25LC   53   /* (52 stays unassigned like 50: the readers refuse both as unknown streams) */
int64_t rcf_chan_read_p25lc(rcf_t *h, int chan_id, uint32_t *out, size_t max_records);
/* device pointer of the record ring and its capacity in records (zero-copy): record i lives at word 8 (i & (capacity - 1)) */
int rcf_chan_p25lc_ring(rcf_t *h, int chan_id, void **rec_ring, size_t *capacity);
/* drift probe of p25_control_demod.py:123-127: moving_average_ff(window, 1) * (1/window) of the
 * discriminator output (window = 10000 there) == mean of gain*fm over the last `window` samples; this is
 * the value demod_watcher hands to frontend_connector.report_offset */
int rcf_chan_fm_level(rcf_t *h, int chan_id, float gain, int window, float *level);
/* Analog NBFM voice chain behind a channel (logging_receiver.py:211-222, file_to_wav.py:109-122):
 *   analog.pwr_squelch_cc(db, alpha, 0, True)           gates (drops) samples while the smoothed power is low
 *   analog.fm_demod_cf(...) = quadrature_demod_cf(k) -> fm_deemph(rate, tau) -> fir_filter_fff(1, audio_taps)
 *   filter.fir_filter_fff(1, firdes.high_pass(...))
 *   filter.rational_resampler_fff(8000, rate)
 * The chain starts, with zero state, at the channel's next output.  The squelch and the de-emphasis IIR are
 * sequential per channel (one lane per channel walks the new samples); the FIRs and the resampler run one
 * thread per output.  Taps are the caller's (rcf/audio.py derives them as the reference's calls do). */
typedef struct rcf_audio_params {
    double squelch_db;        /* pwr_squelch_cc threshold, dB */
    double squelch_alpha;     /* its single-pole power filter */
    float quad_gain;          /* quadrature_demod_cf gain k = rate / (2 pi deviation) */
    int reserved_;
    double deemph_b[2];       /* iir_filter_ffd(btaps, ataps, False); {1,0},{1,0} = no de-emphasis */
    double deemph_a[2];
    const float *lpf_taps;    /* audio low-pass, fir_filter_fff(1, taps) */
    int n_lpf;
    int n_hpf;
    const float *hpf_taps;    /* 300 Hz high-pass */
    const float *rs_taps;     /* rational_resampler_base_fff(interpolation, decimation, taps) */
    int n_rs;
    int interpolation;
    int decimation;
    int reserved2_;
} rcf_audio_params_t;
int rcf_chan_audio_open(rcf_t *h, int chan_id, const rcf_audio_params_t *p);
int rcf_chan_audio_close(rcf_t *h, int chan_id);
/* audio samples (resampler outputs) produced so far / samples that passed the squelch (syncs the stream) */
int rcf_chan_audio_produced(rcf_t *h, int chan_id, int64_t *n_audio, int64_t *n_ungated);
/* unread audio samples, oldest first; returns the count or a negative error */
int64_t rcf_chan_read_audio(rcf_t *h, int chan_id, float *out, size_t max_samples);
/* device pointers of the channel's rings (cf32 iq ring, f32 unit-gain discriminator ring) and their
 * power-of-two capacity: sample k lives at index k & (capacity-1) */
int rcf_chan_rings(rcf_t *h, int chan_id, void **iq_ring, void **fm_ring, size_t *capacity);
/* receiver.source_offset folds demod-reported drift into the SDR centre frequency
 * (rc_frontend/receiver.py:436-475); here the same Hz shift is added to every channel's offset. */
int rcf_source_shift(rcf_t *h, double delta_hz);

/* The discriminator of EVERY bin, computed by the filterbank's own kernel (frame-major banks: 400 / 800 / 1600 / 3200 bins
 * at the reference's channel rule, rc_frontend/channel.py:31-35).  What analog.quadrature_demod_cf does behind each
 * channel's pub_sink (p25_control_demod.py:120-121) happens before the channel ever leaves the GPU:
 *     fm_k[n] = fast_atan2f(Im, Re of bin_k[n] conj(bin_k[n - 1]) x inc_k)          (gain 1; readers apply theirs)
 * into a frame-major ring fm_ring[((n - n0) & (capacity - 1)) n_bins + k] -- the arithmetic (and the bits) of a tap opened
 * with rcf_pfb_tap_open(bin, gr_phase) + rcf_chan_set_fm_only, without the tap matrix, the IQ round trip through HBM and
 * the tap_finalize pass: 8 + 8 bytes per input sample instead of 48 at 1600 bins / decimation 800.
 *   mode 1: beside the bins ring;  mode 2: INSTEAD of it -- rcf_pfb_read_bin, rcf_pfb_rings, rcf_pfb_chan_open and any other
 *   channel on a bin (rcf_chan_open_taps with src >= RCF_SRC_PFB_BIN0) then fail with RCF_ESTATE, and mode 2 itself is
 *   refused (RCF_ESTATE) while such a channel is open; taps (rcf_pfb_tap_open) keep working.  Leaving mode 2, readers of the
 *   bins ring go on from the frame of the switch;  mode 0: off again.  Takes effect with the next block.
 *   gr_phase != 0: inc_k = the float32 rotator increment GNU Radio's freq_xlating_fir_filter_ccc on bin k would carry
 *   (what rcf_pfb_tap_open(bin, 1) models); 0: the bank's exact phases (inc_k = 1).  rcf_source_shift is followed.
 * The first frame after enabling takes its predecessor from the input history (recomputed, not stored): the handle's
 * history capacity must hold (chunk + taps-per-branch x oversampling + 2) x decim + n_bins samples (RCF_ECAP otherwise). */
int rcf_pfb_fm_enable(rcf_t *h, int mode, int gr_phase);
/* bin's discriminator samples not yet read by this call, x gain -> out; a reader more than the ring behind loses the oldest */
int64_t rcf_pfb_read_fm(rcf_t *h, int bin, float gain, float *out, size_t max_samples);
/* how many chunk hand-overs inside the bank's kernel never arrived (a bounded wait gave up: those frames were demodulated
 * against a zero predecessor).  0 on a healthy device: a check for tests and health probes, not a data path. */
int64_t rcf_pfb_fm_lost(rcf_t *h);
/* zero-copy: the device ring (floats), its capacity in frames and the relative index of its first valid frame; bin k of
 * relative frame i sits at fm_ring[(i & (capacity - 1)) n_bins + k].  Order reads on rcf_stream(h) after rcf_sync / an event. */
int rcf_pfb_fm_ring(rcf_t *h, void **fm_ring, size_t *capacity_frames, int64_t *first_frame);

/* ------------------------------------------------------------------ carrier detect (scanning_receiver.py) */
/*
 * The reference's conventional-channel ("scanner") system type hangs analog.simple_squelch_cc(system['threshold'], 0.1)
 * behind a 12.5 kHz channel, polls squelch.unmuted() every 10 ms and calls call_progress(freq), which opens or keeps
 * alive a logging_receiver (scanning_receiver.py:53,108-113).  Here that block is one more optional stage behind a
 * channel, and -- what a flowgraph per frequency cannot do -- a stage on EVERY bin of an open filterbank at once: a
 * band-wide activity map at block latency.  It reports and gates nothing: the IQ stream passes unchanged.
 * The definition restates GNU Radio 3.8's simple_squelch_cc_impl (unpinned against GNU Radio's own build, like the symbol
 * loops):
 *      thr   = pow(10.0, threshold_db / 10)
 *      p     = (float)(re * re + im * im)          float products, float sum, not contracted; then widened to double
 *      level = alpha * p + (1 - alpha) * level     filter::single_pole_iir<double,double,double>: double, level 0 at the start
 *      open  = level >= thr                        per sample; `unmuted` is that comparison for the last sample seen
 * A NaN level reads as muted and stays NaN; an Inf level stays open (with alpha == 1 the next sample turns it into a
 * NaN: 0 x Inf, as in GNU Radio).  The call that attached the stage resets it.
 * Limits: no ramp (simple_squelch_cc has none), and this stage reports only (the reference connects the
 * block to a null sink and reads unmuted() only): gating the IQ stream is rcf_chan_capture's, below.
 *
 * Behind a channel: exact, bit for bit the sequential evaluation above, however the stream is cut into blocks.  p == NULL
 * detaches the stage; calling it again resets the state (level 0, counters 0) from the channel's next output on.  It
 * reads the channel's IQ ring over each block's new samples, so it serves every channel kind (direct, chained, stage 2 on
 * a bin, filterbank tap) on one front-end and in a group; a retune keeps it, closing the channel releases it.
 * RCF_EINVAL: alpha outside (0, 1] or a threshold that is not finite; RCF_ENOCHAN: no such channel; RCF_ESTATE: the
 * channel exposes its discriminator only (rcf_chan_set_fm_only: no IQ ring) -- and rcf_chan_set_fm_only(on) is refused
 * (RCF_ESTATE) while the channel carries the stage. */
typedef struct rcf_squelch_params {
    double threshold_db;        /* simple_squelch_cc's threshold, dB */
    double alpha;               /* its filter's alpha, (0, 1]; the reference uses 0.1 */
} rcf_squelch_params_t;
int rcf_chan_squelch(rcf_t *h, int chan_id, const rcf_squelch_params_t *p);
/* the stage's state as of everything queued; syncs the stream.  Indices count the channel's outputs (sample k is the k-th
 * sample rcf_chan_read_iq ever delivers to a reader that keeps up); -1: none.  RCF_ESTATE without the stage. */
typedef struct rcf_squelch_state {
    double level;               /* the filter's output after the last sample seen */
    int64_t n_seen, n_open;     /* samples seen / of them open, since the stage was (last) attached */
    int64_t first_open, last_open;      /* index of the first / the last open sample since then */
    int32_t unmuted;            /* the last sample seen was open */
    int32_t reserved_;
} rcf_squelch_state_t;
int rcf_chan_squelch_state(rcf_t *h, int chan_id, rcf_squelch_state_t *out);
/* The same stage on every bin of the open filterbank, over each block's new frames of the bins ring (either layout: every
 * shape rcf_pfb_open accepts).  n == n_bins: one threshold per bin; n == 1: one for all; threshold_db == NULL: off (the
 * last state stays readable).  Takes effect with the next block; calling it again resets every bin.
 * The recurrence is cut in time -- segments of rcf_pfb_squelch_segment() frames, each first walked from level 0, then
 * entered at the level the segments before it leave, carried across a segment by pow(1 - alpha, segment) -- which is exact
 * up to rounding: a bin's level differs from the sequential evaluation by at most 64 x 2^-53 / alpha, relative (both add
 * positive terms, commit two roundings of 2^-53 per step and forget them at rate alpha; the factor covers both and the one
 * pow and one product per segment).  n_open, last_open and the mask are those of the sequential evaluation wherever no
 * sample's level lies within that distance of its threshold.
 * RCF_ESTATE: no filterbank open, or the bank writes its discriminator ring only (rcf_pfb_fm_enable mode 2: no bins to
 * read) -- and mode 2 is refused (RCF_ESTATE) while the stage is on, as it is while a channel reads a bin; mode 1 is
 * fine.  RCF_EINVAL: n neither 1 nor n_bins, alpha outside (0, 1], a threshold that is not finite. */
int rcf_pfb_squelch(rcf_t *h, const double *threshold_db, int n, double alpha);
/* per bin: the level after the last frame, the open frames and the last open frame (index since rcf_pfb_open, as
 * rcf_pfb_read_bin counts; -1: none) since the stage was (last) switched on, and whether the last frame was open (bin k:
 * word k / 32, bit k % 32 of unmuted_mask, (n_bins + 31) / 32 words); *frames_seen: frames walked since then.  Any array
 * may be NULL; n_bins must be the bank's (RCF_EINVAL).  Syncs the stream.  RCF_ESTATE: no bank, or the stage never on. */
int rcf_pfb_squelch_read(rcf_t *h, double *level, int64_t *n_open, int64_t *last_open, uint32_t *unmuted_mask, int n_bins,
                         int64_t *frames_seen);
/* frames per segment of the bank's stage (no device needed) */
int rcf_pfb_squelch_segment(void);

/* ------------------------------------------------------------------ carrier-operated capture */
/*
 * The reference does not stop at the report: scanning_receiver.py:108-113 polls unmuted() every 10 ms, call_progress
 * (:62-97) opens a logging_receiver on that frequency, and the receiver stays alive hang_time = 0.5 s behind the last
 * activity.  What it records has lost the head of the transmission (the poll period plus the connect at least).  Here the
 * gate itself is one more optional stage behind a channel, independent of rcf_chan_squelch (a channel may carry either or
 * both): it turns the channel's IQ stream into the samples of its transmissions only, with a lead-in the reference cannot
 * have, a hang time counted in samples, and a record per transmission.
 *
 * Definition.  Let a be the channel-output index of the first sample after the attaching call (indices as
 * rcf_squelch_state_t counts them).
 *   Detector: exactly rcf_chan_squelch's -- thr = pow(10, threshold_db / 10), p = (float)(re re + im im),
 *     level = alpha p + (1 - alpha) level in double from level 0 at a, open(i) <=> level_i >= thr; a NaN level is muted for
 *     good, an Inf level stays open.
 *   Gate: with integers pre >= 0 and hang >= 0 in channel samples, sample j >= a is KEPT <=> some i >= a has open(i) and
 *     j - hang <= i <= j + pre.  With L(n) the greatest open index <= n (or none): keep(j) <=> L(j + pre) >= j - hang.  So the
 *     writer runs pre samples behind the detector and needs only L at the detector's position: O(1) per sample and exact,
 *     however the stream is cut into blocks.  After n_seen samples the stage has DECIDED samples a .. a + n_seen - pre - 1;
 *     the last pre samples wait for the next block.  Nothing before a is ever kept: the lead-in is clipped at the attach
 *     point.
 *   Captured stream (RCF_READ_CAPTURE: cf32, counted on the device): the kept samples in order, bits unchanged, compacted
 *     into a ring of `capacity` samples the stage owns.
 *   Records (RCF_HARD_CAPTURE: rcf_capture_rec_t, 32 bytes, counted on the device, a ring of rec_capacity records): an OPEN
 *     record at every j with keep(j) && !(j > a && keep(j - 1)), a CLOSE record at every j with !keep(j) && keep(j - 1).
 *     OPEN: sample = the first kept sample, pos = its index in the captured stream, n_open = 0, peak = 0.  CLOSE: sample =
 *     the first sample not kept, pos = one past the window's last captured sample, n_open = the open samples of the
 *     window (saturating), peak = (float) of the largest level at one of them.  The two CLOSE accumulators count from the
 *     last CLOSE on, which is exact: keep(j) is false at a CLOSE, so no index in [j - hang, j + pre] is open -- every open
 *     sample the detector has seen by then lies inside the window that just ended (or one before it, whose CLOSE took it
 *     out).  Records alternate OPEN, CLOSE, OPEN, ... and start with OPEN; close.pos - open.pos == close.sample -
 *     open.sample; every open sample lies in exactly one window.
 * p == NULL detaches the stage.  Calling it again resets everything and restarts both streams at item 0, from the channel's
 * next output on.  It reads the channel's IQ ring, so it serves every channel kind on one front-end and in a group; a retune
 * keeps it, closing the channel releases it.
 * capacity and rec_capacity are rounded up to powers of two; 0: the handle's ring capacity / 256 records; capacity is at
 * least 64, rec_capacity at least 16 (smaller values are raised).
 * RCF_EINVAL: alpha outside (0, 1], a threshold that is not finite, pre or hang negative, a capacity beyond 2^26 samples or
 * 2^20 records.  RCF_ECAP: the writer re-reads the channel's IQ ring pre samples behind the detector, so pre plus the most
 * outputs one block can give the channel must fit that ring: with N the handle's block capacity and the channel's chain of
 * decimations D_1 .. D_m (the filterbank's first for a channel on a bin), M_0 = N, M_i = M_(i-1) / D_i + 1 (integer
 * division), the call is refused when pre + M_m exceeds the ring capacity.  (A block that would still overrun the ring is
 * refused when it is pushed, as for every stage that looks back.)  RCF_ESTATE: the channel exposes its discriminator only
 * (rcf_chan_set_fm_only) -- and rcf_chan_set_fm_only(on) is refused (RCF_ESTATE) while the channel carries the stage.
 * RCF_ENOCHAN: no such channel.
 * A reader of either stream that lags more than its ring loses the oldest items, like every counted stream. */
/* (enumerators, not macros: the RCF_READ_* macros are the rows of the stream table proper -- what rcf_pump_start takes, and a list
 * the suite pins --, and these two streams stand behind that table, with the readers' rows) */
enum {
    RCF_READ_CAPTURE = 24,    /* cf32 samples of rcf_chan_capture's captured stream */
    RCF_HARD_CAPTURE = 56     /* its 32-byte records */
};
#define RCF_CAPTURE_OPEN  1
#define RCF_CAPTURE_CLOSE 2
typedef struct rcf_capture_params {
    double threshold_db;        /* the detector's threshold, dB */
    double alpha;               /* its filter's alpha, (0, 1]; the reference uses 0.1 */
    int64_t pre;                /* lead-in, channel samples */
    int64_t hang;               /* hang time, channel samples */
    uint32_t capacity;          /* captured-stream ring, samples; 0: the handle's ring capacity */
    uint32_t rec_capacity;      /* record ring, records; 0: 256 */
} rcf_capture_params_t;
typedef struct rcf_capture_rec {
    uint32_t kind;              /* RCF_CAPTURE_OPEN / RCF_CAPTURE_CLOSE */
    uint32_t n_open;
    int64_t sample;
    int64_t pos;
    float peak;
    uint32_t reserved_;         /* 0 */
} rcf_capture_rec_t;
int rcf_chan_capture(rcf_t *h, int chan_id, const rcf_capture_params_t *p);
/* the stage's state as of everything queued; syncs the stream.  RCF_ESTATE without the stage. */
typedef struct rcf_capture_state {
    double level;               /* the detector's level after the last sample seen */
    int64_t n_seen;             /* samples the detector has seen since the stage was (last) attached */
    int64_t n_decided;          /* samples decided: max(0, n_seen - pre) */
    int64_t n_kept;             /* items of the captured stream so far */
    int64_t n_records;          /* items of the record stream so far */
    int64_t n_windows;          /* OPEN records among them */
    int64_t last_open;          /* index of the last open sample, -1: none */
    int32_t in_window;          /* the last decided sample was kept: an OPEN without its CLOSE */
    int32_t unmuted;            /* the last sample seen was open */
} rcf_capture_state_t;
int rcf_chan_capture_state(rcf_t *h, int chan_id, rcf_capture_state_t *out);
/* unread captured samples, oldest first: out = cf32[max_samples] (one round trip) */
int64_t rcf_chan_read_capture(rcf_t *h, int chan_id, float *out, size_t max_samples);
/* unread records, oldest first: out = rcf_capture_rec_t[max_records] as uint32[max_records][8] */
int64_t rcf_chan_read_capture_rec(rcf_t *h, int chan_id, uint32_t *out, size_t max_records);
/* zero-copy: the two device rings and their capacities in items (order reads on rcf_stream(h)) */
int rcf_chan_capture_rings(rcf_t *h, int chan_id, void **cap_ring, size_t *capacity, void **rec_ring, size_t *rec_capacity);


/* ------------------------------------------------------------------ polyphase filterbank */
/*
 * n_bins-channel PFB with prototype `taps` and decimation `decim` (n_bins % decim == 0): bin k is
 * exactly freq_xlating_fir_filter_ccc(decim, taps, k*fs/n_bins, fs) evaluated with exact phases
 * (SURVEY.md 7.2); it is the throughput path for on-grid channels and replaces the dead
 * pfb.channelizer_ccf branch of rc_frontend/receiver.py:242-261.  Output: n_bins streams at fs/decim.
 * Supported shapes (anything else: RCF_EINVAL):
 *   n_bins in {64, 128, 256, 512, 1024}, n_bins / decim in {1, 2}, up to 16 taps per branch
 *   n_bins in {400, 800, 1600, 3200},    n_bins / decim = 1 with up to 4 taps per branch, 2 with up to 2, 4 with 1
 *   n_bins in {160, 192, 480, 640, 960, 1280}, n_bins / decim = 2 with up to 2 taps per branch
 * (rcf_pfb_shape_family tells which of the three a shape belongs to.)
 * The second and third families are what makes the bins the REFERENCE's channels: with the reference's own channel filter
 * (rcf_channel_params: decim = int(fs/cr)/2, low_pass_2(1, fs, cr/2, cr/2, 20, HAMMING)) at fs = 20 Msps,
 * cr = 12.5 kHz -- decim 800, 2909 taps -- a 1600-bin bank is every 12.5 kHz-grid channel and a 3200-bin bank every
 * 6.25 kHz-grid channel rc_frontend/channel.py:31-35 could build, at the same 25 kS/s (10 Msps: 800 bins,
 * 5 Msps: 400).  The third family is the same rule at the rates the reference is deployed at -- 2, 2.4, 6, 8, 12 and
 * 16 Msps on the 12.5 kHz grid (2.4 Msps: 192 bins, decim 96, 349 taps).  Its banks have bins, taps, stage-2 channels and
 * rcf_pfb_read_bin like the second family's; rcf_pfb_fm_enable does NOT cover them (RCF_EINVAL: no fused-discriminator
 * kernel for these shapes).
 */
int rcf_pfb_open(rcf_t *h, int n_bins, int decim, const float *taps, int ntaps);
int rcf_pfb_close(rcf_t *h);
int64_t rcf_pfb_produced(rcf_t *h);
/* bin index in [0, n_bins): bin k is centred at k*fs/n_bins for k < n_bins/2, (k-n_bins)*fs/n_bins above */
int64_t rcf_pfb_read_bin(rcf_t *h, int bin, float *out_interleaved, size_t max_samples);
/* device layout of the bin outputs (complex samples; i = n & (capacity-1), n = frame index since rcf_pfb_open).
 * Power-of-two banks: tiles of 16 frames, sample n of bin k at bins_ring[(i >> 4) * tile_pitch + 16 * k + (i & 15)]
 * with tile_pitch = 16 * n_bins + 80 (a chunk of 16 frames is one contiguous run for the kernel that writes it, a bin's
 * 16 frames are one 128-byte line for whoever reads it; the padding keeps one bin's lines off a single memory channel),
 * and *pitch = 16 (frames per tile).  All other banks (400 2^k bins and the 160 .. 1280-bin family): ONE ring of whole frames, sample n of bin k at
 * bins_ring[i * n_bins + k], and *pitch = 0. */
int rcf_pfb_rings(rcf_t *h, void **bins_ring, size_t *capacity, size_t *pitch);
/* stage 2 on one bin: channel.py's own rule at the bin rate -- decim2 = int(bin_rate/cr)/2,
 * low_pass_2(1.0, bin_rate, cr/2, cr/2, 20, HAMMING), xlating by delta_hz -- output as a normal
 * channel id (read_iq / read_fm). */
#define RCF_SRC_PFB_BIN0 0x40000000
int rcf_pfb_chan_open(rcf_t *h, int bin, int channel_rate, double delta_hz, int *chan_id);
/* One bin AS a channel: when the bank was opened with the reference's own channel filter (rcf_channel_params
 * decimation and prototype), bin k already is channel.channel(.., channel_rate, samp_rate, k*fs/n_bins)
 * (rc_frontend/channel.py:31-35) -- the tap copies its new frames into a normal channel id (read_iq / read_fm /
 * audio / symbol filter all work), discriminator fused into the copy.  This is what the reference's dead
 * connect_channel_pfb (rc_frontend/receiver.py:343-383) was meant to do, without its second filter stage.
 * gr_phase != 0: the channel's rotator also carries the per-output phase and magnitude increment by which GNU
 * Radio's float32 rotator differs from the bank's exact phases, so the discriminator DC matches the reference's, and
 * starts at the phase GNU Radio's rotator has at a channel's first output (1, where the bin carries
 * e^{-j 2 pi k decim n0 / n_bins} at the frame n0 it is opened at): the IQ stream is that of a
 * freq_xlating_fir_filter_ccc started at the opening sample -- except that the bin comes with the filter's history
 * in it, where a new flowgraph starts from zeros. */
int rcf_pfb_tap_open(rcf_t *h, int bin, int gr_phase, int *chan_id);
/* A tap that is only ever demodulated: tap_finalize then writes its discriminator ring alone -- 4 instead of 12 bytes
 * per output; with every bin of the 1600-bin reference grid demodulated (rc_frontend/channel.py:35 +
 * p25_control_demod.py:120-121: every channel of the reference IS demodulated, in a process of its own) the finalize
 * launch moves 0.8 GB instead of 1.34 per 2^25-sample block.  The channel's IQ stream is then not available:
 * rcf_chan_read_iq / rcf_chan_read_many(RCF_READ_IQ) / rcf_chan_rings(iq) / chaining a channel or a voice chain on it
 * fail with RCF_ESTATE, and switching it on is refused (RCF_ESTATE) while something reads that stream.  on = 0 gives the
 * stream back from the next block on (the IQ read cursor skips what was never written).  Frame-major filterbank taps
 * only (RCF_EINVAL otherwise).  The discriminator path then rotates nothing either: arg(y[n] conj(y[n-1])) of the rotated
 * stream is arg(bin[n] conj(bin[n-1]) x incr) -- equal to an ordinary tap's discriminator to float32 rounding (~1e-7 rad),
 * bit-identical however the stream is cut, continuous across a switch in mid-stream (the call converts the one ring
 * sample the next block's first discriminator output is taken against; it synchronises the stream for that). */
int rcf_chan_set_fm_only(rcf_t *h, int chan_id, int on);
/* How far bin `bin` of an exact-phase bank is from GNU Radio's own channel at that offset, before any sample is seen
 * (no device needed).  freq_xlating_fir_filter_ccc (rc_frontend/channel.py:35) builds its composite taps as
 * h[i] e^{j float32(i * fwT0)}; the float32 product is rounded to 2.4-9.8e-4 rad at |offset| -> fs/2,
 * the bank's tap phases 2 pi k i / n_bins are exact.  The difference is a constant rotation (*const_phase, radians:
 * rcf_pfb_tap_open(gr_phase) puts it into the tap's rotator) plus an error filter g[i] = h[i] (e^{j (d[i] - const)} - 1)
 * whose output -- leakage of the whole wideband input, white input power P giving P * leak_l2^2 -- is what a bin tap
 * cannot reproduce.  rcf/receiver.py routes a request to the direct kernel (rcf_chan_open, GNU Radio's float32 phases
 * tap for tap) when the predicted discriminator error gain * leak_l2 * sqrt(P_wideband / P_carrier) exceeds its budget. */
int rcf_pfb_tap_leakage(double samp_rate, int n_bins, const float *taps, int ntaps, int bin, double *leak_l2,
                        double *const_phase);
/* 1 when rcf_pfb_open would accept this shape (no device needed) */
int rcf_pfb_shape_supported(int n_bins, int decim, int ntaps);
/* which kernel family rcf_pfb_open would run this shape on (no device needed): 0 none (the shape is not supported),
 * 1 power-of-two bin counts, 2 400 2^k bins, 3 the mixed-radix family {160, 192, 480, 640, 960, 1280} */
int rcf_pfb_shape_family(int n_bins, int decim, int ntaps);

/* ------------------------------------------------------------------ scan (fft_vector.py + fft_peak_detection.py) */
/*
 * fft_vector.py:37-60: stream_to_vector(fft_len) -> fft_vcc(fft_len, forward, blackmanharris, shift)
 * -> complex_to_mag_squared -> nlog10_ff(1, fft_len, 1) -> moving_average_ff(avg_len, 1, ..) ->
 * head(n_frames) -> skiphead(n_frames-1): one float32[fft_len] vector.
 * rcf_scan_start arms the scanner at the next ingested sample; the following pushes/commits feed it;
 * rcf_scan_result returns RCF_EAGAIN until n_frames frames have been consumed, then copies the
 * vector (the content of /tmp/fft_source_<i>) to the host.  fft_len: power of two, 256 .. 1<<20.
 */
int rcf_scan_start(rcf_t *h, int fft_len, int n_frames, int avg_len);
int rcf_scan_result(rcf_t *h, float *out_spectrum);
int rcf_scan_frames_done(rcf_t *h);
/* device pointer of the finished spectrum (float32[fft_len]); valid until the next rcf_scan_start */
int rcf_scan_result_device(rcf_t *h, void **dev_spectrum);
/*
 * fft_peak_detection.py:54-72 on a float32 spectrum of n bins: data += |min(data)|; mean (sequential
 * float64); scipy.signal.find_peaks(data, width=[min_w,max_w], prominence=prominence); keep
 * data[line] > 2*mean.  Writes the surviving `line` indices in ascending order (at most cap) and
 * returns how many survived in *count (may exceed cap).  Host arithmetic in float64, bit-exact with
 * scipy.  spectrum is a HOST pointer.
 */
int rcf_find_peaks(const float *spectrum, int64_t n, double min_w, double max_w, double prominence,
                   int64_t *idx, int64_t cap, int64_t *count, double *mean_out);
/* fft_peak_detection.py:72: frequency = int(line*hz_per_bin - bandwidth/2 + center_freq) */
int64_t rcf_peak_frequency(int64_t line, double samp_rate, int64_t fft_len, double center_freq);
/* same detection run on the device-resident result of the last scan (HIP kernels: local maxima,
 * block-skipping prominence/width walks); indices land in a device int64 buffer and are also copied to
 * idx (host) when idx != NULL.  At most min(cap, 4096) indices are kept (the device sort's size); *count
 * still reports how many survived. */
int rcf_scan_find_peaks(rcf_t *h, double prominence, int64_t *idx, int64_t cap, int64_t *count,
                        double *mean_out, void **dev_idx);

/* ------------------------------------------------------------------ multi-GPU: peak-list exchange */
/*
 * One process (one rcf_t) per GPU, one SDR front-end / spectrum slice each -- the reference already runs one
 * channelizer process per SDR (systemd/radiocapture-channelizer@.service, rc_frontend/receiver.py:67-70) and the
 * only thing its fft_based_scan.sh instances have in common is the list of detected frequencies.  These calls
 * give every rank the lists of all ranks with ONE ncclAllGather over xGMI (librccl, loaded on first use):
 *   rank 0: rcf_comm_unique_id(id) -> the host passes the 128 bytes to the other ranks (any transport)
 *   every rank: rcf_comm_init(h, rank, n_ranks, id)      (ncclCommInitRank on the handle's device; collective)
 *   after a scan: rcf_allgather_peaks(h, mine, n, all, cap, counts): all[w * cap + i], i < counts[w], is rank w's
 *   i-th value (at most cap per rank are exchanged; fixed records, 8 (cap + 1) bytes per rank -- latency-bound).
 * Without rcf_comm_init (or with n_ranks = 1 and id128 = NULL) the gather is a local copy; n_ranks = 1 WITH an id
 * builds a real one-rank communicator (same RCCL calls, one GPU).  rcf_allreduce_max is the barrier +
 * max-over-ranks the benchmark needs (syncs the handle's stream, then one ncclAllReduce on a double).
 */
int rcf_comm_unique_id(void *id128);
int rcf_comm_init(rcf_t *h, int rank, int n_ranks, const void *id128);
int rcf_comm_destroy(rcf_t *h);
int rcf_comm_size(rcf_t *h);
int rcf_allgather_peaks(rcf_t *h, const int64_t *mine, int n, int64_t *all, int cap, int *counts);
int rcf_allreduce_max(rcf_t *h, double *value);

/* ------------------------------------------------------------------ groups of front-ends */
/*
 * The reference's receiver holds ALL configured SDR sources in one top block when no -i is given
 * (rc_frontend/receiver.py:67-70,170-204; ten sources per host in configs/config_denver_dev_den817.py:25-118).  A group
 * is that: G front-ends of one device whose blocks are processed by ONE launch per stage -- one conversion (wire format
 * -> cf32, the history tails dual-written on the way), one filterbank launch over the chunks of every member (members of
 * the same bank shape; the others follow one by one), one stage-2 FIR + discriminator launch per (decimation, taps)
 * class, one tap-finalize launch, one gather for the read -- instead of G of each.  A real-time block is a handful of
 * ~5 us kernels: launched per front-end, one MI355X is launch-bound at a few hundred front-ends; grouped, the PCIe link
 * is what bounds it.  Outputs are the same bits as the members run one by one (tests/test_gpu_group.py).
 *   - members must live on one device and have the same out_capacity; a handle belongs to at most one group; while it
 *     does, it runs on the group's stream (every single-handle call keeps working) and rcf_close() on it is refused.
 *   - a call processes any SUBSET of the members: n_samples[i] = 0 (or blocks[i] = NULL) skips member i this time --
 *     independent SDRs are not synchronised, a pump takes whichever blocks are complete.
 *   - rcf_group_push returns once the callers' buffers have been read; pinned buffers (rcf_host_alloc) are read in
 *     place across PCIe, pageable ones are staged by the runtime first.
 *   - on a planning failure (a ring too small, an exhausted arena) nothing is queued and no member has advanced.
 */
typedef struct rcf_group rcf_group_t;
int rcf_group_open(rcf_t *const *handles, int n, rcf_group_t **out);
/* the members stay open and go back to their own streams */
int rcf_group_close(rcf_group_t *g);
int rcf_group_size(rcf_group_t *g);
/* blocks[i]: n_samples[i] samples of member i in `fmt` (RCF_FMT_CF32 / U8 / S8 / S16; scale and offset as rcf_push_raw) */
int rcf_group_push(rcf_group_t *g, const void *const *blocks, const size_t *n_samples, int fmt, float scale, float offset);
/* rcf_commit for every member with n_samples[i] > 0: the data is already where rcf_ingest_ptr said */
int rcf_group_commit(rcf_group_t *g, const size_t *n_samples);
/* rcf_chan_read_many over channels of several members: entry j is channel chan_ids[j] of member members[j] */
int rcf_group_read_many(rcf_group_t *g, int what, const int *members, const int *chan_ids, int n, float gain, void *out,
                        size_t cap_each, int64_t *counts);
int rcf_group_sync(rcf_group_t *g);

/* ------------------------------------------------------------------ real-time pump (native thread) */
/*
 * What moves the samples in a channelizer process -- in the reference GNU Radio's scheduler threads, started by
 * receiver.start() (rc_frontend/receiver.py:271) and channel.start() (:336) -- as ONE native thread per group with no
 * interpreter in it: whenever blocks
 * of some members are complete it pushes them as one group block, gathers the new output of their subscribed channels
 * with one launch into per-channel HOST rings (pinned memory the gather kernel writes across PCIe -- no host copy), and
 * publishes the counts once the launch has finished.  Two group blocks are in flight at most: the next one is planned
 * and queued while the previous one runs.
 *   Sources are rings of whole blocks in pinned memory (rcf_host_alloc), ring_blocks[i] blocks of block_samples each:
 *   written[i] != NULL: *written[i] counts the blocks the producer (an SDR driver thread) has completed -- block k is
 *     taken from slot k % ring_blocks[i] once *written[i] > k;
 *   written == NULL or written[i] == NULL: paced by the wall clock -- block k of member i is complete at
 *     t0 + (k + 1) * block_samples / samp_rate + phase_s[i] (a recorded or synthetic stream replayed at its rate).
 *   Latency of a block = from that instant (or from the moment the pump saw the counter) to its outputs being in host
 *   memory; late = latency above one block period; overrun = the pump got to a block more than a period after it was due.
 */
typedef struct rcf_pump rcf_pump_t;
typedef struct rcf_pump_config {
    size_t block_samples;
    int fmt;                             /* RCF_FMT_* of the source rings */
    float scale, offset;
    double samp_rate;                    /* pacing rate (samples per second of every member) */
    const void *const *rings;            /* [group size] */
    const size_t *ring_blocks;           /* [group size] */
    const double *phase_s;               /* [group size] or NULL */
    const volatile uint64_t *const *written;   /* [group size] or NULL */
    int what;                            /* RCF_READ_IQ / FM / AGC / SYM .. AUDIO: what the subscribed channels deliver */
    float gain;                          /* RCF_READ_FM: quadrature_demod_cf gain */
    const int *read_members;             /* [n_read] subscribed channels: member index ... */
    const int *read_chans;               /* ... and channel id */
    int n_read;
    size_t out_ring_samples;             /* host ring per subscribed channel, rounded up to a power of two (0: 4096) */
    int64_t n_blocks;                    /* blocks per member, then the pump stops by itself (0: until rcf_pump_stop) */
    int64_t warm_blocks;                 /* first blocks of every member that the statistics do not judge */
    int max_batch;                       /* most members per group block (0: all that are ready) */
    int cpu;                             /* pin the thread to this CPU (-1: leave it to the scheduler) */
    double start_delay_s;                /* t0 = now + this */
    double batch_window_s;               /* a complete block waits up to this long for others to share its launches (0: none) */
    int rt_priority;                     /* > 0: the thread asks for SCHED_FIFO at this priority (needs CAP_SYS_NICE; refused: it runs as it is) */
    int spin_us;                         /* idle waits up to this long are spun instead of slept (a late wake-up is a late block) */
    int max_read;                        /* subscription slots (>= n_read; 0: n_read): room for rcf_pump_subscribe while it runs */
} rcf_pump_config_t;
typedef struct rcf_pump_stats {
    int64_t blocks_done;                 /* member blocks whose outputs are in host memory */
    int64_t blocks_judged, late, overruns;
    int64_t group_blocks;                /* launches of the group (batches) */
    int64_t max_batch;
    int64_t samples_out;                 /* output samples written to the host rings */
    double latency_ms_p50, latency_ms_p99, latency_ms_max;
    double host_plan_ms, host_wait_ms;   /* thread time spent planning + queueing / waiting for the device */
    double elapsed_s;
    double max_plan_ms, max_wait_ms;     /* the longest single planning + queueing of a group block / wait for the device */
    double max_sleep_overshoot_ms;       /* how much later than asked the thread ever came back from a sleep (host scheduling) */
    int64_t slow_plans, slow_waits, slow_sleeps;   /* judged region: plans > 5 ms, device waits > 5 ms, sleeps that overshot by > 2 ms */
    int rt_priority_granted;             /* 1 when the SCHED_FIFO request of rt_priority went through */
    int running;                         /* 0 once the thread has finished */
    int error;                           /* RCF_E* that stopped it (0: none) */
    /* WHY a wait or a wake-up was late (appended in round 6).  /proc/thread-self/schedstat's run_delay is the time the
     * thread was RUNNABLE but had no CPU: lateness that is run_delay is the host scheduler (other tenants' threads on the
     * CPUs this container may use -- it has a CFS quota, no CPUs of its own and no SCHED_FIFO), not the GPU or the link.
     * -1: /proc not readable. */
    int cpu;                             /* the CPU the thread is pinned to (-1: it floats over the process's mask) */
    double runq_ms_total;                /* run_delay over the judged region */
    double slow_wait_ms_total, runq_ms_in_slow_waits;    /* device waits > 5 ms: their summed length / the run_delay inside them */
    double slow_sleep_ms_total, runq_ms_in_slow_sleeps;  /* wake-ups > 2 ms late: their summed lateness / the run_delay inside them */
    int64_t involuntary_switches;        /* getrusage(RUSAGE_THREAD).ru_nivcsw over the judged region */
} rcf_pump_stats_t;
int rcf_pump_start(rcf_group_t *g, const rcf_pump_config_t *cfg, rcf_pump_t **out);
int rcf_pump_stats(rcf_pump_t *p, rcf_pump_stats_t *st);
/* samples of subscribed channel `entry` (index into read_members / read_chans) in its host ring so far */
int64_t rcf_pump_written(rcf_pump_t *p, int entry);
/* copies up to max_items new items (cf32 pairs or floats) from *cursor on; a reader that fell more than the ring behind
 * loses the oldest (as a PUB socket at its HWM does) */
int64_t rcf_pump_read(rcf_pump_t *p, int entry, int64_t *cursor, void *out, size_t max_items);
/* rcf_pump_read for n slots at once: slot entries[i] from cursors[i] on into out + i * cap_each * 8 bytes (cf32 pairs, or
 * floats in the first half of the row), counts[i] items (-1: no such slot).  Row i stays at out + i * cap_each * 8 bytes
 * whatever its slot delivers and holds at most cap_each * 8 / item_bytes items: cap_each of up to 8 bytes (a 4-byte stream
 * fills the first half of its row), cap_each / 4 of the 32-byte records of rcf_pump_subscribe_hard */
int rcf_pump_read_many(rcf_pump_t *p, const int *entries, int64_t *cursors, int n, void *out, size_t cap_each, int64_t *counts);
/* Channels come and go while a channelizer runs (rc_frontend/receiver.py:296-342 connect_channel builds and starts a
 * channel flowgraph under the running top block, :424-435 / :635-648 release and destroy it): a running pump takes a new
 * subscription -- channel chan_id of member `member`, delivered as `what` (RCF_READ_IQ, RCF_READ_FM x gain, or a stage's stream: below) from where
 * the channel's own reader stands (a channel nobody has read: its first output, as far as its device ring still holds
 * it) -- into a free slot.  Returns the slot (>= 0; use it as `entry` above) and in *cursor where in
 * the slot's item count the new stream begins; RCF_ECAP when all max_read slots are taken.
 *   what = RCF_READ_AGC (cf32) and RCF_READ_SYM .. RCF_READ_AUDIO (float32) deliver a stage's stream the same way.  The
 * soft symbols of a loop and the voice chain's audio (RCF_READ_CLOCK / COSTAS / FSK4 / AUDIO) are counted on the device,
 * and the pump never waits for it: while such a slot is subscribed IT owns the stream's cursor, on the device, starting
 * where the channel's own reader stood; the channel's host-side reader position is left alone (an rcf_chan_read_costas
 * beside the subscription reads the same symbols again).  A stage switched off under its subscription starves the slot, as
 * a closed channel does; attached again (a fresh ring, symbol 0) the slot goes on with symbol 0 of the new attachment,
 * appended to its item count without a gap.
 *   what = RCF_READ_CAPTURE (cf32) delivers the captured stream of rcf_chan_capture by the same rules: counted on the device,
 * the slot owns its cursor there; a channel without the stage starves the slot.  A gather takes at most n_k samples after a
 * block of n_k channel outputs: the writer decides as many samples as the detector saw, once it runs pre behind.
 * (rcf_pump_start does not take it: subscribe it.) */
int rcf_pump_subscribe(rcf_pump_t *p, int member, int chan_id, int what, float gain, int64_t *cursor);
/* chan_id = RCF_SRC_PFB_BIN0 + bin (here and in rcf_pump_config_t.read_chans) with what = RCF_READ_FM subscribes ONE BIN of the
 * member's fused discriminator ring (rcf_pfb_fm_enable: every bin of the bank demodulated inside its launch) instead of a
 * channel: delivered from the bank's next frame on, x gain -- quadrature_demod_cf behind the reference's channel at that
 * bin's frequency (p25_control_demod.py:120-121) without a tap, a tap matrix or a tap_finalize pass. */
/* Everything behind the slicer through the pump: `what` = RCF_HARD_BITS, RCF_HARD_SYNC (uint32 items), RCF_HARD_TSBK,
 * RCF_HARD_EDACS, RCF_HARD_OSW or RCF_HARD_P25LC (32-byte records); anything else is RCF_EINVAL, the plain and soft streams
 * stay with rcf_pump_subscribe (which, like rcf_pump_start, goes on refusing these six).  The slot comes out of the same
 * max_read slots and is used as any other entry: rcf_pump_unsubscribe, rcf_pump_written, rcf_pump_read and
 * rcf_pump_read_many count in items -- a word, a hit, a record.
 *   Ring geometry.  A slot is out_ring_samples (rounded up to a power of two) x 8 bytes whatever it delivers.  The host ring of
 * a hard slot holds R items: R = out_ring_samples for the 4-byte streams (half the slot, as a discriminator slot),
 * R = out_ring_samples / 4 for the records.  R < 16: RCF_ECAP.
 *   Rules.  These streams are counted on the device, so the slot owns a cursor there as a soft-symbol slot does: the stream
 * begins where the channel's single reader of that stream stands (rcf_chan_read_hard .. rcf_chan_read_p25lc; left alone
 * afterwards), or at the oldest item the stage's ring still holds if that has wrapped past it; a stage attached again -- and
 * a slicer attached again takes its decoder with it -- starts a new stream at its item 0, appended to the slot's item count
 * without a gap; a slot handed from one tenant to the next keeps counting, whatever the two tenants' item sizes.  A channel
 * that lacks the stage is no error: the slot starves until the stage is attached.
 *   Lag.  The pump reserves for every gather in flight (two at most) the most it may take: after a block of n_k channel
 * outputs ceil(n_k bps / 32) + 1 words, n_k + 1 hits, (n_k + 15) / 24 + 3 TSBK records, (n_k + 15) / 24 + 1 voice records,
 * (n_k + 31) / 288 + 1 EDACS records, (n_k + 31) / 76 + 1 OSWs -- each the framing rule's densest case; what a stage has
 * ready beyond it leaves with the next block -- and min(the stage's ring, R) for the first gather of a stream.  With
 * `bound` the larger of the two blocks' figures a reader loses nothing while it lags fewer than R - 2 bound items.
 * RCF_EINVAL as well: no such member or channel; RCF_ECAP as well: no free slot.
 *   what = RCF_HARD_CAPTURE delivers the records of rcf_chan_capture (32 bytes, R = out_ring_samples / 4) by the same rules;
 * its per-block bound is 2 (n_k / (pre + hang + 2)) + 4 records: an OPEN and its CLOSE lie at least pre + hang + 1 samples
 * apart, a CLOSE and the next OPEN at least 1, so two records cost pre + hang + 2 samples; the + 4 covers the span's two ends
 * and the one window per attachment whose lead-in is clipped. */
int rcf_pump_subscribe_hard(rcf_pump_t *p, int member, int chan_id, int what, int64_t *cursor);
/* frees the slot (its channel may already be closed) */
int rcf_pump_unsubscribe(rcf_pump_t *p, int entry);
/* stops the thread (if still running), waits for it, releases the pump */
int rcf_pump_stop(rcf_pump_t *p);

#ifdef __cplusplus
}
#endif
#endif /* RCF_H */
