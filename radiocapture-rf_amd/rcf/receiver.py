"""Drop-in for the in-process surface of /root/reference/rc_frontend/receiver.py (SURVEY 8(b) (1')).

Keeps: `connect_channel(channel_rate, freq) -> (block_id, port)`, `release_channel(block_id)`,
`source_offset(block_id, offset)`, attributes `channels`, `sources`, `realsources`, `access_lock`,
`last_channel_cleanup`, `channel_idle_timeout`, `scan_mode` -- same argument meaning and error
behaviour (exceptions signal failure; the protocol handler maps them to 'na').

Replaces: the GNU Radio top_block.  Each configured source owns one `native.Frontend` (an HBM-resident
wideband buffer on one MI355X); channels are slots in that front-end's batched HIP kernels instead of
per-channel flowgraphs fed by ZMQ copies of the whole stream (receiver.py:201-202, channel.py:29).
`feed(source_id, iq)` is where an SDR driver / replay file / synthetic generator delivers samples.
"""
from __future__ import annotations

import logging
import random
import threading
import math
import time
import uuid

from . import channel as channel_mod


class receiver:
    def __init__(self, config, index=None, frontend_factory=None, device=0):
        """config: an object shaped like the reference's `rc_config` (configs/*.py): `.sources` dict of
        {type, center_freq, samp_rate, ...}, `.frontend_mode`, optional `.scan_mode`.
        index: as `receiver.py -i <index>`: keep only that source (receiver.py:67-70).
        frontend_factory(samp_rate, center_freq, device) -> native.Frontend-like (tests inject a stub)."""
        self.log = logging.getLogger("frontend" if index is None else "frontend-%s" % index)
        self.access_lock = threading.RLock()
        self.access_lock.acquire()
        self.config = config
        self.channel_idle_timeout = 10                     # receiver.py:51
        self.last_channel_cleanup = time.time()
        self.scan_mode = bool(getattr(config, "scan_mode", False))
        self.bind_port = None                              # set by the egress pump: port -> bound?
        self.release_port = None                           # set by the egress pump: close what bind_port(port) bound
        self.fault = None                                  # first data-plane failure (GPU / driver error): healthy() -> False
        self._fed = {}                                     # source_id -> samples delivered
        self._fed_t0 = time.time()
        self._fed_mark = (self._fed_t0, 0)
        if frontend_factory is None:
            from . import native

            def frontend_factory(samp_rate, center_freq, device):
                return native.Frontend(samp_rate, center_freq, device=device)
        self.realsources = dict(config.sources)
        if index is not None:                              # receiver.py:67-70
            index = int(index)
            self.realsources = {index: config.sources[index]}
        self.sources = {}
        numsources = 0
        for source in sorted(self.realsources):
            src = self.realsources[source]
            fe = frontend_factory(float(src["samp_rate"]), float(src["center_freq"]), device)
            # The channels of a receiver iterate GNU Radio's own float32 rotator (rcf_set_rotator): the IQ egress then
            # carries GNU Radio's phase at any stream length, for ~30 ns per output and channel per block -- under 1 %
            # of a block at real-time rates, which is what a receiver runs at.  config.rotator = 'fast' selects the
            # closed form instead (the C ABI's own default, what bench.py measures at 10^4 x real time; the
            # discriminator cannot tell the two apart, the IQ stream differs by a slowly turning common phase).
            if getattr(config, "rotator", "exact") == "exact" and hasattr(fe, "set_rotator"):
                fe.set_rotator(True)
            # config.py2_decim = True: decim = int(fs/cr) // 2, the Python-2 reading of channel.py:31 that the author's
            # 10 666 666 sps deployment ran (configs/config_denver_massive_p25.py:20,31 with receiver_split2 = False);
            # default: such a request is refused, as GNU Radio refuses the 426.5 Python 3 hands it
            if getattr(config, "py2_decim", False) and hasattr(fe, "set_decim_rule"):
                fe.set_decim_rule(1)
            if getattr(config, "receiver_split2", False):
                # receiver.py:205-237: each source becomes two half-rate sources, centre -/+ fs/4, through
                # freq_xlating_fir_filter_ccc(2, firdes.low_pass(1, fs, fs/4, fs/8), -/+fs/4, fs).
                # firdes.low_pass(...) == low_pass_2(..., 53 dB, HAMMING): same body, and compute_ntaps uses
                # window::max_attenuation(HAMMING) = 53 where low_pass_2 takes the attenuation argument.
                from . import native
                fs = float(src["samp_rate"])
                taps = native.design_low_pass_2(1.0, fs, fs / 4, fs / 8, 53.0)
                for sign in (-1.0, +1.0):
                    half = fe.chan_open_taps(-1, 2, taps, sign * fs / 4)
                    self.sources[numsources] = {
                        "center_freq": src["center_freq"] + sign * fs / 4, "samp_rate": src["samp_rate"] / 2,
                        "block": fe, "source_id": source, "offset": src.get("offset", 0), "parent_chan": half,
                    }
                    numsources += 1
                continue
            self.sources[numsources] = {
                "center_freq": src["center_freq"], "samp_rate": src["samp_rate"],
                "block": fe, "source_id": source, "offset": src.get("offset", 0),
            }
            if getattr(config, "frontend_mode", "xlat") == "pfb":
                self.sources[numsources]["pfb"] = self._open_pfb(fe, float(src["samp_rate"]))
            numsources += 1
        if getattr(config, "frontend_mode", "xlat") not in ("xlat", "pfb"):
            self.access_lock.release()
            raise Exception("No frontend_mode selected")
        self.channels = {}
        self.access_lock.release()

    def _open_pfb(self, fe, samp_rate):
        """frontend_mode == 'pfb' (the reference's receiver.py:242-261 built pfb.channelizer_ccf(fs / 400 kHz bins)
        + a second xlating stage per channel and never finished it).  Here the bank is built from the channel
        filter itself -- decim = int(fs/cr)/2, low_pass_2(1, fs, cr/2, cr/2, 20, HAMMING) (channel.py:31-33) on a
        `pfb_grid` Hz raster (default: cr = 12.5 kHz) -- so every bin IS the channel the xlat path would have built
        at that frequency and no second stage is needed.  Returns the plan, or None when librcf has no kernel for
        the shape (then every request takes the direct path, as in 'xlat' mode).

        Deployment knobs (config attributes; defaults reproduce the SURVEY 8(d) cfg2 environment):
          pfb_parity_budget   discriminator rms error allowed between a served bin and GNU Radio's channel (1e-4);
                              None = no routing, every on-grid request is a bin (exact phases instead of GNU Radio's)
          pfb_parity_env_db   wideband input power over the served carrier's power in dB (default 15.3 = unit noise + 32
                              carriers of +30 dB at 20 Msps).  Weaker carriers in a busier band -> larger value -> fewer
                              bins served by the bank; measure it as 10 log10(mean |x|^2 / carrier power)
          pfb_parity_gain     discriminator gain of the consumers (default P25's out_rate / (2 pi 600))
          pfb_parity_margin   measured / predicted safety factor (2.5)
          pfb_mixed_radix     True: also open the banks of the mixed-radix family (native.pfb_shape_family == 3: 160, 192,
                              480, 640, 960, 1280 bins -- 2, 2.4, 6, 8, 12, 16 Msps on the 12.5 kHz grid).  Default False:
                              those rates were served by direct channels before the family existed, and a deployment does
                              not change its serving path through a library upgrade
        How requests were routed is logged per channel and counted in metrics() (rcf_pfb_served_by_bank,
        rcf_pfb_direct_parity_budget, rcf_pfb_direct_off_grid)."""
        from . import native
        cr = int(getattr(self.config, "pfb_channel_rate", 12500))
        grid = float(getattr(self.config, "pfb_grid", cr))
        try:
            decim, ntaps = native.channel_params(samp_rate, cr, 1 if getattr(self.config, "py2_decim", False) else 0)
        except native.RcfError:
            return None
        n_bins = samp_rate / grid
        if n_bins != int(n_bins) or int(n_bins) % decim or not native.pfb_shape_supported(int(n_bins), decim, ntaps):
            self.log.warning("no filterbank kernel for fs=%s grid=%s: direct channels only" % (samp_rate, grid))
            return None
        if native.pfb_shape_family(int(n_bins), decim, ntaps) == 3 and not getattr(self.config, "pfb_mixed_radix", False):
            self.log.warning("no filterbank kernel for fs=%s grid=%s: direct channels only "
                             "(a %d-bin mixed-radix bank exists: config.pfb_mixed_radix = True opens it)"
                             % (samp_rate, grid, int(n_bins)))
            return None
        taps = native.design_low_pass_2(1.0, samp_rate, cr / 2, cr / 2, 20.0)
        fe.pfb_open(int(n_bins), decim, taps)
        plan = {"n_bins": int(n_bins), "grid": grid, "decim": decim, "ntaps": ntaps, "channel_rate": cr,
                "samp_rate": samp_rate, "taps": taps, "leak": {}}
        # Parity routing.  A bin of the bank has exact tap phases; GNU Radio's channel at the same offset has
        # float32-rounded ones (freq_xlating_fir_filter_ccc: float32(i * fwT0)) -- a per-bin error filter
        # the bank cannot reproduce (native.pfb_tap_leakage).  A request is served by its bin only while the
        # discriminator error predicted from that filter stays inside the budget; otherwise it takes the direct
        # kernel, which carries GNU Radio's phases tap for tap.
        #   predicted fm rms = gain * margin * leak_l2(bin) * 10^(env_db / 20)
        #   gain    discriminator gain the consumers use (P25: out_rate / (2 pi 600), p25_control_demod.py:120)
        #   env_db  wideband input power over the served carrier's power.  Default = the SURVEY 8(d) cfg2 stream:
        #           unit-variance noise + 32 carriers of +30 dB in 12.5 kHz at 20 Msps, 10 log10(21 / 0.625)
        #   margin  the leakage is not white (images of strong carriers); 2.4 was the largest measured / predicted
        #           ratio over all 1600 bins (profiles/r03_pfb_allbins_vs_gr.json)
        budget = getattr(self.config, "pfb_parity_budget", 1e-4)
        plan["parity"] = None if budget is None else {
            "budget": float(budget),
            "gain": float(getattr(self.config, "pfb_parity_gain", (samp_rate / decim) / (2 * math.pi * 600.0))),
            "env_db": float(getattr(self.config, "pfb_parity_env_db", 10 * math.log10(21.0 / 0.625))),
            "margin": float(getattr(self.config, "pfb_parity_margin", 2.5)),
        }
        return plan

    @staticmethod
    def pfb_predicted_fm_error(plan, k):
        """discriminator rms error predicted for bin k served by the bank (see _open_pfb); 0.0 when routing is off"""
        from . import native
        par = plan.get("parity")
        if par is None:
            return 0.0
        k %= plan["n_bins"]
        if k not in plan["leak"]:
            plan["leak"][k] = native.pfb_tap_leakage(plan["samp_rate"], plan["n_bins"], plan["taps"], k)[0]
        return par["gain"] * par["margin"] * plan["leak"][k] * 10 ** (par["env_db"] / 20)

    @staticmethod
    def pfb_serves_bin(plan, k):
        """True when the parity budget lets the bank's bin k stand in for GNU Radio's channel at that offset"""
        par = plan.get("parity")
        return par is None or receiver.pfb_predicted_fm_error(plan, k) <= par["budget"]

    # ------------------------------------------------------------------ data plane
    def feed(self, source_id, iq):
        """Deliver wideband cf32 samples for one source (replaces source -> pub_sink, receiver.py:201).
        With receiver_split2 both halves of a real source share one front-end: feed either, once."""
        src = self.sources[source_id]
        try:
            if "parent_chan" in src:
                # the half-band channel writes n/2 samples per push into a ring of the front-end's out_capacity
                # (default 2^16): deliver in pieces that fit, block cuts do not change the result
                step = src.get("feed_chunk", 1 << 16)
                for at in range(0, len(iq), step):
                    src["block"].push(iq[at:at + step])
            else:
                src["block"].push(iq)
        except Exception as e:
            # a failed launch / copy leaves the front-end's stream state undefined: remember it (the registry
            # publisher stops heartbeating on healthy() == False, so clients move to another channelizer within
            # the manager's 5 s expiry) and let the producer see the error
            if self.fault is None:
                self.fault = "%s: %s" % (type(e).__name__, e)
                self.log.error("data plane failed on source %s: %s" % (source_id, self.fault))
            raise
        self._fed[source_id] = self._fed.get(source_id, 0) + len(iq)

    def feed_raw(self, source_id, raw, fmt, scale, offset=0.0):
        """feed() for samples still in the SDR's wire format (interleaved I, Q as uint8 / int8 / int16: what the rtlsdr
        and USRP sc8 / sc16 links of receiver.py:91-98,170-191 carry before the driver converts them): (v - offset) *
        scale happens on the GPU (rcf_push_raw), the link carries 2 or 4 bytes per sample instead of 8."""
        src = self.sources[source_id]
        n = len(raw) // 2
        try:
            step = src.get("feed_chunk", 1 << 16) if "parent_chan" in src else max(n, 1)
            for at in range(0, n, step):
                src["block"].push_raw(raw[2 * at:2 * (at + step)], fmt, scale, offset)
        except Exception as e:
            if self.fault is None:
                self.fault = "%s: %s" % (type(e).__name__, e)
                self.log.error("data plane failed on source %s: %s" % (source_id, self.fault))
            raise
        self._fed[source_id] = self._fed.get(source_id, 0) + n

    # ---- all sources at once: the reference's receiver holds EVERY configured source in one top block when no -i is
    # given (receiver.py:67-70,170-204; ten of them in configs/config_denver_dev_den817.py:25-118) and GNU Radio's
    # scheduler moves all their samples.  Here the front-ends of one receiver form a group (rcf_group_*): the blocks that
    # are handed over together go out as ONE conversion / filterbank / stage-2 / tap launch instead of one set per source.
    def _group_for_feed(self):
        """the native group over this receiver's front-ends, built on first use; None when there is nothing to group (one
        source, a stub front-end without the native handle, half-band sub-sources that are fed in pieces)"""
        if getattr(self, "_group_tried", False):
            return self._group
        self._group_tried, self._group, self._group_index = True, None, {}
        if any("parent_chan" in s_ for s_ in self.sources.values()):
            return None
        blocks = []
        for sid in sorted(self.sources):
            fe = self.sources[sid]["block"]
            if not hasattr(fe, "_h"):
                return None
            self._group_index[sid] = len(blocks)
            blocks.append(fe)
        if len(blocks) < 2:
            return None
        try:
            from . import native
            self._group = native.Group(blocks)
        except Exception as e:                               # (different devices / ring sizes): one by one, as before
            self.log.warning("sources are fed one by one: %s" % e)
            self._group = None
        return self._group

    def feed_all(self, blocks, fmt=None, scale=1.0, offset=0.0):
        """blocks: {source_id: samples} for any subset of the sources -- complex64 (fmt None) or the SDR's wire format
        (fmt = native.FMT_U8 / FMT_S8 / FMT_S16 with scale / offset as feed_raw).  One group block for all of them."""
        grp = self._group_for_feed()
        if grp is None:
            for sid, b in blocks.items():
                if fmt is None:
                    self.feed(sid, b)
                else:
                    self.feed_raw(sid, b, fmt, scale, offset)
            return
        row = [None] * len(grp)
        for sid, b in blocks.items():
            row[self._group_index[sid]] = b
        try:
            grp.push(row, 0 if fmt is None else fmt, scale, offset)
        except Exception as e:
            if self.fault is None:
                self.fault = "%s: %s" % (type(e).__name__, e)
                self.log.error("data plane failed on a group block: %s" % self.fault)
            raise
        for sid, b in blocks.items():
            self._fed[sid] = self._fed.get(sid, 0) + (len(b) if fmt is None else len(b) // 2)

    def enable_kernel_metrics(self, stride=32):
        """kernel time and HBM rate in the status line and the registry record.  Every `stride`-th
        launch of each kernel class is bracketed with HIP events on the front-end's own stream (rcf_timing_*: an event
        record costs ~6 us of queue gap, hence the stride); metrics() turns them into per-class average launch times, the
        estimated GPU-busy share and the input bytes per second of kernel time."""
        self._kernel_stride = int(stride)
        for fe in {id(s["block"]): s["block"] for s in self.sources.values()}.values():
            if hasattr(fe, "timing_enable"):
                fe.timing_enable(True)
                fe.timing_stride(self._kernel_stride)
        self._kernel_mark = time.time()

    def _kernel_metrics(self, d_samples):
        from . import native
        names = {native.T_FIR: "fir", native.T_FIR_MFMA: "fir_mfma", native.T_PFB: "pfb", native.T_FIR_DERIVED: "fir_stage2",
                 native.T_DISC: "disc", native.T_TAPS: "tap_finalize", native.T_SCAN_FFT: "scan_fft",
                 native.T_SCAN_MOVSUM: "scan_sum", native.T_AUDIO: "audio", native.T_HISTORY: "copies"}
        now = time.time()
        wall = max(now - self._kernel_mark, 1e-9)
        self._kernel_mark = now
        per, est_ms = {}, 0.0
        for fe in {id(s["block"]): s["block"] for s in self.sources.values()}.values():
            for cls, name in names.items():
                try:
                    ms, n = fe.timing_read(cls)
                except Exception:
                    continue
                if n:
                    a = per.setdefault(name, [0.0, 0])
                    a[0] += ms
                    a[1] += n
                    est_ms += ms * self._kernel_stride        # every stride-th launch was timed
        out = {"rcf_kernel_us": {k: v[0] / v[1] * 1e3 for k, v in per.items()},
               "rcf_gpu_busy_fraction_est": est_ms * 1e-3 / wall}
        if est_ms > 0:
            out["rcf_input_GBps_of_kernel_time"] = d_samples * 8.0 / (est_ms * 1e-3) / 1e9
        return out

    def healthy(self):
        """False once a push has failed (GPU / driver error).  The reference has no such signal: a dead flowgraph
        keeps publishing; here the heartbeat stops (registry.redis_channel_publisher(health=...))."""
        return self.fault is None

    def metrics(self):
        """Additive keys for the registry record (metrics): samples delivered and the input rate since the
        previous call, channels in use, the fault string if any.  Nothing the reference's readers look at."""
        now = time.time()
        total = sum(self._fed.values())
        t_prev, n_prev = self._fed_mark
        rate = (total - n_prev) / (now - t_prev) / 1e6 if now > t_prev else 0.0
        self._fed_mark = (now, total)
        kernel = self._kernel_metrics(total - n_prev) if getattr(self, "_kernel_stride", 0) else {}
        with self.access_lock:
            in_use = sum(1 for c in self.channels.values() if getattr(c, "in_use", False))
            n_chan = len(self.channels)
            routes = [getattr(c, "route", "direct") for c in self.channels.values()]
        out = {"rcf_samples_in": int(total), "rcf_msps_in": rate, "rcf_channels_in_use": in_use,
               "rcf_channels_open": n_chan, "rcf_healthy": self.fault is None}
        if any(s.get("pfb") is not None for s in self.sources.values()):
            # frontend_mode == 'pfb': how the open channels are served (the parity routing was silent)
            out["rcf_pfb_served_by_bank"] = sum(1 for r in routes if r.startswith("bank"))
            out["rcf_pfb_direct_parity_budget"] = sum(1 for r in routes if "parity budget" in r)
            out["rcf_pfb_direct_off_grid"] = sum(1 for r in routes if "off the bank" in r)
        if self.fault is not None:
            out["rcf_fault"] = self.fault
        out.update(kernel)
        return out

    # ------------------------------------------------------------------ control plane
    def connect_channel(self, channel_rate, freq):
        mode = getattr(self.config, "frontend_mode", "xlat")
        if mode in ("xlat", "pfb"):
            # one entry point for both modes: in 'pfb' mode the source carries a filterbank plan and the channel
            # object picks bin or direct kernel per request (channel._build); source selection, idle re-use and the
            # return value are the xlat ones (the reference's own 'pfb' branch is dead code: receiver.py:403 calls
            # channel() with four arguments)
            return self.connect_channel_xlat(channel_rate, freq)
        raise Exception("No frontend_mode selected")

    def connect_channel_xlat(self, channel_rate, freq):
        """receiver.py:282-341"""
        source_id = None
        source_distance = None
        if not self.scan_mode:
            for i in list(self.sources):
                if abs(freq - self.sources[i]["center_freq"]) < self.sources[i]["samp_rate"] / 2:
                    if source_distance is None or abs(freq - self.sources[i]["center_freq"]) < source_distance:
                        source_id = i
                        source_distance = abs(freq - self.sources[i]["center_freq"])
            if source_id is None:
                raise Exception("Unable to find source for frequency %s" % freq)
        else:
            source_id = 0
        source_center_freq = self.sources[source_id]["center_freq"]
        source_samp_rate = self.sources[source_id]["samp_rate"]
        frontend = self.sources[source_id]["block"]

        offset = freq - source_center_freq
        if freq < 10000000:
            offset = freq                                   # scan mode, relative freq (receiver.py:304-305)

        with self.access_lock:
            block = None
            for c in list(self.channels):
                ch = self.channels[c]
                if ch.source_id == source_id and ch.channel_rate == channel_rate and not ch.in_use:
                    block = ch                              # re-use an idling channel (receiver.py:311-319)
                    block.set_offset(offset)
                    block.channel_close_time = 0
                    break
            if block is None:
                port = None
                for attempt in range(3):                    # receiver.py:322-329
                    cand = random.randint(10000, 60000)
                    if self.bind_port is None or self.bind_port(cand):
                        port = cand
                        break
                    self.log.error("Failed to build channel on port: %s attempt: %s" % (cand, attempt))
                if port is None:
                    raise Exception("no free egress port")
                try:
                    block = channel_mod.channel(frontend, port, channel_rate, source_samp_rate, offset,
                                                parent_chan=self.sources[source_id].get("parent_chan"),
                                                pfb=self.sources[source_id].get("pfb"),
                                                decim_rule=1 if getattr(self.config, "py2_decim", False) else 0)
                except Exception:
                    if self.release_port is not None:      # the sockets bound above have no channel: close them
                        self.release_port(port)
                    raise
                block.source_id = source_id
                if self.sources[source_id].get("pfb") is not None:
                    self.log.info("channel at offset %s Hz served by: %s" % (offset, block.route))
                block.block_id = "%s" % uuid.uuid4()
                self.channels[block.block_id] = block
                block.start()
            block.in_use = True
            return block.block_id, block.port

    def release_channel(self, block_id):
        """receiver.py:424-435: release only marks the channel idle; the sweep destroys it later."""
        with self.access_lock:
            if block_id not in self.channels:
                return True
            self.channels[block_id].in_use = False
            self.channels[block_id].channel_close_time = time.time()
            return True

    def source_offset(self, block_id, offset):
        """receiver.py:436-475: demod-reported drift -> Hz -> retune.  The reference retunes the SDR
        hardware; here the same Hz correction is applied to every channel's NCO (rcf_source_shift)."""
        if self.scan_mode:
            return False
        try:
            src = self.sources[self.channels[block_id].source_id]
        except Exception:
            return False
        accumulated_offset = src.get("accumulated_offset", 0)
        if offset > 1 or offset < -1:
            hz_offset = offset * 50
        elif offset > 0.5 or offset < -0.5:
            hz_offset = offset * 10
        else:
            hz_offset = offset * 4
        if -5 < hz_offset < 5:
            return True
        total_offset = accumulated_offset + hz_offset
        if abs(total_offset) > self.channels[block_id].channel_rate / 2:
            total_offset = (total_offset / 2) * -1
        with self.access_lock:
            # hardware: set_center_freq(center + total) moves every signal by -total at baseband while the
            # channel NCOs stay put; moving every NCO by +total instead leaves the same signal-to-NCO
            # distance, so the shift to apply is the change of the accumulated offset
            src["block"].source_shift(total_offset - accumulated_offset)
            src["accumulated_offset"] = total_offset
            # (filterbank mode: bins stay on the raster, the taps' rotators carry the correction -- rcf_source_shift
            # applies to channels fed by bins too -- and new requests keep landing on bins)
        return True

    def scan_mode_set_freq(self, freq):
        """handler 'scan_mode_set_freq' (receiver.py:556-566): retune source 0's centre frequency."""
        self.sources[0]["center_freq"] = freq
        return True

    def sweep_idle_channels(self, now=None):
        """receiver.py:635-648: destroy channels idle for longer than channel_idle_timeout."""
        now = time.time() if now is None else now
        deleted = []
        with self.access_lock:
            for c in list(self.channels):
                ch = self.channels[c]
                if ch.channel_close_time != 0 and now - ch.channel_close_time > self.channel_idle_timeout:
                    ch.destroy()
                    del self.channels[c]
                    deleted.append(c)
            self.last_channel_cleanup = now
        return deleted

    def close(self):
        with self.access_lock:
            if getattr(self, "_group", None) is not None:
                self._group.close()
                self._group = None
            for c in list(self.channels):
                self.channels[c].destroy()
            self.channels.clear()
            for fe in {id(s["block"]): s["block"] for s in self.sources.values()}.values():
                fe.close()
