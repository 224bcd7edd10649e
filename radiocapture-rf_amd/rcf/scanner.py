"""The conventional-channel ("scanner") system type: what scanning_receiver.py is to the reference.

There, one scanning_receiver per watched frequency hangs analog.simple_squelch_cc(system['threshold'], 0.1) behind a
12.5 kHz channel, and a thread polls squelch.unmuted() every 10 ms and calls call_progress(freq), which opens or keeps alive
a logging_receiver with hang_time 0.5 ("1 channel per scanner pls", scanning_receiver.py:104).  Here the detector runs on
the GPU (rcf_chan_squelch / rcf_pfb_squelch, include/rcf.h) and a Scanner watches any number of frequencies of one
front-end:

  * a frequency on the grid of the front-end's open filterbank IS one of its bins: the bank's detector covers every bin
    with two launches per block, and the scanner reads the watched ones out of one rcf_pfb_squelch_read;
  * any other frequency gets a 12.5 kHz channel with the stage attached, as in the reference.

poll() reports every frequency whose count of open samples advanced since the last poll.  The reference's rule is "unmuted
at the poll"; this one does not miss a transmission that opened and closed between two polls.  There is no polling thread:
whoever feeds the front-end calls poll() as often as it wants progress (a block's latency at the least).

With capture=dict(pre_s=..., hang_s=...) every watched frequency also gets the capture stage (rcf_chan_capture): the detector as
a gate on the device, so that poll() hands on_call(freq, rec, iq) the samples of every finished transmission -- and nothing
else crosses the link.  The reference's logging_receiver opens only after the poll has seen the carrier and has lost the
head of the transmission by then: its 10 ms poll period at the very least, which is the default lead-in here (pre_s =
poll_period).  Handing over the head is a deliberate improvement on the reference, not parity with it."""
from __future__ import annotations

import numpy as np


class Scanner:
    hang_time = 0.5                  # what call_progress puts into the call record (scanning_receiver.py:27,93)
    channel_rate = 12500             # scanning_receiver.py:28
    alpha = 0.1                      # simple_squelch_cc's second argument (scanning_receiver.py:53)
    poll_period = 0.010              # the reference's poll of unmuted() (scanning_receiver.py:108-113): what it loses at best

    def __init__(self, system, frontend, on_progress, n_bins=None, capture=None, on_call=None):
        """system: {'id', 'channels': {key: freq in Hz}, 'threshold' (dB), 'modulation'}; frontend: a native.Frontend (or
        anything with its samp_rate, center_freq, chan_open / chan_close / chan_squelch / chan_squelch_state and
        pfb_squelch / pfb_squelch_read); on_progress(freq): the reference's call_progress; n_bins: the bins of the
        front-end's open filterbank, None when it has none.
        capture: None (nothing changes), or dict(pre_s=Scanner.poll_period, hang_s=Scanner.hang_time, capacity=0,
        rec_capacity=0): every watched frequency gets the capture stage -- an off-grid one on its 12.5 kHz channel, an on-grid
        one on a pfb_tap_open of its bin --, pre and hang rounded from seconds at the channel's output rate (chan_info), and
        poll() calls on_call(freq, rec, iq) once per CLOSED window: iq the window's samples (complex64), rec a dict(sample,
        end: the window's first sample and the first one behind it, in channel samples; pos: its place in the captured
        stream; n_open, peak: the CLOSE record's; rate: the channel's output rate; lost: samples of the window a lagging
        reader lost, 0 for a whole one).  The front-end then also needs chan_capture / chan_capture_state /
        chan_read_capture / chan_read_capture_rec, chan_info and pfb_tap_open.  poll() and whoever pushes blocks share one
        thread."""
        self.system = system
        self.system_id = system["id"]
        self.channels = dict(system["channels"])
        self.threshold = float(system["threshold"])
        self.modulation = system.get("modulation", "analog")
        self.fe = frontend
        self.on_progress = on_progress
        self.n_bins = int(n_bins) if n_bins else 0
        self.bins = {}               # freq -> bin of the bank
        self.chans = {}              # freq -> channel id
        self._seen = {}              # freq -> n_open at the last poll
        for freq in self.channels.values():
            if freq in self._seen:
                continue
            b = self.bin_of(freq)
            if b is None:
                cid = frontend.chan_open(self.channel_rate, float(freq) - frontend.center_freq)
                frontend.chan_squelch(cid, self.threshold, self.alpha)
                self.chans[freq] = cid
            else:
                self.bins[freq] = b
            self._seen[freq] = 0
        if self.bins:
            frontend.pfb_squelch(self.threshold, self.alpha)
        self.capture = None if capture is None else dict(capture)
        self.on_call = on_call
        self.cap = {}                # freq -> the capture's state on the host (_attach_capture)
        if self.capture is not None:
            for freq in self._seen:
                self._attach_capture(freq)

    def _attach_capture(self, freq):
        fe, c = self.fe, self.capture
        if freq in self.chans:
            cid, own = self.chans[freq], False
        else:
            cid, own = fe.pfb_tap_open(self.bins[freq], gr_phase=False), True
        rate = float(fe.chan_info(cid)["out_rate"])
        pre = int(round(float(c.get("pre_s", self.poll_period)) * rate))
        hang = int(round(float(c.get("hang_s", self.hang_time)) * rate))
        fe.chan_capture(cid, self.threshold, self.alpha, pre=pre, hang=hang, capacity=int(c.get("capacity", 0)),
                        rec_capacity=int(c.get("rec_capacity", 0)))
        # at: captured-stream items consumed; n_rec: records consumed; open: the pending OPEN record; segs: [(pos, samples)]
        # read but not yet handed over
        self.cap[freq] = dict(cid=cid, own=own, rate=rate, pre=pre, hang=hang, at=0, n_rec=0, open=None, segs=[], rec_lost=False)

    def _take(self, k, lo, hi):
        """the buffered samples of stream positions [lo, hi) -- what is left of them --, and everything before hi dropped"""
        parts, rest = [], []
        for pos, a in k["segs"]:
            i, j = max(lo - pos, 0), min(hi - pos, len(a))
            if j > i:
                parts.append(a[i:j])
            if pos + len(a) > hi:
                cut = max(hi - pos, 0)
                rest.append((pos + cut, a[cut:]))
        k["segs"] = rest
        return np.concatenate(parts) if parts else np.zeros(0, np.complex64)

    def _poll_capture(self, freq):
        k = self.cap[freq]
        recs = self.fe.chan_read_capture_rec(k["cid"])
        iq = self.fe.chan_read_capture(k["cid"])
        st = self.fe.chan_capture_state(k["cid"])
        # a reader that lagged more than a ring gets the NEWEST items: the chunks end where the stage's counters stand
        if len(iq):
            k["segs"].append((int(st["n_kept"]) - len(iq), iq))
        k["at"] = int(st["n_kept"])
        if int(st["n_records"]) - len(recs) != k["n_rec"]:          # records lost: the pending OPEN cannot be trusted
            k["open"], k["rec_lost"] = None, True
        k["n_rec"] = int(st["n_records"])
        calls = []
        for r in recs:
            if int(r["kind"]) == 1:                                 # OPEN
                k["open"] = r
                continue
            o, hi = k["open"], int(r["pos"])
            lo = int(o["pos"]) if o is not None else (k["segs"][0][0] if k["segs"] else hi)
            iq_w = self._take(k, lo, hi)
            n_win = hi - int(o["pos"]) if o is not None else None
            lost = (n_win - len(iq_w)) if n_win is not None else -1  # -1: the OPEN record itself was lost, the length unknown
            first = int(o["sample"]) if o is not None else int(r["sample"]) - len(iq_w)
            calls.append((dict(sample=first, end=int(r["sample"]), pos=lo, n_open=int(r["n_open"]), peak=float(r["peak"]),
                               rate=k["rate"], lost=lost), iq_w))
            k["open"], k["rec_lost"] = None, False
        if k["open"] is None and not st["in_window"]:
            k["segs"] = []                                          # nothing pending: what is buffered belongs to lost windows
        for rec, iq_w in calls:
            if self.on_call is not None:
                self.on_call(freq, rec, iq_w)
        return len(calls)

    def bin_of(self, freq):
        """the bank's bin centred on freq -- bin k at k fs / n_bins for k < n_bins / 2, (k - n_bins) fs / n_bins above --, or
        None: no bank, off its grid, or outside the band"""
        if not self.n_bins:
            return None
        k = (float(freq) - self.fe.center_freq) * self.n_bins / self.fe.samp_rate
        kr = round(k)
        if abs(k - kr) > 1e-6 or not -self.n_bins // 2 <= kr < (self.n_bins + 1) // 2:
            return None
        return int(kr) % self.n_bins

    def poll(self):
        """on_progress(freq) for every watched frequency whose open-sample count advanced since the last poll, in the order
        of system['channels']; -> the frequencies reported"""
        counts = {}
        if self.bins:
            n_open = self.fe.pfb_squelch_read(self.n_bins)["n_open"]
            for freq, b in self.bins.items():
                counts[freq] = int(n_open[b])
        for freq, cid in self.chans.items():
            counts[freq] = int(self.fe.chan_squelch_state(cid)["n_open"])
        active = []
        for freq in self._seen:
            if counts[freq] > self._seen[freq]:
                active.append(freq)
            self._seen[freq] = counts[freq]
        for freq in active:
            self.on_progress(freq)
        for freq in self.cap:
            self._poll_capture(freq)
        return active

    def close(self):
        """the channels go (a capture's tap among them), the bank's detector is switched off"""
        for k in self.cap.values():
            if k["own"]:
                self.fe.chan_close(k["cid"])
        self.cap = {}
        for cid in self.chans.values():
            self.fe.chan_close(cid)
        self.chans = {}
        if self.bins:
            self.fe.pfb_squelch(None)
        self.bins = {}
        self._seen = {}
