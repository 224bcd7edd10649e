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
whoever feeds the front-end calls poll() as often as it wants progress (a block's latency at the least)."""
from __future__ import annotations


class Scanner:
    hang_time = 0.5                  # what call_progress puts into the call record (scanning_receiver.py:27,93)
    channel_rate = 12500             # scanning_receiver.py:28
    alpha = 0.1                      # simple_squelch_cc's second argument (scanning_receiver.py:53)

    def __init__(self, system, frontend, on_progress, n_bins=None):
        """system: {'id', 'channels': {key: freq in Hz}, 'threshold' (dB), 'modulation'}; frontend: a native.Frontend (or
        anything with its samp_rate, center_freq, chan_open / chan_close / chan_squelch / chan_squelch_state and
        pfb_squelch / pfb_squelch_read); on_progress(freq): the reference's call_progress; n_bins: the bins of the
        front-end's open filterbank, None when it has none."""
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
        return active

    def close(self):
        """the channels go, the bank's detector is switched off"""
        for cid in self.chans.values():
            self.fe.chan_close(cid)
        self.chans = {}
        if self.bins:
            self.fe.pfb_squelch(None)
        self.bins = {}
        self._seen = {}
