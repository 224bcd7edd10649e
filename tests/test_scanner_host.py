"""rcf.scanner.Scanner -- the reference's scanning_receiver on the GPU's carrier detector -- against a small fake front end:
the grid mapping (the negative-frequency bins too), a channel for an off-grid frequency, one on_progress per advance, and a
transmission shorter than a poll interval."""
import numpy as np

from rcf import scanner


class FakeFrontend:
    """what Scanner asks of a front end, with the detector's counters set by the test"""

    def __init__(self, samp_rate, center_freq):
        self.samp_rate, self.center_freq = float(samp_rate), float(center_freq)
        self.opened, self.closed = [], []          # (channel rate, offset) / channel ids
        self.chan_thr = {}                         # cid -> (threshold, alpha)
        self.chan_n_open = {}
        self.pfb_thr = None
        self.bin_n_open = None
        self.reads = 0

    def chan_open(self, channel_rate, offset_hz):
        self.opened.append((channel_rate, offset_hz))
        cid = len(self.opened)
        self.chan_n_open[cid] = 0
        return cid

    def chan_close(self, cid):
        self.closed.append(cid)

    def chan_squelch(self, cid, threshold_db, alpha=0.1):
        self.chan_thr[cid] = (threshold_db, alpha)

    def chan_squelch_state(self, cid):
        assert cid in self.chan_thr
        return dict(level=0.0, n_seen=0, n_open=self.chan_n_open[cid], first_open=-1, last_open=-1, unmuted=0)

    def pfb_squelch(self, threshold_db, alpha=0.1):
        self.pfb_thr = None if threshold_db is None else (threshold_db, alpha)

    def pfb_squelch_read(self, n_bins):
        assert self.pfb_thr is not None
        self.reads += 1
        if self.bin_n_open is None:
            self.bin_n_open = np.zeros(n_bins, np.int64)
        return dict(n_open=self.bin_n_open.copy())


FS, FC, NB = 20e6, 855e6, 1600                      # the reference grid: 12.5 kHz bins


def system(channels):
    return {"id": 7, "channels": channels, "threshold": -35.0, "modulation": "analog"}


def make(channels, n_bins=NB):
    fe = FakeFrontend(FS, FC)
    calls = []
    sc = scanner.Scanner(system(channels), fe, calls.append, n_bins=n_bins)
    fe.bin_n_open = np.zeros(n_bins or 1, np.int64)
    return fe, sc, calls


def test_grid_frequencies_map_to_their_bins_the_negative_ones_too():
    chans = {0: FC, 1: FC + 12500, 2: FC - 12500, 3: FC + 799 * 12500, 4: FC - 800 * 12500, 5: FC - 37 * 12500}
    fe, sc, _ = make(chans)
    assert sc.bins == {FC: 0, FC + 12500: 1, FC - 12500: NB - 1, FC + 799 * 12500: 799, FC - 800 * 12500: 800, FC - 37 * 12500: NB - 37}
    assert not sc.chans and not fe.opened
    assert fe.pfb_thr == (-35.0, 0.1)              # system['threshold'], the reference's alpha
    assert sc.hang_time == 0.5 and sc.channel_rate == 12500


def test_off_grid_and_out_of_band_frequencies_and_no_bank_open_a_channel():
    chans = {"a": FC + 6250.0, "b": FC + 12500.0, "c": FC + 800 * 12500.0, "d": FC + 100.0}
    fe, sc, _ = make(chans)
    assert sc.bins == {FC + 12500.0: 1}
    assert fe.opened == [(12500, 6250.0), (12500, 800 * 12500.0), (12500, 100.0)]          # a 12.5 kHz channel each
    assert sorted(sc.chans) == sorted([FC + 6250.0, FC + 800 * 12500.0, FC + 100.0])
    assert all(fe.chan_thr[cid] == (-35.0, 0.1) for cid in sc.chans.values())
    # no bank: every frequency is a channel, and the bank's detector is never touched
    fe2, sc2, _ = make({"b": FC + 12500.0, "e": FC - 25000.0}, n_bins=None)
    assert not sc2.bins and len(fe2.opened) == 2 and fe2.pfb_thr is None
    sc2.poll()
    assert fe2.reads == 0
    sc2.close()
    assert fe2.closed == [1, 2]


def test_one_on_progress_per_advance_and_none_without():
    f_bin, f_bin2, f_chan = FC + 25000.0, FC - 50000.0, FC + 3000.0
    fe, sc, calls = make({0: f_bin, 1: f_bin2, 2: f_chan})        # no one-channel limit
    cid = sc.chans[f_chan]
    assert sc.poll() == [] and calls == []
    fe.bin_n_open[2] = 40
    assert sc.poll() == [f_bin] and calls == [f_bin]
    assert sc.poll() == [] and calls == [f_bin]                   # nothing advanced: nothing reported
    fe.bin_n_open[2] = 41
    fe.bin_n_open[NB - 4] = 9
    fe.chan_n_open[cid] = 3
    assert sc.poll() == [f_bin, f_bin2, f_chan]                   # the order of system['channels']
    assert calls == [f_bin, f_bin, f_bin2, f_chan]
    fe.bin_n_open[5] = 1000                                       # a bin nobody watches
    assert sc.poll() == []
    assert fe.reads == 5                                          # one read of the bank per poll, however many bins
    sc.close()
    assert fe.pfb_thr is None and fe.closed == [cid]


def test_a_transmission_shorter_than_a_poll_interval_is_still_reported():
    """it opened and closed between two polls: `unmuted` is 0 at both, the count of open samples has advanced"""
    f = FC + 12500.0
    fe, sc, calls = make({0: f})
    sc.poll()
    fe.bin_n_open[1] += 12          # twelve open frames, and the bin is muted again by the time anybody looks
    assert sc.poll() == [f] and calls == [f]
    assert sc.poll() == []


def test_a_frequency_listed_twice_is_watched_once():
    f = FC + 12500.0
    fe, sc, calls = make({0: f, 1: f})
    fe.bin_n_open[1] = 2
    assert sc.poll() == [f] and calls == [f]
