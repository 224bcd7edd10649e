"""rcf.scanner.Scanner(capture=...) against a fake front end that replays a scripted capture stage: a stream of kept samples
and OPEN / CLOSE records, released to the readers step by step, in rings that lose their oldest items as the device's do.
Windows split across polls, two windows in one poll, a window whose head a lagging reader lost (flagged), the wiring of
on-grid and off-grid frequencies, and capture=None left as it was."""
import numpy as np

import capture_ref as R
from rcf import scanner
from test_scanner_host import FakeFrontend, FS, FC, NB, system


class CaptureFake(FakeFrontend):
    """adds the capture stage: script[cid] = (samples complex64, records REC_DTYPE) is the stage's whole output; advance(cid,
    n_kept, n_records) says how much of it exists; the readers hand out what is new, the oldest lost beyond the rings"""

    def __init__(self, samp_rate, center_freq, rates=None):
        super().__init__(samp_rate, center_freq)
        self.rates = rates or {}
        self.taps, self.captures, self.script, self.now, self.rd, self.in_window = {}, {}, {}, {}, {}, {}

    def pfb_tap_open(self, bin_, gr_phase=True):
        cid = 1000 + bin_
        self.taps[cid] = (bin_, gr_phase)
        return cid

    def chan_info(self, cid):
        return dict(decim=1, ntaps=1, out_rate=self.rates.get(cid, 25000.0), offset_hz=0.0)

    def chan_capture(self, cid, threshold_db, alpha=0.1, pre=0, hang=0, capacity=0, rec_capacity=0):
        self.captures[cid] = dict(threshold_db=threshold_db, alpha=alpha, pre=pre, hang=hang, capacity=capacity or 4096,
                                  rec_capacity=rec_capacity or 256)
        self.now[cid], self.rd[cid], self.in_window[cid] = [0, 0], [0, 0], 0

    def advance(self, cid, n_kept, n_records, in_window=0):
        self.now[cid] = [n_kept, n_records]
        self.in_window[cid] = in_window

    def _read(self, cid, which, items, cap):
        end = self.now[cid][which]
        lo = max(self.rd[cid][which], end - cap)           # lag_clamp
        self.rd[cid][which] = end
        return items[lo:end].copy()

    def chan_read_capture(self, cid, max_samples=1 << 20):
        return self._read(cid, 0, self.script[cid][0], self.captures[cid]["capacity"])

    def chan_read_capture_rec(self, cid, max_records=1 << 12):
        return self._read(cid, 1, self.script[cid][1], self.captures[cid]["rec_capacity"])

    def chan_capture_state(self, cid):
        return dict(level=0.0, n_seen=0, n_decided=0, n_kept=self.now[cid][0], n_records=self.now[cid][1], n_windows=0, last_open=-1,
                    in_window=self.in_window[cid], unmuted=0)


def script(windows):
    """windows: [(first sample, length, n_open, peak)] -> the stage's whole output: sample k of the captured stream is k + 1j
    x its channel-sample index"""
    iq, recs, pos = [], [], 0
    for first, n, n_open, peak in windows:
        recs.append((R.OPEN, 0, first, pos, 0.0, 0))
        iq.append(np.arange(pos, pos + n) + 1j * np.arange(first, first + n))
        pos += n
        recs.append((R.CLOSE, n_open, first + n, pos, peak, 0))
    return np.concatenate(iq).astype(np.complex64), np.array(recs, R.REC_DTYPE)


F_OFF = FC + 6250.0                                    # off the grid: a channel of its own


def make(capture, channels=None, n_bins=None, rates=None):
    fe = CaptureFake(FS, FC, rates)
    calls, prog = [], []
    sc = scanner.Scanner(system(channels or {0: F_OFF}), fe, prog.append, n_bins=n_bins, capture=capture,
                         on_call=lambda f, rec, iq: calls.append((f, rec, iq)))
    fe.bin_n_open = np.zeros(n_bins or 1, np.int64)
    return fe, sc, calls


def test_wiring_of_on_grid_and_off_grid_frequencies():
    chans = {"a": F_OFF, "b": FC + 12500.0, "c": FC - 3 * 12500.0}
    fe, sc, _ = make(dict(pre_s=0.010, hang_s=scanner.Scanner.hang_time), chans, NB, rates={1: 25000.0, 1001: 12500.0, 1000 + NB - 3: 12500.0})
    assert sc.chans == {F_OFF: 1} and sc.bins == {FC + 12500.0: 1, FC - 3 * 12500.0: NB - 3}
    assert fe.taps == {1001: (1, False), 1000 + NB - 3: (NB - 3, False)}          # a tap per watched bin
    # pre and hang from seconds at the channel's own output rate; the detector's parameters are the scanner's
    assert fe.captures[1]["pre"] == 250 and fe.captures[1]["hang"] == 12500
    assert fe.captures[1001]["pre"] == 125 and fe.captures[1001]["hang"] == 6250
    assert all(c["threshold_db"] == -35.0 and c["alpha"] == 0.1 for c in fe.captures.values())
    assert fe.chan_thr == {1: (-35.0, 0.1)} and fe.pfb_thr == (-35.0, 0.1)         # the reporting half is as it was
    sc.close()
    assert sorted(fe.closed) == [1, 1001, 1000 + NB - 3]


def test_the_default_lead_in_is_the_references_poll_period():
    fe, sc, _ = make({})
    assert scanner.Scanner.poll_period == 0.010
    assert fe.captures[1]["pre"] == 250 and fe.captures[1]["hang"] == 12500


def test_capture_none_changes_nothing():
    fe = CaptureFake(FS, FC)
    sc = scanner.Scanner(system({0: F_OFF}), fe, lambda f: None)
    assert not fe.captures and sc.cap == {} and sc.poll() == []


def test_windows_split_across_polls_and_two_windows_in_one_poll():
    fe, sc, calls = make(dict(pre_s=0.001, hang_s=0.002))
    iq, recs = script([(100, 700, 400, 0.5), (2000, 50, 3, 0.25), (2100, 60, 9, 0.125), (5000, 300, 100, 2.0)])
    fe.script[1] = (iq, recs)
    fe.advance(1, 0, 0); sc.poll()
    assert calls == []
    fe.advance(1, 300, 1, in_window=1); sc.poll()          # the OPEN and the window's first 300 samples
    fe.advance(1, 300, 1, in_window=1); sc.poll()          # nothing new
    fe.advance(1, 650, 1, in_window=1); sc.poll()
    assert calls == []
    fe.advance(1, 700, 2); sc.poll()                       # the CLOSE: one call, the window whole, assembled from three reads
    assert len(calls) == 1
    f, rec, got = calls[0]
    assert f == F_OFF and rec == dict(sample=100, end=800, pos=0, n_open=400, peak=0.5, rate=25000.0, lost=0)
    assert got.dtype == np.complex64 and np.array_equal(got, iq[:700])
    fe.advance(1, 700 + 50 + 60 + 120, 7, in_window=1); sc.poll()     # two whole windows and the head of a fourth in one poll
    assert len(calls) == 3
    assert calls[1][1] == dict(sample=2000, end=2050, pos=700, n_open=3, peak=0.25, rate=25000.0, lost=0)
    assert calls[2][1] == dict(sample=2100, end=2160, pos=750, n_open=9, peak=0.125, rate=25000.0, lost=0)
    assert np.array_equal(calls[1][2], iq[700:750]) and np.array_equal(calls[2][2], iq[750:810])
    fe.advance(1, len(iq), 8); sc.poll()
    assert len(calls) == 4 and calls[3][1]["sample"] == 5000 and calls[3][1]["lost"] == 0
    assert np.array_equal(calls[3][2], iq[810:])
    assert sc.cap[F_OFF]["segs"] == []                     # nothing is kept behind a delivered window


def test_a_window_whose_head_a_lagging_reader_lost_is_delivered_flagged():
    fe, sc, calls = make(dict(pre_s=0.0, hang_s=0.0, capacity=256))
    iq, recs = script([(10, 100, 50, 1.0), (1000, 600, 500, 3.0), (4000, 40, 7, 0.5)])
    fe.script[1] = (iq, recs)
    fe.advance(1, 100, 2); sc.poll()
    assert len(calls) == 1 and calls[0][1]["lost"] == 0
    # the reader sleeps through the whole second window: its ring of 256 holds the window's last 256 samples only
    fe.advance(1, 700, 4); sc.poll()
    assert len(calls) == 2
    rec, got = calls[1][1], calls[1][2]
    assert rec["sample"] == 1000 and rec["end"] == 1600 and rec["lost"] == 344 and rec["n_open"] == 500
    assert np.array_equal(got, iq[700 - 256:700])          # what is left: the window's tail
    fe.advance(1, 740, 6); sc.poll()                       # and the stream goes on whole
    assert len(calls) == 3 and calls[2][1]["lost"] == 0 and np.array_equal(calls[2][2], iq[700:740])


def test_lost_records_resynchronise_on_the_next_open():
    fe, sc, calls = make(dict(pre_s=0.0, hang_s=0.0, rec_capacity=2))
    iq, recs = script([(10, 20, 5, 1.0), (100, 30, 6, 1.0), (200, 40, 7, 1.0), (300, 50, 8, 1.0)])
    fe.script[1] = (iq, recs)
    fe.advance(1, 20 + 30 + 10, 5, in_window=1); sc.poll()  # five records behind a ring of two: CLOSE of window 2, OPEN of window 3
    assert len(calls) == 1 and calls[0][1]["lost"] == -1 and calls[0][1]["end"] == 130 and calls[0][1]["n_open"] == 6
    fe.advance(1, 90, 6); sc.poll()
    assert len(calls) == 2 and calls[1][1] == dict(sample=200, end=240, pos=50, n_open=7, peak=1.0, rate=25000.0, lost=0)
    assert np.array_equal(calls[1][2], iq[50:90])
