#!/usr/bin/env python3
"""The carrier detector's launches under a kernel trace:
   rocprofv3 --kernel-trace --stats -- python tools/squelch_probe.py      (what do the detector's launches cost?)

Two workloads, nothing timed on the host:
  bank      the 1600-bin / D 800 reference-grid bank of one 20 Msps front end, resident blocks of 2^25 samples (41943 frames),
            rcf_pfb_squelch on every bin: the two passes (pfb_squelch_z_kernel, pfb_squelch_walk_kernel) beside the bank's own
            kernel in the same trace.  Their algorithmic traffic is one read of the block's frames each, 2 x 537 MB, plus the
            z scratch (163 x 1600 doubles written once, read by every later segment of its bin).
  channels  4096 direct 12.5 kHz channels of a 400 kS/s front end, 500 samples each per block of 8000, rcf_chan_squelch on
            all of them: one squelch_kernel launch of 64 waves per block.
SQUELCH_PROBE=bank|channels runs one of them; the last stdout line is a JSON object with what the detectors saw."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "radiocapture-rf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from rcf import native  # noqa: E402


def noise(n, seed, amp):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(2 * n, dtype=np.float32) * np.float32(amp)).view(np.complex64)


def bank(steps=12):
    fs, B = 20e6, 1 << 25
    D, _ = native.channel_params(fs, 12500)
    taps = native.design_low_pass_2(1.0, fs, 6250.0, 6250.0, 20.0)
    tile = noise(1 << 20, 1, 0.05)
    with native.Frontend(fs, 0.0, device=0, block_capacity=B, hist_capacity=1 << 16, out_capacity=1 << 17) as fe:
        fe.pfb_open(1600, D, taps)
        for _ in range(2):                                   # both input buffers
            for at in range(0, B, len(tile)):
                fe.ingest_write(tile, at)
            fe.commit(B)
        fe.pfb_squelch(-70.0, 0.1)                           # (the noise stands near it: bins open and close)
        for _ in range(steps):
            fe.commit(B)
        st = fe.pfb_squelch_read(1600)
    return dict(bins=1600, decim=D, block=B, steps=steps, frames_seen=st["frames_seen"], segment=native.pfb_squelch_segment(),
                open_frames=int(st["n_open"].sum()), bins_ever_open=int((st["n_open"] > 0).sum()))


def channels(steps=40):
    fs, n_ch, blk = 400e3, 4096, 8000
    x = noise(blk * 4, 2, 0.05)
    with native.Frontend(fs, 0.0, device=0, block_capacity=blk) as fe:
        cids = [fe.chan_open(12500, -190e3 + 92.0 * i) for i in range(n_ch)]
        for c in cids:
            fe.chan_squelch(c, -50.0, 0.1)
        for b in range(steps):
            fe.push(x[(b % 4) * blk:(b % 4 + 1) * blk])
        first, last = fe.chan_squelch_state(cids[0]), fe.chan_squelch_state(cids[-1])
    return dict(channels=n_ch, samples_per_block=blk // 16, steps=steps, n_seen=[first["n_seen"], last["n_seen"]],
                n_open=[first["n_open"], last["n_open"]])


if __name__ == "__main__":
    which = os.environ.get("SQUELCH_PROBE", "bank,channels").split(",")
    out = {}
    if "bank" in which:
        out["bank"] = bank()
    if "channels" in which:
        out["channels"] = channels()
    print(json.dumps(out))
