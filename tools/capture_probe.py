#!/usr/bin/env python3
"""The capture stage's launch beside the carrier detector's under a kernel trace:
   rocprofv3 --kernel-trace --stats -- python tools/capture_probe.py      (capture_kernel against squelch_kernel)

One workload, nothing timed on the host: 2048 direct 12.5 kHz channels of a 400 kS/s front end, 1000 samples each per block
of 16000, rcf_chan_squelch AND rcf_chan_capture on all of them with the same threshold and alpha: one squelch_kernel and one
capture_kernel launch of 32 waves per block, over the same rings, in the same trace.  The noise in a channel stands at the
threshold (-38 dB), so the gates open and close all the time and the write-back has work.  The last stdout line is a JSON object with what the stages saw."""
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


def channels(steps=40, pre=20, hang=30, thr_db=-38.0):
    fs, n_ch, blk = 400e3, 2048, 16000
    x = noise(blk * 4, 2, 0.05)
    with native.Frontend(fs, 0.0, device=0, block_capacity=blk) as fe:
        cids = [fe.chan_open(12500, -190e3 + 185.0 * i) for i in range(n_ch)]
        for c in cids:
            fe.chan_squelch(c, thr_db, 0.1)
            fe.chan_capture(c, thr_db, 0.1, pre=pre, hang=hang)
        for b in range(steps):
            fe.push(x[(b % 4) * blk:(b % 4 + 1) * blk])
        sq = [fe.chan_squelch_state(c) for c in (cids[0], cids[-1])]
        cp = [fe.chan_capture_state(c) for c in cids[::64]]
    return dict(channels=n_ch, samples_per_block=blk // 16, steps=steps, pre=pre, hang=hang, n_seen=[s["n_seen"] for s in sq],
                n_open=[s["n_open"] for s in sq], kept=int(sum(s["n_kept"] for s in cp)), decided=int(sum(s["n_decided"] for s in cp)),
                records=int(sum(s["n_records"] for s in cp)))


if __name__ == "__main__":
    print(json.dumps(dict(channels=channels())))
