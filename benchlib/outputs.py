"""--dump-outputs DIR: what the timed path computed in its last step, as .npy files two builds can be compared by.

Read right after the timed region (rank 0's front-end), before anything else commits to it:
  pfb_bins.npy        [bins, FRAME_SAMPLE, 2] float32  every bin of the bank's last block, at a fixed, seeded set of
                                                       FRAME_SAMPLE frame indices (the whole block is 256 MB)
  pfb_bins_frames.npy [FRAME_SAMPLE] float64           those frame indices
  chan_iq.npy         [channels, n, 2] float32         each stage-2 channel's newest n = frames / decim IQ outputs
  chan_fm.npy         [channels, n] float32            ... and its discriminator's (gain 1)
The block, the tile and the number of commits before the last step depend on the arguments alone, so the same
arguments give the same inputs run after run."""
import os

import numpy as np

FRAME_SAMPLE = 8192
SEED = 20250


def frame_sample(frames):
    rng = np.random.default_rng(SEED)
    return np.sort(rng.choice(frames, size=min(frames, FRAME_SAMPLE), replace=False))


def _newest(a, n):
    a = np.asarray(a)
    return a[max(len(a) - n, 0):]


def dump_outputs(fe, nb, frames, out_cap, chans, path):
    """-> {name: shape} of what was written under `path`"""
    os.makedirs(path, exist_ok=True)
    idx = frame_sample(frames)
    bins = np.empty((nb, len(idx), 2), dtype=np.float32)
    for b in range(nb):
        last = _newest(fe.pfb_read_bin(b, max_samples=out_cap), frames)
        if len(last) != frames:
            raise RuntimeError("bin %d: %d samples of the last block readable, %d expected" % (b, len(last), frames))
        bins[b] = last[idx].view(np.float32).reshape(-1, 2)
    arrays = {"pfb_bins": bins, "pfb_bins_frames": idx.astype(np.float64)}
    if chans:
        n = min(frames // fe.chan_info(c)["decim"] for c in chans)
        iq = [_newest(fe.chan_read_iq(c, max_samples=out_cap), n) for c in chans]
        fm = [_newest(fe.chan_read_fm(c, 1.0, max_samples=out_cap), n) for c in chans]
        if min(len(x) for x in iq + fm) != n:
            raise RuntimeError("a channel holds fewer than the %d outputs of the last block" % n)
        arrays["chan_iq"] = np.stack(iq).astype(np.complex64).view(np.float32).reshape(len(chans), n, 2)
        arrays["chan_fm"] = np.stack(fm).astype(np.float32)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}
