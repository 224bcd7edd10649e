"""bench.py's plain run on the device: the K timed steps and one line, and --dump-outputs writing what the last of them
computed -- the same arrays, bit for bit, from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 1 << 22


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--block", str(BLOCK),
                        "--prewarm-steps", "16", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_dumps_the_same_outputs_twice(gpu_required, tmp_path):
    a, b = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and "sustained" not in d
    frames = BLOCK // 256
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["chan_fm.npy", "chan_iq.npy", "pfb_bins.npy", "pfb_bins_frames.npy"]
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y, err_msg=n)
    bins = np.load(tmp_path / "a" / "pfb_bins.npy")
    fm = np.load(tmp_path / "a" / "chan_fm.npy")
    assert bins.shape == (256, 8192, 2) and fm.shape == (32, frames // 3)
    assert np.abs(bins).max() > 0 and np.abs(fm).max() > 0        # the stream's carriers came through
