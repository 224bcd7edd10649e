"""The mixed-radix filterbank family (radiocapture-rf_amd/csrc/pfbm.hip: 160, 192, 480, 640, 960, 1280 bins at D = NB / 2)
as far as it can be checked without a device: which shapes librcf accepts and which family serves them, that the family
covers the reference's own source rates, how the receiver routes a 2.4 Msps source with config.pfb_mixed_radix, and the
register butterflies the kernel is built on (fft_core.hpp compiled for the host against a double-precision DFT)."""
import json
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

from oracle import grspec as G
from rcf import native, receiver

from test_host_protocol import StubFrontend, StubPfbFrontend

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (fs, bins, taps): rc_frontend/channel.py:31-33 -- D = int(fs / 12500) / 2, T = odd(int(fs / 6875))
FAMILY = [(2.0e6, 160, 291), (2.4e6, 192, 349), (6e6, 480, 873), (8e6, 640, 1163), (12e6, 960, 1745), (16e6, 1280, 2327)]


def test_the_six_reference_rate_shapes_are_supported_and_family_three():
    for fs, nb, T in FAMILY:
        D, taps = G.channel_params(fs, 12500)
        assert (D, len(taps)) == (nb // 2, T), (fs, D, len(taps))
        assert native.pfb_shape_supported(nb, nb // 2, len(taps)), nb
        assert native.pfb_shape_family(nb, nb // 2, len(taps)) == 3, nb
        assert native.pfb_shape_family(nb, nb // 2, nb) == 3            # one tap per branch: zero padded
    assert native.pfb_shape_family(1600, 800, 2909) == 2
    assert native.pfb_shape_family(256, 256, 3584) == 1
    assert native.pfb_shape_family(228, 114, 415) == 0
    # the family is oversampling 2 with up to two taps per branch, nothing else
    assert native.pfb_shape_family(192, 192, 349) == 0 and not native.pfb_shape_supported(192, 192, 349)
    assert native.pfb_shape_family(192, 96, 3 * 192) == 0 and not native.pfb_shape_supported(192, 96, 3 * 192)
    assert native.pfb_shape_family(192, 48, 192) == 0
    assert native.pfb_shape_family(0, 96, 349) == 0 and native.pfb_shape_family(192, 0, 349) == 0


def test_every_reference_config_rate_on_the_grid_has_a_bank_shape():
    cfgs = json.load(open(os.path.join(HERE, "golden", "reference_configs.json")))
    rates = sorted({int(s["samp_rate"]) for c in cfgs.values() for s in c["sources"] if s.get("samp_rate")})
    assert rates, cfgs
    # (2.85 Msps -- 228 bins = 12 x 19 -- is named beside them as a rate the family leaves out; the recorded configurations
    # carry no such source, so it is asked about here on its own)
    rates = sorted(set(rates) | {2850000})
    without = set()
    for fs in rates:
        nb = fs / 12500.0
        try:
            D, taps = G.channel_params(float(fs), 12500)
        except Exception:
            without.add(fs)
            continue
        ok = nb == int(nb) and int(nb) % D == 0 and native.pfb_shape_supported(int(nb), D, len(taps))
        if nb in (160, 192, 480, 640, 800, 960, 1280):
            assert ok, (fs, nb, D, len(taps))
        if not ok:
            without.add(fs)
    assert without == {2850000, 10666666}, without


def _leak_l2(fs, nb, taps, k):
    """numpy restatement of rcf_pfb_tap_leakage (tests/test_host_protocol.py: test_tap_leakage_matches_the_float32_phase_model)"""
    i = np.arange(len(taps), dtype=np.float64)
    h = taps.astype(np.float64)
    ks = k if k < nb // 2 else k - nb
    fw = np.float32(2 * np.pi * (ks * fs / nb) / fs)
    th = (np.arange(len(taps), dtype=np.float32) * fw).astype(np.float64)
    d = th - 2 * np.pi * ks * i / nb
    c = np.sum(h * h * d) / np.sum(h * h)
    return float(np.sqrt(np.sum(np.abs(h * (np.exp(1j * (d - c)) - 1)) ** 2)))


def test_receiver_opens_a_192_bin_bank_at_2p4_msps_only_with_the_knob():
    fs, nb, fc = 2400000, 192, 855050000
    src = {0: dict(type="synthetic", center_freq=fc, samp_rate=fs)}
    # without the knob: as before the family existed
    tb0 = receiver.receiver(types.SimpleNamespace(sources=src, frontend_mode="pfb"), frontend_factory=StubPfbFrontend)
    assert tb0.sources[0]["pfb"] is None and StubFrontend.instances[-1].pfb is None
    b0, _ = tb0.connect_channel(12500, fc + 12500)
    assert tb0.channels[b0].pfb_bin is None
    assert "rcf_pfb_served_by_bank" not in tb0.metrics()
    # with it
    cfg = types.SimpleNamespace(sources=src, frontend_mode="pfb", pfb_mixed_radix=True)
    tb = receiver.receiver(cfg, frontend_factory=StubPfbFrontend)
    fe = StubFrontend.instances[-1]
    assert fe.pfb == dict(n_bins=192, decim=96, ntaps=349)
    plan = tb.sources[0]["pfb"]
    assert plan["n_bins"] == 192 and plan["grid"] == 12500.0 and plan["decim"] == 96
    par = plan["parity"]
    assert par["budget"] == 1e-4 and par["margin"] == 2.5 and abs(par["gain"] - 25000.0 / (2 * math.pi * 600)) < 1e-9
    D, taps = G.channel_params(float(fs), 12500)
    env = 10 ** (par["env_db"] / 20)
    served, predicted = set(), set()
    for m in range(-95, 96):                                   # every requestable on-grid offset: |offset| < fs / 2
        if m == 0:
            continue
        k = m % nb
        bid, _ = tb.connect_channel(12500, fc + m * 12500)
        ch = tb.channels[bid]
        if ch.pfb_bin is not None:
            assert ch.pfb_bin == k and fe.chans[ch.chan_id]["bin"] == k, (m, ch.pfb_bin)
            served.add(k)
        else:
            assert fe.chans[ch.chan_id]["cr"] == 12500 and fe.chans[ch.chan_id]["off"] == m * 12500
        if par["gain"] * par["margin"] * _leak_l2(float(fs), nb, taps, k) * env <= par["budget"]:
            predicted.add(k)
    bid, _ = tb.connect_channel(12500, fc)                     # the centre: bin 0, no phase rounding at all
    assert tb.channels[bid].pfb_bin == 0
    assert served == predicted
    assert len(served) >= 180, len(served)
    # off the raster and another channel rate: the direct kernel
    b3, _ = tb.connect_channel(12500, fc + 6250)
    assert tb.channels[b3].pfb_bin is None and fe.chans[tb.channels[b3].chan_id]["cr"] == 12500
    b4, _ = tb.connect_channel(6250, fc + 12500)
    assert tb.channels[b4].pfb_bin is None and fe.chans[tb.channels[b4].chan_id]["cr"] == 6250
    m = tb.metrics()
    assert m["rcf_pfb_served_by_bank"] == len(served) + 1
    assert m["rcf_pfb_direct_parity_budget"] == 190 - len(served)
    assert m["rcf_pfb_direct_off_grid"] == 1                    # (the 6.25 kHz channel rate is no bank request at all)
    assert m["rcf_channels_open"] == 193


def test_register_butterflies_against_a_double_precision_dft():
    """Dft<3>, Dft<32> and the prime-factor composites 10, 12, 24, 40 (fft_core.hpp, compiled for the host from the same
    source the kernels include) against a naive double-precision DFT over unit impulses at every input and noise: relative
    rms error <= 1e-6 (float32 butterflies of this depth sit below 1e-7)."""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "fft_butterfly_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc"),
                           os.path.join(HERE, "native", "fft_butterfly_check.cpp"), "-o", exe, "-lm"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = p.stdout.decode()
    assert p.returncode == 0, text
    rows = re.findall(r"R (\d+) sign (-?\d+) relerr (\S+)", text)
    seen = {(int(r), int(s)) for r, s, _ in rows}
    for r in (3, 10, 12, 24, 32, 40):
        assert (r, 1) in seen and (r, -1) in seen, text
    for r, s, e in rows:
        assert float(e) <= 1e-6, (r, s, e)
