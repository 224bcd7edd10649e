#!/usr/bin/env python3
"""The mixed-radix banks (pfbm.hip: 160 .. 1280 bins, D = NB / 2, the reference's channel filter) on one device, input
resident, blocks of 2^22 samples, 20 warm-up blocks, 50 timed ones (HIP events, rcf_timing_read):
  bank_ms     the filterbank launch per block (RCF_T_PFB)
  direct_ms   the same outputs the only other way there is: NB - 1 direct channels at every grid offset (RCF_T_FIR_MFMA)
  frac        24 B x samples / bank_ms / 8 TB/s, beside the 400-bin bank (pfb5.hip) of the same run
and the grouped point: ten 192-bin members with 48 000-sample blocks, one grouped launch against ten single ones.
Writes profiles/pfbm_banks.json (or the path given)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radiocapture-rf_amd")]
import numpy as np
from rcf import native

B, WARM, TIMED = 1 << 22, 20, 50
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pfbm_banks.json")
rng = np.random.default_rng(1)
tile = (rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)).astype(np.complex64)


def resident(fe):
    for _ in range(2):                                       # both input buffers
        for at in range(0, B, len(tile)):
            fe.ingest_write(tile, at)
        fe.commit(B)


def timed(fe, classes):
    for _ in range(WARM):
        fe.commit(B)
    fe.sync()
    fe.timing_enable(True, classes=classes)
    for c in classes:
        fe.timing_read(c)
    for _ in range(TIMED):
        fe.commit(B)
    fe.sync()
    out = {}
    for c in classes:
        ms, n = fe.timing_read(c)
        out[c] = (ms / TIMED, n)
    fe.timing_enable(False)
    return out


def bank(fs, nb):
    D, T = native.channel_params(fs, 12500)
    assert D * 2 == nb
    taps = native.design_low_pass_2(1.0, fs, 6250.0, 6250.0, 20.0)
    with native.Frontend(fs, block_capacity=B, hist_capacity=1 << 16, out_capacity=1 << 16) as fe:
        fe.pfb_open(nb, D, taps)
        resident(fe)
        ms, n = timed(fe, [native.T_PFB])[native.T_PFB]
    assert n == TIMED, n
    return D, T, ms


def direct(fs, nb):
    with native.Frontend(fs, block_capacity=B, hist_capacity=1 << 16, out_capacity=1 << 16) as fe:
        for k in range(nb):
            if k == nb // 2:                                   # (-fs/2 is no channel offset)
                continue
            fe.chan_open(12500, (k if k < nb // 2 else k - nb) * fs / nb)
        resident(fe)
        t = timed(fe, [native.T_FIR_MFMA, native.T_FIR])
    return t[native.T_FIR_MFMA][0], t[native.T_FIR_MFMA][1], t[native.T_FIR][0]


rows = []
_, _, ms400 = bank(5e6, 400)
frac400 = 24.0 * B / (ms400 * 1e-3) / 8e12
print("400 bins (pfb5.hip): %.4f ms  frac %.3f" % (ms400, frac400), flush=True)
for fs, nb in ((2.0e6, 160), (2.4e6, 192), (6e6, 480), (8e6, 640), (12e6, 960), (16e6, 1280)):
    D, T, ms = bank(fs, nb)
    d_ms, d_n, d_vec = direct(fs, nb)
    frac = 24.0 * B / (ms * 1e-3) / 8e12
    rows.append({"fs": fs, "bins": nb, "decim": D, "taps": T, "bank_ms": ms, "direct_ms": d_ms, "direct_launches": d_n,
                 "direct_vector_fir_ms": d_vec, "direct_over_bank": d_ms / ms, "frac": frac, "frac_over_400_bins": frac / frac400,
                 "msps": B / ms / 1e3, "x_realtime": B / (ms * 1e-3) / fs})
    print("%4d bins D=%d T=%d: bank %.4f ms  direct %.3f ms (x%.0f)  frac %.3f (400 bins: %.3f)"
          % (nb, D, T, ms, d_ms, d_ms / ms, frac, frac400), flush=True)
    assert ms < d_ms, (nb, ms, d_ms)

# the grouped point
fs, nb, G_, blk = 2.4e6, 192, 10, 48000
D, T = native.channel_params(fs, 12500)
taps = native.design_low_pass_2(1.0, fs, 6250.0, 6250.0, 20.0)
blocks = [(rng.standard_normal(blk) + 1j * rng.standard_normal(blk)).astype(np.complex64) for _ in range(G_)]


def members():
    fes = [native.Frontend(fs, 0.0, device=0, block_capacity=blk, hist_capacity=1 << 12, out_capacity=1 << 11) for _ in range(G_)]
    for fe in fes:
        fe.pfb_open(nb, D, taps)
    return fes


fes = members()
singles = 0.0
for fe, x in zip(fes, blocks):
    for _ in range(WARM):
        fe.push(x)
    fe.timing_enable(True, classes=[native.T_PFB]); fe.timing_read(native.T_PFB)
    for _ in range(TIMED):
        fe.push(x)
    fe.sync()
    ms, n = fe.timing_read(native.T_PFB)
    singles += ms / n
    fe.close()
fes = members()
grp = native.Group(fes)
for _ in range(WARM):
    grp.push(blocks)
grp.sync()
for fe in fes:
    fe.timing_enable(True, classes=[native.T_PFB]); fe.timing_read(native.T_PFB)
for _ in range(TIMED):
    grp.push(blocks)
grp.sync()
g_ms, g_n = 0.0, 0
for fe in fes:
    ms, n = fe.timing_read(native.T_PFB)
    g_ms += ms
    g_n += n
grp.close()
for fe in fes:
    fe.close()
group = {"members": G_, "bins": nb, "block_samples": blk, "grouped_launch_ms": g_ms / TIMED, "launches_per_block": g_n / TIMED,
         "sum_of_single_launches_ms": singles, "single_over_grouped": singles / (g_ms / TIMED)}
print("group of %d x %d bins, %d-sample blocks: grouped %.4f ms (%.2f launches per block), ten single launches %.4f ms"
      % (G_, nb, blk, g_ms / TIMED, g_n / TIMED, singles), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump({"device": "MI355X", "block_samples": B, "warmup_blocks": WARM, "timed_blocks": TIMED,
               "bytes_per_input_sample": 24, "hbm_peak_bytes_per_s": 8e12,
               "bank_400_bins": {"bank_ms": ms400, "frac": frac400}, "shapes": rows, "group_192": group}, fh, indent=1)
