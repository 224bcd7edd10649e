"""The RCF_T_SLICE leg per block with 256 channels behind one 4800-baud C4FM carrier (400 kS/s front-end, 25 kS/s channels, blocks
of 16000 samples = 192 symbols a channel): slicers alone, with the TSBK stage on TSDUs sent back to back, with the P25 voice stage
on LDU1 / LDU2 sent back to back -- as it always was (p25lc), with LDU2's encryption sync decoded (p25lc+es) and with erasures as
well (p25lc+es+er); +nid on tsbk or p25lc decodes the NID's BCH word first (RCF_NID_BCH).  The package directory names the tree whose rcf package (and librcf.so) is measured, so that a
parent commit's build can stand next to this one's in one session; prints one JSON line (profiles/p25lc_slice_leg.json holds them).
    python tools/slice_leg_probe.py <package dir> <none|tsbk|tsbk+nid|p25lc|p25lc+es|p25lc+es+er|p25lc+nid|p25lc+es+er+nid>"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG, STAGE = os.path.abspath(sys.argv[1]), sys.argv[2]
STAGE, OPTIONS = STAGE.split("+")[0], STAGE.split("+")[1:]
for p in (os.path.join(ROOT, "tests"), PKG):
    sys.path.insert(0, p)
import fsk4_ref as F  # noqa: E402
import tsbk_ref as T  # noqa: E402
from rcf import native as nat, p25  # noqa: E402

FS, CR, OFF = F.FS, F.CHANNEL_RATE, F.CHANNEL_OFFSET
BLK, N_CH, WARM = 16000, 256, 8
rng = np.random.default_rng(3)
settle = np.random.default_rng(25).integers(0, 4, 1000).astype(np.uint8)
if STAGE == "p25lc":
    import p25lc_ref as R  # noqa: E402
    lc = R.lc_group_voice(0x1234, 0xABCDEF)
    frames = []
    for _ in range(7):
        frames += [R.unit_frame(0x293, R.LDU1, lc, rng, lsd=bytes(4)), R.frame(0x293, 0xA, 864, rng)]
else:
    frames = [T.frame(0x293, 7, [T.tsbk_octets(rng) for _ in range(3)], rng) for _ in range(34)]
d = np.concatenate([settle] + frames + [rng.integers(0, 4, 900).astype(np.uint8)])
x = F.c4fm_carrier(d, 4800, FS, OFF + 150.0, 0.5, 600.0)
K = len(x) // BLK
with nat.Frontend(FS, device=0, block_capacity=BLK) as fe:
    cids = []
    for j in range(N_CH):
        c = fe.chan_open(CR, OFF)
        fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
        fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, p25.SLICER_LEVELS, p25.FRAME_SYNC, 48, 4)
        if STAGE == "tsbk":
            fe.chan_tsbk(c, **({"nid": True} if "nid" in OPTIONS else {}))                                    # (no option: a parent's binding too)
        elif STAGE == "p25lc" and "nid" in OPTIONS:
            fe.chan_p25lc_ex(c, es="es" in OPTIONS, erasures="er" in OPTIONS, nid=True)
        elif STAGE == "p25lc":
            fe.chan_p25lc(c, **({"es": "es" in OPTIONS, "erasures": "er" in OPTIONS} if OPTIONS else {}))     # (no option: a parent's binding too)
        cids.append(c)
    fe.timing_enable(True, classes=[nat.T_SLICE])
    for b in range(WARM):
        fe.push(x[b * BLK:(b + 1) * BLK])
    fe.timing_read(nat.T_SLICE)
    per = []
    for b in range(WARM, K):
        fe.push(x[b * BLK:(b + 1) * BLK])
        ms, n = fe.timing_read(nat.T_SLICE)
        per.append(ms)
    st = {} if STAGE == "none" else (fe.chan_tsbk_state(cids[-1]) if STAGE == "tsbk" else fe.chan_p25lc_state(cids[-1]))
per = np.array(per)
print(json.dumps(dict(pkg=os.path.relpath(PKG, ROOT), stage="+".join([STAGE] + OPTIONS), channels=N_CH, blocks=len(per), launches_per_block=int(n),
                      slice_leg_ms_per_block_median=round(float(np.median(per)), 4), min=round(float(per.min()), 4),
                      max=round(float(per.max()), 4), last_channel_state=st)))
