#!/usr/bin/env python3
"""Generate tests/golden/p25_voice.npz by RUNNING the reference's own voice-channel code.

p25_general.procHDU / procLDU1 / procTLC (p25_general.py) and the codecs beside it -- hamming.py, golay.py, rs64.py, which
logging_receiver.py imports -- are plain Python and import as they stand.  This generator (build container only) builds
frames and code words with an encoder of its OWN (tests/p25lc_ref.py: checked here against the reference's encoders first)
and hands them to the reference.  Written, data only:
  (a) frames: HDU, LDU1 and TLC frame bytes, clean and with 1, 2, 4, 8 and 16 flipped bits behind the NID, and the fields
      procHDU / procLDU1 / procTLC returned for them
  (b) hamming: hamming.decode_lc(w, True) for all 1024 words (-1: None)
  (c) golay: golay.decode_lc for six code words under every error pattern of weight <= 3 in the first 23 bits, for 2000
      random words with 4 errors there, and for 2000 (18,6) words (six leading zero data bits) with <= 3 errors in their
      first 17 bits (-1: None), each with the data sent
  (d) rs: rs64.decode_lc / rs64.Codec(17).decode for 200 random code words per error count 0 .. t + 2 of (24,12,13) and
      (36,20,17): the received symbols, whether the answer was None, and the answer xor the received data symbols
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "radiocapture-rf_amd"))
import golay  # noqa: E402
import hamming  # noqa: E402
import rs64  # noqa: E402
from p25_general import p25_general  # noqa: E402

import p25lc_ref as R  # noqa: E402

OUT = os.path.join(HERE, "p25_voice.npz")


def check_encoders(rng):
    for d in range(4096):
        assert R.golay24_encode(d) == golay.encode_lc(d)
    for d in range(64):
        assert R.hamming_encode(d) == hamming.encode_lc(d)
    c17 = rs64.Codec(17)
    for _ in range(50):
        data = [int(v) for v in rng.integers(0, 64, 12)]
        assert R.rs_encode(data, 24, 12) == list(rs64.encode_lc(bytearray(data)))
        data = [int(v) for v in rng.integers(0, 64, 20)]
        msg = bytearray(data) + bytearray(16)
        c17.encode(msg)
        assert R.rs_encode(data, 36, 20) == list(msg)


def lc_fields(lc):
    return [lc["lcf"], lc["mfid"], int(lc.get("emergency", "0") or 0), lc.get("tgid", 0), lc.get("source_id", 0), int("lcf_long" in lc)]


def frames(rng):
    ref = p25_general()
    out = dict(frames=[], lengths=[], kind=[], flips=[], nid=[], hdu_mi=[], hdu=[], lc=[], lsd=[])
    for kind in (R.HDU, R.LDU1, R.TLC):
        for flips, count in ((0, 20), (1, 10), (2, 10), (4, 10), (8, 10), (16, 10)):
            for n in range(count):
                if kind == R.HDU:
                    octets = bytes(rng.integers(0, 256, 15).astype(np.uint8))
                elif n % 2:
                    octets = R.lc_group_voice(int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 24)), int(rng.integers(0, 2)))
                else:
                    octets = R.LC_TERMINATION if n % 4 == 0 else bytes(rng.integers(0, 256, 9).astype(np.uint8))
                d = R.unit_frame(int(rng.integers(0, 4096)), kind, octets, rng, lsd=bytes(rng.integers(0, 256, 4).astype(np.uint8)))
                by = np.packbits(np.stack([d >> 1, d & 1], axis=1).reshape(-1)).copy()
                for at in rng.choice(np.arange(114, 8 * len(by)), flips, replace=False):
                    by[at // 8] ^= 0x80 >> (at % 8)
                r = (ref.procHDU, ref.procLDU1, ref.procTLC)[kind](bytes(by))
                out["frames"].append(by); out["lengths"].append(len(by)); out["kind"].append(kind); out["flips"].append(flips)
                out["nid"].append(int(r["nid"], 16))
                if kind == R.HDU:
                    if flips == 0:
                        assert int(r["mi"], 2).to_bytes(9, "big") + bytes([r["mfid"], r["algid"]]) + r["kid"].to_bytes(2, "big") + r["tgid"].to_bytes(2, "big") == octets
                    out["hdu_mi"].append(np.frombuffer(int(r["mi"], 2).to_bytes(9, "big"), np.uint8))
                    out["hdu"].append([r["mfid"], r["algid"], r["kid"], r["tgid"]])
                else:
                    if flips == 0 and octets[0] == 0:
                        assert (r["lc"]["tgid"], r["lc"]["source_id"]) == (int.from_bytes(octets[4:6], "big"), int.from_bytes(octets[6:9], "big"))
                    out["lc"].append(lc_fields(r["lc"]))
                    if kind == R.LDU1:
                        out["lsd"].append(np.frombuffer(int(r["lsd"], 2).to_bytes(4, "big"), np.uint8))
    return dict(frames=np.concatenate(out["frames"]), lengths=np.array(out["lengths"], np.int32), kind=np.array(out["kind"], np.uint8),
                flips=np.array(out["flips"], np.uint8), nid=np.array(out["nid"], np.uint64), hdu_mi=np.stack(out["hdu_mi"]),
                hdu=np.array(out["hdu"], np.int32), lc=np.array(out["lc"], np.int32), lsd=np.stack(out["lsd"]))


def golay_cases(rng):
    def answer(w):
        r = golay.decode_lc(int(w))
        return -1 if r is None else r

    patterns = [0] + [sum(1 << p for p in c) << 1 for n in (1, 2, 3) for c in itertools.combinations(range(23), n)]
    assert len(patterns) == 2048
    le3_w, le3_sent = [], []
    for d in [0, 0xfff] + [int(v) for v in rng.integers(0, 4096, 4)]:
        le3_w += [R.golay24_encode(d) ^ p for p in patterns]
        le3_sent += [d] * len(patterns)
    four_w, four_sent = [], []
    for _ in range(2000):
        d = int(rng.integers(0, 4096))
        four_w.append(R.golay24_encode(d) ^ sum(1 << (1 + int(p)) for p in rng.choice(23, 4, replace=False)))
        four_sent.append(d)
    short_w, short_sent = [], []
    for n in range(2000):
        d = int(rng.integers(0, 64))
        short_w.append(R.golay18_encode(d) ^ sum(1 << (1 + int(p)) for p in rng.choice(17, n % 4, replace=False)))
        short_sent.append(d)
    g = {}
    for name, w, sent in (("le3", le3_w, le3_sent), ("four", four_w, four_sent), ("short", short_w, short_sent)):
        g["golay_%s_w" % name] = np.array(w, np.uint32)
        g["golay_%s_sent" % name] = np.array(sent, np.int16)
        g["golay_%s_ref" % name] = np.array([answer(v) for v in w], np.int16)
    return g


def rs_cases(rng):
    g = {}
    for name, n, k, decode in (("24", 24, 12, rs64.decode_lc), ("36", 36, 20, rs64.Codec(17).decode)):
        t = (n - k) // 2
        words, none, fix, errors = [], [], [], []
        for n_err in range(t + 3):
            for _ in range(200):
                cw = R.rs_encode([int(v) for v in rng.integers(0, 64, k)], n, k)
                for at in rng.choice(n, n_err, replace=False):
                    cw[int(at)] ^= int(rng.integers(1, 64))
                r = decode(bytearray(cw))
                words.append(cw); errors.append(n_err); none.append(r is None)
                fix.append([0] * k if r is None else [a ^ b for a, b in zip(r, cw[:k])])
        g["rs%s_w" % name] = np.array(words, np.uint8)
        g["rs%s_none" % name] = np.array(none, np.uint8)
        g["rs%s_fix" % name] = np.array(fix, np.uint8)
        g["rs%s_errors" % name] = np.array(errors, np.uint8)
    return g


def main():
    rng = np.random.default_rng(2520)
    check_encoders(rng)
    g = frames(rng)
    g["hamming_ref"] = np.array([-1 if (r := hamming.decode_lc(w, True)) is None else r for w in range(1024)], np.int16)
    g.update(golay_cases(rng))
    g.update(rs_cases(rng))
    np.savez_compressed(OUT, **g)
    le3 = g["golay_le3_ref"]
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(g["lengths"]), "frames; golay None on <= 3 errors:",
          int(np.sum(le3 < 0)), "of", len(le3), "and", int(np.sum(g["golay_short_ref"] < 0)), "of 2000 (18,6) words; rs None:",
          {n: int(np.sum(g["rs%s_none" % n])) for n in ("24", "36")})


if __name__ == "__main__":
    main()
