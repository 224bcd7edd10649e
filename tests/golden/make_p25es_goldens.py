#!/usr/bin/env python3
"""Generate tests/golden/p25_es.npz by RUNNING the reference's own code, like make_p25lc_goldens.py (build container only).

rs64.Codec(9), Codec(13) and Codec(17) encode and decode, with and without their `erasures` list; hamming.py and golay.py
beside them; p25_general's stubs hamming_10_6_3_decode and rs_24_16_9_decode composed over procLDU1's slices, which is what an
LDU2's encryption sync is to the reference (its procLDU2 is empty).  Frames and code words come from the encoders of
tests/p25lc_ref.py and tests/p25es_ref.py, checked here against the reference's first.  Written, data only:
  (a) rs<d>_*: per code RS(24,16,9), RS(24,12,13), RS(36,20,17) words with e erased symbols and v errors elsewhere for every
      pair with d - 2 <= 2 v + e <= d + 1 -- just inside the bound, on it, one and two steps beyond -- 24 words a pair, the
      erased symbols all wrong; for every pair on the bound with e > 0 another 8 words whose erased symbols are right at every
      second place; for (0, t) and (d - 1, 0) 16 words each whose positions cover symbol 0 and symbol n - 1.  Stored: the
      received symbols, the sent code word, the erased positions as a mask, e, v, whether decode(msg, erasures) answered None,
      and the data it returned
  (b) ldu2_*: LDU2 frame bytes, clean and with 1, 2, 4, 8 and 16 flipped bits behind the NID, and the 96 bits
      rs_24_16_9_decode(hamming_10_6_3_decode(lc)) gave for procLDU1's slices of them, with the nid and lsd procLDU1 returned
  (c) golay_par_*: (24,12) words with three and four errors among all 24 bits: golay.decode_lc's answer (-1: None) and the
      24th bit golay.encode_lc gives that answer
"""
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

import p25es_ref as E  # noqa: E402
import p25lc_ref as R  # noqa: E402

OUT = os.path.join(HERE, "p25_es.npz")
CODES = (("9", 24, 16), ("13", 24, 12), ("17", 36, 20))


def check_encoders(rng):
    for name, n, k in CODES:
        codec = rs64.Codec(int(name))
        for _ in range(50):
            data = [int(v) for v in rng.integers(0, 64, k)]
            msg = bytearray(data) + bytearray(n - k)
            codec.encode(msg)
            assert R.rs_encode(data, n, k) == list(msg)
    for d in range(64):
        assert R.hamming_encode(d) == hamming.encode_lc(d)
    for d in range(4096):
        assert golay.encode_lc(d) & 1 == bin(int(R.GOLAY23[d])).count("1") & 1 and golay.encode_lc(d) >> 1 == int(R.GOLAY23[d])


def rs_cases(rng):
    g = {}
    for name, n, k in CODES:
        codec, d = rs64.Codec(int(name)), int(name)
        t = (d - 1) // 2
        rows = []

        def add(e, v, erased, errors, right=()):
            cw = R.rs_encode([int(x) for x in rng.integers(0, 64, k)], n, k)
            w = list(cw)
            for at in list(erased) + list(errors):
                if at not in right:
                    w[at] ^= int(rng.integers(1, 64))
            r = codec.decode(bytearray(w), [int(at) for at in erased]) if len(erased) else codec.decode(bytearray(w))
            mask = np.zeros(n, np.uint8)
            mask[list(erased)] = 1
            rows.append((w, cw, mask, e, v, r is None, [0] * k if r is None else list(r)))

        def places(e, v, first=()):
            rest = [int(x) for x in rng.permutation(n) if int(x) not in first]
            at = list(first) + rest
            return at[:e], at[e:e + v]

        for total in range(d - 2, d + 2):
            for v in range(total // 2 + 1):
                e = total - 2 * v
                if e + v > n:
                    continue
                for _ in range(24):
                    add(e, v, *places(e, v))
        for v in range(t):                             # on the bound, e > 0: erased symbols that are right
            e = d - 1 - 2 * v
            for _ in range(8):
                erased, errors = places(e, v)
                add(e, v, erased, errors, right=erased[::2])
        for _ in range(16):
            add(0, t, *places(0, t, first=(0, n - 1)))
            add(d - 1, 0, *places(d - 1, 0, first=(0, n - 1)))
        g["rs%s_w" % name] = np.array([r[0] for r in rows], np.uint8)
        g["rs%s_sent" % name] = np.array([r[1] for r in rows], np.uint8)
        g["rs%s_erased" % name] = np.stack([r[2] for r in rows])
        g["rs%s_e" % name] = np.array([r[3] for r in rows], np.uint8)
        g["rs%s_v" % name] = np.array([r[4] for r in rows], np.uint8)
        g["rs%s_none" % name] = np.array([r[5] for r in rows], np.uint8)
        g["rs%s_data" % name] = np.array([r[6] for r in rows], np.uint8)
    return g


def ldu2_frames(rng):
    ref = p25_general()
    ref.subprocLC = lambda lc: lc                      # procLDU1 hands its Hamming-"decoded" 144 bits on as they are
    frames, flips_of, nid, es, lsd = [], [], [], [], []
    for flips, count in ((0, 20), (1, 10), (2, 10), (4, 10), (8, 10), (16, 10)):
        for _ in range(count):
            octets = bytes(rng.integers(0, 256, 12).astype(np.uint8))
            d = E.unit_frame(int(rng.integers(0, 4096)), E.LDU2, octets, rng, lsd=bytes(rng.integers(0, 256, 4).astype(np.uint8)))
            by = np.packbits(np.stack([d >> 1, d & 1], axis=1).reshape(-1)).copy()
            for at in rng.choice(np.arange(114, 8 * len(by)), flips, replace=False):
                by[at // 8] ^= 0x80 >> (at % 8)
            r = ref.procLDU1(bytes(by))
            bits = ref.rs_24_16_9_decode(r["lc"])
            assert len(bits) == 96 and (flips or int(bits, 2).to_bytes(12, "big") == octets)
            frames.append(by); flips_of.append(flips); nid.append(int(r["nid"], 16))
            es.append(np.frombuffer(int(bits, 2).to_bytes(12, "big"), np.uint8))
            lsd.append(np.frombuffer(int(r["lsd"], 2).to_bytes(4, "big"), np.uint8))
    return dict(ldu2_frames=np.stack(frames), ldu2_flips=np.array(flips_of, np.uint8), ldu2_nid=np.array(nid, np.uint64),
                ldu2_es=np.stack(es), ldu2_lsd=np.stack(lsd))


def golay_parity_cases(rng):
    words, ans, bit = [], [], []
    for n in range(3000):
        d = int(rng.integers(0, 4096))
        w = R.golay24_encode(d) ^ sum(1 << int(p) for p in rng.choice(24, 3 + n % 2, replace=False))
        r = golay.decode_lc(w)
        words.append(w); ans.append(-1 if r is None else r); bit.append(-1 if r is None else golay.encode_lc(r) & 1)
    return dict(golay_par_w=np.array(words, np.uint32), golay_par_ref=np.array(ans, np.int16), golay_par_bit=np.array(bit, np.int8))


def main():
    rng = np.random.default_rng(2594)
    check_encoders(rng)
    g = rs_cases(rng)
    g.update(ldu2_frames(rng))
    g.update(golay_parity_cases(rng))
    np.savez_compressed(OUT, **g)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    for name, n, k in CODES:
        d = int(name)
        inside = g["rs%s_e" % name].astype(int) + 2 * g["rs%s_v" % name].astype(int) <= d - 1
        none = g["rs%s_none" % name].astype(bool)
        print("RS d = %s: %d words, %d inside the bound of which None %d; beyond: %d of which answered %d" %
              (name, len(none), inside.sum(), (none & inside).sum(), (~inside).sum(), (~none & ~inside).sum()))


if __name__ == "__main__":
    main()
