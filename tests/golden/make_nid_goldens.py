#!/usr/bin/env python3
"""Generate tests/golden/p25_nid.npz by RUNNING the reference's own code, like make_p25es_goldens.py (build container only).

BCH(63,16,23), the code of the P25 NID, is the binary subfield subcode of RS(63,41,23) over GF(64) with x^6 + x + 1, alpha = 2
and the roots alpha^1 .. alpha^22: rs64.Codec(23) of the reference, for which a word of 63 symbols that are all 0 or 1 is a
valid msg.  This runs rs64.Codec(23).decode on such words.  Code words and patterns come from tests/nid_ref.py, whose encoder
is checked here against the reference's first.  Written, data only:
  nid_w      the received word, 63 bits in a uint64, code bit 0 (the nac's first bit) highest
  nid_sent   the 16 data bits sent
  nid_flips  how many bits were flipped
  nid_class  0: a random (code word, pattern) pair -- per weight 0 .. 14, 16, 20 and 31 at least 200, positions 0 and 62
             each in some pattern of every weight >= 1; 1: all 63 single flips of one word; 2 / 3 / 4: for 50 code words c' of
             weight 23 the sent word with 12 / 11 / 13 of c' 's support bits flipped
  nid_other  class 2 .. 4: c'
  nid_ref    the reference's answer: the 16 data bits, -1 for None, -2 for an answer that is not all 0 / 1
  counts     (printed as well) inside the bound: words, answers other than the sent word; beyond: words, None, answers, of
             them answers that differ from the rule (the code word within 11 bits if there is one, else none)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "radiocapture-rf_amd"))
import rs64  # noqa: E402

import nid_ref as N  # noqa: E402

OUT = os.path.join(HERE, "p25_nid.npz")
WEIGHTS = list(range(15)) + [16, 20, 31]
CODEC = rs64.Codec(23)


def symbols(word):
    return bytearray((word >> (62 - i)) & 1 for i in range(63))


def reference(word):
    r = CODEC.decode(symbols(word))
    if r is None:
        return -1
    if len(r) != 41 or any(v > 1 for v in r):
        return -2
    # the answer is the RS code's 41 data symbols; those of a BCH code word are its first 41 bits, the first 16 the data
    full = int("".join(str(v) for v in r), 2)
    return full >> 25 if N.encode(full >> 25) >> 22 == full else -2


def main():
    rng = np.random.default_rng(6323)
    for _ in range(200):                               # the encoder against the reference's: parity of 16 data bits, 25 zeros
        data = int(rng.integers(0, 1 << 16))
        msg = bytearray((data >> (15 - i)) & 1 for i in range(16)) + bytearray(47)
        CODEC.encode(msg)
        # (the RS encoder's parity of a binary word need not be binary: the BCH word is the one the decoder accepts)
        assert not max(CODEC.calculate_syndrome(symbols(N.encode(data))))
    rows = []

    def add(sent, places, cls, other=0):
        w = N.flip(N.encode(sent), places)
        rows.append((w, sent, len(places), cls, other, reference(w)))

    for weight in WEIGHTS:
        for n in range(200):
            first = [] if weight == 0 else [0] if n == 0 else [62] if n == 1 else []
            rest = [p for p in range(63) if p not in first]
            places = first + [int(p) for p in rng.choice(rest, weight - len(first), replace=False)]
            add(int(rng.integers(0, 1 << 16)), places, 0)
    one = int(rng.integers(0, 1 << 16))
    for p in range(63):
        add(one, [p], 1)
    light = np.flatnonzero(N.WEIGHTS == 23)
    assert len(light) == 1890 and N.WEIGHTS[1:].min() == 23
    for at in rng.choice(light, 50, replace=False):
        other = int(N.WORDS[at])
        sent = int(rng.integers(0, 1 << 16))
        for cls, n_flips in ((2, 12), (3, 11), (4, 13)):
            add(sent, [int(p) for p in rng.choice(N.support(other), n_flips, replace=False)], cls, other)
    w, sent, flips, cls, other, ref = (np.array(c) for c in zip(*rows))
    inside = beyond = wrong_inside = none = answered = differs = 0
    for r in rows:
        word, fix = N.decode(r[0])
        rule = word >> 47 if fix != N.BAD else -1
        if r[3] in (0, 1, 3) and r[2] <= 11:
            inside += 1
            wrong_inside += r[5] != r[1]
            assert rule == r[1]
        else:
            beyond += 1
            none += r[5] == -1
            answered += r[5] != -1
            differs += r[5] != rule
    counts = dict(inside=inside, wrong_inside=int(wrong_inside), beyond=beyond, none=int(none), answered=int(answered), differs=int(differs))
    np.savez_compressed(OUT, nid_w=w.astype(np.uint64), nid_sent=sent.astype(np.uint16), nid_flips=flips.astype(np.uint8),
                        nid_class=cls.astype(np.uint8), nid_other=other.astype(np.uint64), nid_ref=ref.astype(np.int32),
                        counts=np.array([counts[k] for k in ("inside", "wrong_inside", "beyond", "none", "answered", "differs")], np.int64))
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(rows), "words;", counts)


if __name__ == "__main__":
    main()
