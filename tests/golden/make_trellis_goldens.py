#!/usr/bin/env python3
"""Generate tests/golden/p25_trellis.npz by RUNNING the reference's own TSBK block decoder.

The pieces of p25_general.subprocTSBK -- data_deinterleave, trellis_1_2_decode, dibits_to_bit, crc16 (p25_general.py) -- are
plain Python and import as they stand.  This generator (build container only) encodes blocks with an encoder of its OWN --
the trellis run forward with the flushing dibit, the interleaver as the inverse of the index map, a CRC solved so that the
reference's crc16 gives 0 --, flips channel bits of the block's 196 and hands the 98 received dibits to those pieces in
subprocTSBK's order.  Written, data only, per block: the 12 sent octets, the 98 received dibits (packed, the first bit
highest), the 96 bits the reference decoded, its crc (0 good / 1 bad, as subprocTSBK sets it), the number of flipped bits
and the class.  What the reference answered is recorded whether or not it is right.

Classes: 0 clean; 1 every one of the 196 single flips of two blocks; 2 2000 random double flips; 3 500 each of 3, 4, 6 and 8
random flips; 4 bursts of 4 and of 8 adjacent channel bits (100 each), which the deinterleaver spreads over code words.
The sent blocks come from a pool of 12, so that the file stays small.
"""
import os
import sys

import numpy as np

sys.path.insert(0, "/root/reference")
from p25_general import p25_general  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "p25_trellis.npz")
W = ((0x2, 0xC, 0x1, 0xF), (0xE, 0x0, 0xD, 0x3), (0x9, 0x7, 0xA, 0x4), (0x5, 0xB, 0x6, 0x8))


def crc_field(payload_bits):
    """the 16 bits that make the register end at 0xffff behind the 80 payload bits"""
    reg = 0
    for bit in list(payload_bits) + [0] * 16:
        reg = (reg << 1) | int(bit)
        if reg & 0x10000:
            reg = (reg & 0xffff) ^ 0x1021
    return reg ^ 0xffff


def encode_block(rng):
    """80 random bits + CRC -> (the 96 bits, the block's 196 channel bits)"""
    payload = rng.integers(0, 2, 80)
    f = crc_field(payload)
    bits = [int(v) for v in payload] + [(f >> (15 - i)) & 1 for i in range(16)]
    coded, state = [], 0
    for d in [2 * bits[2 * i] + bits[2 * i + 1] for i in range(48)] + [0]:        # the flushing dibit
        w = W[state][d]
        coded += [w >> 2, w & 3]
        state = d
    order = []                                                                    # deinterleaved dibit n comes from block dibit order[n]
    for i in range(0, 23, 2):
        for j in (0, 26, 50, 74):
            order += [i + j, i + j + 1]
    order += [24, 25]
    block = [0] * 98
    for n, at in enumerate(order):
        block[at] = coded[n]
    return bits, [v for d in block for v in (d >> 1, d & 1)]


def reference_answer(ref, channel_bits):
    """subprocTSBK's steps on a block's 196 bits -> (the 96 decoded bits, crc)"""
    dibits = ref.bits_to_dibit("".join(str(b) for b in channel_bits))
    dibits = ref.data_deinterleave(dibits)
    bitframe = ref.dibits_to_bit(ref.trellis_1_2_decode(dibits))
    assert len(bitframe) == 96
    return [int(c) for c in bitframe], 0 if ref.crc16(int(bitframe, 2), 12) == 0 else 1


def main():
    rng = np.random.default_rng(4211)
    ref = p25_general()
    pool = [encode_block(rng) for _ in range(12)]
    jobs = [(0, n, []) for n in range(12)]
    jobs += [(1, n, [q]) for n in (0, 1) for q in range(196)]
    jobs += [(2, int(rng.integers(0, 12)), sorted(rng.choice(196, 2, replace=False).tolist())) for _ in range(2000)]
    for w in (3, 4, 6, 8):
        jobs += [(3, int(rng.integers(0, 12)), sorted(rng.choice(196, w, replace=False).tolist())) for _ in range(500)]
    for w in (4, 8):
        jobs += [(4, int(rng.integers(0, 12)), list(range(at, at + w))) for at in rng.integers(0, 197 - w, 100).tolist()]
    jobs.sort(key=lambda j: (j[0], len(j[2]), j[1], j[2]))
    sent, received, answer, crc, flips, cls = [], [], [], [], [], []
    right = {}
    for c, n, places in jobs:
        bits, channel = pool[n]
        got = list(channel)
        for q in places:
            got[q] ^= 1
        out, bad = reference_answer(ref, got)
        if not places:
            assert out == bits and bad == 0
        sent.append(np.packbits(np.array(bits, np.uint8))); received.append(np.packbits(np.array(got + [0] * 4, np.uint8)))
        answer.append(np.packbits(np.array(out, np.uint8))); crc.append(bad); flips.append(len(places)); cls.append(c)
        key = (c, len(places))
        right.setdefault(key, [0, 0])
        right[key][0] += out == bits; right[key][1] += 1
    np.savez_compressed(OUT, sent=np.stack(sent), received=np.stack(received), ref=np.stack(answer), crc=np.array(crc, np.uint8),
                        flips=np.array(flips, np.uint8), cls=np.array(cls, np.uint8))
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(jobs), "blocks; the reference right per (class, flips):",
          {k: "%d of %d" % tuple(v) for k, v in sorted(right.items())})


if __name__ == "__main__":
    main()
