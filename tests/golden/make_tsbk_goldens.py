#!/usr/bin/env python3
"""Generate tests/golden/p25_tsdu.npz by RUNNING the reference's own TSDU decoder.

p25_general.procTSDU (with subprocTSBK, procStatus, data_deinterleave, trellis_1_2_decode and crc16, p25_general.py) is
plain Python and imports as it stands.  This generator (build container only) builds frames with an encoder of its OWN --
the trellis run forward, the interleaver as the inverse of the index map, a CRC solved so that the reference's crc16 gives
0 -- and hands the frame bytes to the reference.  Written, data only: the frame bytes, the NID the reference read, how many
blocks it returned per frame (its early stop included) and per returned block the 96 bits it checked (the argument of its
own crc16 call, recorded by a subclass) with its crc, lb, opcode and mfid.

Frames are 360, 576 and 720 bits long -- the three TSDU lengths; procStatus raises on a frame whose last status group is
short --: clean ones, and ones with 1, 2, 4 and 8 flipped bits behind the NID.
"""
import os
import sys

import numpy as np

sys.path.insert(0, "/root/reference")
from p25_general import p25_general  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "p25_tsdu.npz")
SYNC = 0x5575F5FF77FF
W = ((0x2, 0xC, 0x1, 0xF), (0xE, 0x0, 0xD, 0x3), (0x9, 0x7, 0xA, 0x4), (0x5, 0xB, 0x6, 0x8))


class Recorder(p25_general):
    """the reference, with the 96 bits of every crc16 call written down"""
    def __init__(self):
        p25_general.__init__(self)
        self.seen = []

    def crc16(self, dat, len):
        self.seen.append(dat)
        return p25_general.crc16(self, dat, len)


def crc_field(payload_bits):
    """the 16 bits that make the register end at 0xffff behind the 80 payload bits"""
    reg = 0
    for bit in list(payload_bits) + [0] * 16:
        reg = (reg << 1) | int(bit)
        if reg & 0x10000:
            reg = (reg & 0xffff) ^ 0x1021
    return reg ^ 0xffff


def encode_block(rng):
    """80 random bits + CRC -> (the 96 bits, the block's 98 interleaved dibits)"""
    payload = rng.integers(0, 2, 80)
    f = crc_field(payload)
    bits = list(payload) + [(f >> (15 - i)) & 1 for i in range(16)]
    states = [2 * bits[2 * i] + bits[2 * i + 1] for i in range(48)] + [0]     # the flushing dibit
    coded, state = [], 0
    for d in states:
        w = W[state][d]
        coded += [w >> 2, w & 3]
        state = d
    order = []                                                                # deinterleaved dibit n comes from block dibit order[n]
    for i in range(0, 23, 2):
        for j in (0, 26, 50, 74):
            order += [i + j, i + j + 1]
    order += [24, 25]
    block = [0] * 98
    for n, at in enumerate(order):
        block[at] = coded[n]
    return bits, block


def frame_bytes(rng, n_blocks, duid=7):
    """sync, NID (nac, duid, 48 parity bits that nobody checks), n_blocks blocks, null dibits up to the TSDU's length; a
    status dibit behind every 35 info dibits"""
    total = {1: 180, 2: 288, 3: 360}[n_blocks]
    info = [(SYNC >> (46 - 2 * i)) & 3 for i in range(24)]
    nid = (int(rng.integers(0, 4096)) << 52) | (duid << 48) | int(rng.integers(0, 1 << 48))
    info += [(nid >> (62 - 2 * i)) & 3 for i in range(32)]
    sent = []
    for _ in range(n_blocks):
        bits, block = encode_block(rng)
        sent.append(bits)
        info += block
    info += [0] * (total - total // 36 - len(info))
    frame = []
    for j, d in enumerate(info):
        frame.append(d)
        if j % 35 == 34:
            frame.append(int(rng.integers(0, 4)))
    assert len(frame) == total
    bits = np.array([[d >> 1, d & 1] for d in frame], np.uint8).reshape(-1)
    return np.packbits(bits), sent


def main():
    rng = np.random.default_rng(2519)
    frames, lengths, flips_of, counts, nids = [], [], [], [], []
    blk_bits, blk_crc, blk_lb, blk_opcode, blk_mfid = [], [], [], [], []
    clean_returned = {2: [0, 0], 3: [0, 0]}
    for flips, per_length in ((0, 60), (1, 16), (2, 16), (4, 16), (8, 16)):
        for n_blocks in (1, 2, 3):
            for _ in range(per_length):
                by, sent = frame_bytes(rng, n_blocks)
                by = by.copy()
                for at in rng.choice(np.arange(114, 8 * len(by)), flips, replace=False):
                    by[at // 8] ^= 0x80 >> (at % 8)
                ref = Recorder()
                r = ref.procTSDU(bytes(by))
                assert len(ref.seen) == len(r["tsbk"])
                if flips == 0:
                    assert all(t["crc"] == 0 for t in r["tsbk"])
                    assert [[(v >> (95 - i)) & 1 for i in range(96)] for v in ref.seen] == sent[:len(ref.seen)]
                    if n_blocks > 1:
                        clean_returned[n_blocks][0] += len(r["tsbk"]); clean_returned[n_blocks][1] += n_blocks
                frames.append(by); lengths.append(len(by)); flips_of.append(flips); counts.append(len(r["tsbk"]))
                nids.append(int(r["nid"], 16))
                for v, t in zip(ref.seen, r["tsbk"]):
                    blk_bits.append(np.frombuffer(v.to_bytes(12, "big"), np.uint8))
                    blk_crc.append(t["crc"]); blk_lb.append(int(t["lb"])); blk_opcode.append(t["opcode"]); blk_mfid.append(t["mfid"])
    np.savez_compressed(OUT, frames=np.concatenate(frames), lengths=np.array(lengths, np.int32), flips=np.array(flips_of, np.uint8),
                        counts=np.array(counts, np.uint8), nid=np.array(nids, np.uint64), octets=np.stack(blk_bits),
                        crc=np.array(blk_crc, np.uint8), lb=np.array(blk_lb, np.uint8), opcode=np.array(blk_opcode, np.uint8),
                        mfid=np.array(blk_mfid, np.uint8))
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(frames), "frames,", len(blk_crc), "blocks returned; clean frames:",
          {n: "%d of %d" % tuple(v) for n, v in clean_returned.items()})


if __name__ == "__main__":
    main()
