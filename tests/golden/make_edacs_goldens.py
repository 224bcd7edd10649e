#!/usr/bin/env python3
"""Generate tests/golden/edacs_frames.npz by RUNNING the reference's own EDACS framer and decoder.

edacs_control_demod.py's get_next_frame, packet_framer, message_election and bch_decode are plain Python string work; the
module imports with GNU Radio, redis and the connectors replaced by stand-ins (build container only: needs /root/reference),
and the four methods run on an instance that was never constructed.  A subclass writes down every bch_decode result.  Frames
come from an encoder of this generator's OWN: systematic, g(x) = (x^6 + x + 1)(x^6 + x^4 + x^2 + x + 1) = 0x1539, 28 message
bits and 12 parity bits.  Written, data only: per frame its 240 bits, esk, m1 and m2 as returned, and per copy the decoded
string and loc; and for get_next_frame buffers of one polarity with the frame it cut out.

Kinds of frames: 0 clean; 1 one or two flipped bits in every copy; 2 copies that differ (one copy of a message is another
valid word); 3 three or four flips in one or more copies -- the reference answers those with a failure, a miscorrection or
the word as received, all three occur --; 4 every copy of a message broken.
"""
import os
import sys
import time
import types
from unittest import mock

import numpy as np

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "edacs_frames.npz")
GEN = 0x1539


class _TopBlock:
    def __init__(self, *a, **k): pass


gr = mock.MagicMock()
gr.top_block = _TopBlock
gnuradio = types.ModuleType("gnuradio")
gnuradio.gr = gr
subs = ("filter", "blocks", "zeromq", "analog", "digital")
for name in subs:
    setattr(gnuradio, name, mock.MagicMock())
sys.modules["gnuradio"] = gnuradio
sys.modules["gnuradio.gr"] = gr
for name in subs:
    sys.modules["gnuradio." + name] = getattr(gnuradio, name)
sys.modules["gnuradio.filter.firdes"] = gnuradio.filter.firdes
for name in ("setproctitle", "frontend_connector", "redis_demod_publisher", "redis_channelizer_manager", "client_redis"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF)
from edacs_control_demod import edacs_control_demod  # noqa: E402


class Recorder(edacs_control_demod):
    """the reference, with every bch_decode result written down"""
    def bch_decode(self, recd):
        r = edacs_control_demod.bch_decode(self, recd)
        self.seen.append((recd, r[0], list(r[1])))
        return r


def reference():
    ref = object.__new__(Recorder)
    ref.seen = []
    ref.framesync = "010101010101010101010111000100100101010101010101"
    ref.failed_loops = 0
    ref.loop_start = time.time()
    ref.log = mock.MagicMock()
    ref.is_locked = False
    return ref


def encode(msg28):
    reg = 0
    for b in list(msg28) + [0] * 12:
        reg = (reg << 1) | int(b)
        if reg & 0x1000:
            reg ^= GEN
    return [int(b) for b in msg28] + [(reg >> (11 - i)) & 1 for i in range(12)]


def frame_bits(copies):
    """six 40-bit copies -> the 240 bits as sent: the middle copy of each three inverted"""
    out = []
    for c, w in enumerate(copies):
        out += [b ^ 1 for b in w] if c in (1, 4) else list(w)
    return out


def flipped(word, rng, n):
    w = list(word)
    for at in rng.choice(40, n, replace=False):
        w[at] ^= 1
    return w


def s(bits):
    return "".join(str(int(b)) for b in bits)


def pack40(string):
    return np.packbits(np.array([int(c) for c in string], np.uint8))


def main():
    rng = np.random.default_rng(4836)
    ref = reference()
    word = lambda: encode(rng.integers(0, 2, 28))
    # the encoder makes words the reference calls clean
    for _ in range(200):
        w = word()
        assert edacs_control_demod.bch_decode(ref, "00000000" + s(w)) == ("00000000" + s(w), [])
    made = []                                          # (kind, copies, the two clean words)
    for _ in range(60):
        a, b = word(), word()
        made.append((0, [a, a, a, b, b, b], a, b))
    for _ in range(90):
        a, b = word(), word()
        made.append((1, [flipped(a, rng, int(rng.integers(0, 3))) for _ in range(3)] + [flipped(b, rng, int(rng.integers(1, 3))) for _ in range(3)], a, b))
    for _ in range(50):
        a, b, x = word(), word(), word()
        copies = [a, a, a, b, b, b]
        copies[int(rng.integers(0, 6))] = x            # outvoted; or, with a second one, no two agree
        if rng.integers(0, 3) == 0:
            copies[int(rng.integers(0, 6))] = word()
        made.append((2, copies, a, b))
    for _ in range(140):
        a, b = word(), word()
        copies = [a, a, a, b, b, b]
        for c in rng.choice(6, int(rng.integers(1, 4)), replace=False):
            copies[c] = flipped(copies[c], rng, int(rng.integers(3, 5)))
        made.append((3, copies, a, b))
    for _ in range(40):
        a, b = word(), word()
        copies = [flipped(a, rng, 3 + int(rng.integers(0, 6))) for _ in range(3)] + [b, flipped(b, rng, 1), b]
        if rng.integers(0, 2):
            copies = copies[3:] + copies[:3]
        made.append((4, copies, a, b))
    kinds, data, esks, ms, has, dec, ok, locs, nloc = [], [], [], [], [], [], [], [], []
    outcomes = dict(fail=0, miscorrected=0, as_received=0)
    recovered = [0, 0]
    for n, (kind, copies, a, b) in enumerate(made):
        bits = frame_bits(copies)
        esk = n % 5 == 4
        ref.seen = []
        m1, m2, bad, total = ref.packet_framer({"esk": esk}, s(bits), 0, 0)
        assert len(ref.seen) == 6 and total == 2
        kinds.append(kind); data.append(np.packbits(np.array(bits, np.uint8))); esks.append(esk)
        ms.append([pack40(m) if m != -1 else np.zeros(5, np.uint8) for m in (m1, m2)])
        has.append([m != -1 for m in (m1, m2)])
        row_dec, row_ok, row_loc, row_n = [], [], [], []
        for c, (recd, out, loc) in enumerate(ref.seen):
            assert recd == "00000000" + s(copies[c])
            row_ok.append(out != "")
            row_dec.append(pack40(out[8:]) if out else np.zeros(5, np.uint8))
            row_loc.append((loc + [-1000, -1000])[:2]); row_n.append(len(loc))
            if kind == 3:
                sent = s(made[n][1][c])
                clean = encode([int(ch) for ch in out[8:36]]) == [int(ch) for ch in out[8:]] if out else False
                if not out:
                    outcomes["fail"] += 1
                elif out[8:] == sent and not clean:
                    outcomes["as_received"] += 1
                elif clean and loc and out[8:] != sent:
                    outcomes["miscorrected"] += 1
        if kind in (0, 1):                              # at most two flips per copy: every message comes back
            for w, g in zip((a, b), (m1, m2)):
                w = [w[0] | 1, w[1], w[2] | 1, w[3]] + w[4:] if esk else w
                recovered[0] += g == s(w)
                recovered[1] += 1
        dec.append(row_dec); ok.append(row_ok); locs.append(row_loc); nloc.append(row_n)
    assert recovered[0] == recovered[1] > 100, recovered
    assert min(outcomes.values()) > 0, outcomes
    # ---- get_next_frame on buffers of one polarity: random bits (with neither word in them) around one frame
    gbuf, glen, goff, ginv, gframe, grest = [], [], [], [], [], []
    for n, off in enumerate([0, 1, 7, 31, 32, 33, 47, 100, 287, 288, 289, 500] * 2):
        inverted = n >= 12
        a, b = word(), word()
        fr = [int(c) for c in ref.framesync] + frame_bits([a, a, a, b, b, b])
        if inverted:
            fr = [x ^ 1 for x in fr]
        while True:
            pre, post = list(rng.integers(0, 2, off)), list(rng.integers(0, 2, int(rng.integers(0, 300))))
            buf = s(pre + fr + post)
            inv = s([1 - int(c) for c in ref.framesync])
            if buf.count(ref.framesync) + buf.count(inv) == 1:
                break
        rest, frame = ref.get_next_frame({}, buf)
        assert frame == s(frame_bits([a, a, a, b, b, b])) and rest == s(post)
        by = np.packbits(np.array([int(c) for c in buf], np.uint8))
        gbuf.append(by); glen.append(len(buf)); goff.append(off); ginv.append(inverted)
        gframe.append(np.packbits(np.array([int(c) for c in frame], np.uint8))); grest.append(len(rest))
    np.savez_compressed(OUT, kind=np.array(kinds, np.uint8), data=np.stack(data), esk=np.array(esks, np.uint8),
                        m=np.array(ms, np.uint8), has_m=np.array(has, np.uint8), copy=np.array(dec, np.uint8),
                        copy_ok=np.array(ok, np.uint8), loc=np.array(locs, np.int16), n_loc=np.array(nloc, np.uint8),
                        gnf_buf=np.concatenate(gbuf), gnf_bits=np.array(glen, np.int32), gnf_offset=np.array(goff, np.int32),
                        gnf_inverted=np.array(ginv, np.uint8), gnf_frame=np.stack(gframe), gnf_rest=np.array(grest, np.int32))
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(made), "frames; three and four flips:", outcomes,
          "; messages with <= 2 flips per copy recovered: %d of %d" % tuple(recovered))


if __name__ == "__main__":
    main()
