"""The EDACS control-frame stage (rcf_chan_edacs, include/rcf.h) restated in numpy / plain Python, for the tests: frames
from the slicer's words and hits, the six copies, BCH(48,36) over GF(64) by the syndromes S1 and S3, the Chien walk, the
election, the records.  Also the other direction for the tests' signals: a systematic encoder and a frame builder, and the
slicer's hit rule with sync_both."""
import numpy as np

import slicer_ref as S
from frames_ref import frame_walk
from rcf import native

SYNC, SYNC_BITS, FRAME_BITS = 0b010101010101010101010111000100100101010101010101, 48, 288
SYNC_STR = "{0:048b}".format(SYNC)
GEN = 0x1539                                        # (x^6 + x + 1)(x^6 + x^4 + x^2 + x + 1)

# GF(64), alpha^6 = alpha + 1
ALPHA, LOG = [0] * 63, [None] * 64
_v = 1
for _e in range(63):
    ALPHA[_e], LOG[_v] = _v, _e
    _v <<= 1
    if _v & 64:
        _v = (_v & 63) ^ 3


def solve(s1, s3):
    """a syndrome pair -> (status, positions): status 0 the copy stands, 1 one position, 2 two positions, 3 failed"""
    if s1 == 0:
        return 0, []
    if s3 == ALPHA[3 * LOG[s1] % 63]:
        pos = [LOG[s1]]
    else:
        aux = ALPHA[3 * LOG[s1] % 63] ^ s3
        e1, e2 = (2 * LOG[s1] - LOG[aux]) % 63, (LOG[s1] - LOG[aux]) % 63
        pos = [i % 63 for i in range(1, 64) if 1 ^ ALPHA[(e1 + i) % 63] ^ ALPHA[(e2 + 2 * i) % 63] == 0]
        if len(pos) != 2:
            return 3, pos
    if any(p > 47 for p in pos):
        return 3, pos
    return len(pos), pos


def syndromes(positions):
    s1 = s3 = 0
    for j in positions:
        s1 ^= ALPHA[j % 63]
        s3 ^= ALPHA[3 * j % 63]
    return s1, s3


def bch(copy):
    """copy: 40 bits (0 / 1), the first one first -> (status, the corrected 40 bits, positions).  status 0 clean or stands,
    1 one position, 2 two positions, 3 failed (the bits then as received)"""
    copy = [int(b) for b in copy]
    status, pos = solve(*syndromes([j for j in range(40) if copy[39 - j]]))
    out = list(copy)
    if status != 3:
        for p in pos:
            if p < 40:
                out[39 - p] ^= 1
    return status, out, pos


def elect(decoded):
    """decoded: three (status, bits) -> the elected 40 bits or None"""
    good = [tuple(b) for st, b in decoded if st != 3]
    if not good:
        return None
    if len(good) == 1:
        return list(good[0])
    for i in range(len(good)):
        if good.count(good[i]) >= 2:
            return list(good[i])
    return None


def decode_frame(data, esk=False):
    """data: the frame's 240 data bits, polarity already applied -> (statuses[6], m1, m2), m a list of 40 bits or None"""
    data = [int(b) for b in data]
    dec = []
    for c in range(6):
        copy = data[40 * c:40 * c + 40]
        if c in (1, 4):
            copy = [b ^ 1 for b in copy]
        st, bits, _ = bch(copy)
        dec.append((st, bits))
    ms = []
    for m in (elect(dec[:3]), elect(dec[3:])):
        if m is not None and esk:
            m = [m[0] | 1, m[1], m[2] | 1, m[3]] + m[4:]
        ms.append(m)
    return [d[0] for d in dec], ms[0], ms[1]


def record(k, inverted, dist, statuses, m1, m2):
    r = np.zeros((), native.EDACS_DTYPE)
    flags = int(inverted) | (m1 is not None) << 1 | (m2 is not None) << 2 | int(dist) << 4
    for c, st in enumerate(statuses):
        flags |= st << (10 + 2 * c)
    r["flags"], r["k"] = flags, k & 0xffffffff
    for name, m in (("m1", m1), ("m2", m2)):
        if m is not None:
            r[name][:5] = np.packbits(np.array(m, np.uint8))
    return r


def bits_of_words(words):
    """the bit stream of the slicer's words (uint32, or their uint8 view as chan_read_hard gives it)"""
    words = np.asarray(words)
    return np.unpackbits(words if words.dtype == np.uint8 else words.astype("<u4").view(np.uint8))


def run(words, k, dist, first_hit=0, launches=None, word_cap=None, hit_cap=None, sync_both=True, esk=False, base_words=0, base_hits=0,
        frames=None):
    """-> (records, dict(n_records, n_frames, n_msgs, n_msgs_none, n_lost)).  words, k, dist: the slicer's streams from its
    start; first_hit: the slicer's n_hits when the stage was attached; launches: [(n_words, n_hits)] after each block (default:
    one, at the end); word_cap / hit_cap: the rings' capacities (default: nothing is ever overwritten); base_words / base_hits:
    the index of the first word / hit given (k, first_hit and the launches count from the slicer's start); frames: a list that
    takes every decided frame's 240 data bits, polarity applied, in the records' order (for census)"""
    bits = bits_of_words(words)
    k = [None] * base_hits + [int(v) for v in k]
    dist = [None] * base_hits + list(dist)
    launches = [(base_words + len(bits) // 32, len(k))] if launches is None else launches
    out = []
    st = dict(n_records=0, n_frames=0, n_msgs=0, n_msgs_none=0, n_lost=0)
    for i, s, _ in frame_walk(k, launches, st, first_hit, word_cap, hit_cap, sync=48, accept=FRAME_BITS, decide=FRAME_BITS, longest=FRAME_BITS,
                              per_word=32, cut=False):
        raw = int(dist[i])
        inverted = bool(sync_both) and raw > 24
        data = bits[s + 48 - 32 * base_words:s + 288 - 32 * base_words] ^ (1 if inverted else 0)
        if frames is not None:
            frames.append(data)
        statuses, m1, m2 = decode_frame(data, esk)
        out.append(record(k[i], inverted, 48 - raw if inverted else raw, statuses, m1, m2))
        st["n_msgs"] += (m1 is not None) + (m2 is not None)
        st["n_msgs_none"] += (m1 is None) + (m2 is None)
    recs = np.array(out, native.EDACS_DTYPE) if out else np.zeros(0, native.EDACS_DTYPE)
    st["n_records"] = len(recs)
    return recs, st


# ---- the slicer with sync_both: the hits of slicer_ref with every window let through, then the rule
def is_hit(dist, max_errors, sync_both, sync_bits=48):
    return dist <= max_errors or (bool(sync_both) and dist >= sync_bits - max_errors)


def slicer(soft, max_errors=0, sync_both=1, cuts=None):
    """-> dict(words, k, dist, n_symbols) of a binary slicer that searches the EDACS word"""
    r = S.run(np.asarray(soft, np.float32), S.BINARY, sync_word=SYNC, sync_bits=48, max_errors=48, cuts=cuts)
    keep = np.array([is_hit(int(d), max_errors, sync_both) for d in r["dist"]], bool)
    return dict(words=r["words"], k=np.asarray(r["k"])[keep], dist=np.asarray(r["dist"])[keep], n_symbols=len(soft))


# ---- the other direction
def encode(msg28):
    """28 message bits -> the 40 bits of a copy: systematic, 12 parity bits behind the message (the remainder of
    m(x) x^12 by the generator)"""
    msg28 = [int(b) for b in msg28]
    reg = 0
    for b in msg28 + [0] * 12:
        reg = (reg << 1) | b
        if reg & 0x1000:
            reg ^= GEN
    return msg28 + [(reg >> (11 - i)) & 1 for i in range(12)]


def frame(m1, m2, inverted=False):
    """the 288 bits of a frame: sync word, three copies of each 40-bit message with the middle one inverted"""
    bits = [int(c) for c in SYNC_STR]
    for m in (m1, m2):
        m = [int(b) for b in m]
        bits += m + [b ^ 1 for b in m] + m
    bits = np.array(bits, np.uint8)
    return bits ^ 1 if inverted else bits


def bitstr(m):
    return -1 if m is None else "".join(str(int(b)) for b in m)


# ---- designed input: copies with chosen error patterns, so that the decoder's correcting paths are walked on purpose
def flip_patterns():
    """-> (the 40 single flips, the 780 pairs of flips) of a 40-bit copy, each a tuple of copy bits (0: the first bit)"""
    return [(a,) for a in range(40)], [(a, b) for a in range(40) for b in range(a + 1, 40)]


def designed_bits(patterns, seed, inverted=False):
    """600 bits for the clock to settle, then back-to-back frames of two random messages each, copy slot n % 6 of frame n // 6
    carrying patterns[n] (a tuple of copy bits to flip; the slots past the last pattern stay clean), 420 bits behind ->
    (bits, per frame (m1, m2) as sent, the frames' starts, per frame the six patterns)"""
    rng = np.random.default_rng(seed)
    patterns = list(patterns) + [()] * (-len(patterns) % 6)
    parts, sent, starts, flips = [rng.integers(0, 2, 600).astype(np.uint8)], [], [], []
    for n in range(0, len(patterns), 6):
        m1, m2 = encode(rng.integers(0, 2, 28)), encode(rng.integers(0, 2, 28))
        f = frame(m1, m2)
        for c in range(6):
            for b in patterns[n + c]:
                f[48 + 40 * c + b] ^= 1
        starts.append(600 + 288 * (n // 6)); sent.append((bitstr(m1), bitstr(m2))); flips.append(patterns[n:n + 6]); parts.append(f)
    parts.append(rng.integers(0, 2, 420).astype(np.uint8))
    bits = np.concatenate(parts)
    return (bits ^ 1 if inverted else bits), sent, starts, flips


CLASSES = ("fails", "miscorrects", "stands", "colour", "beyond")


def pattern_classes(pattern):
    """what the decoder makes of a valid copy with these copy bits flipped (the syndromes are the flips' alone) -> set of:
    fails (status 3), miscorrects (status 2, and not back to what was sent), stands (S1 = 0, S3 != 0: status 0, uncorrected),
    colour (a position in 40 .. 47: accepted, no bit changed), beyond (a position > 47: fails)"""
    js = sorted(39 - b for b in pattern)
    s1, s3 = syndromes(js)
    status, pos = solve(s1, s3)
    out = set()
    if status == 3:
        out.add("fails")
        if any(p > 47 for p in pos):
            out.add("beyond")
    if status == 2 and sorted(pos) != js:
        out.add("miscorrects")
    if s1 == 0 and s3 != 0:
        out.add("stands")
    if status in (1, 2) and any(40 <= p <= 47 for p in pos):
        out.add("colour")
    return out


def class_patterns(seed=3, each=10, limit=200000):
    """random 3- and 4-flip patterns, searched until every class of CLASSES has `each` of them (at most `limit` candidates) ->
    {class: [patterns]}"""
    rng = np.random.default_rng(seed)
    found = {c: [] for c in CLASSES}
    for n in range(limit):
        p = tuple(sorted(int(b) for b in rng.choice(40, 3 + n % 2, replace=False)))
        for c in pattern_classes(p):
            if len(found[c]) < each and p not in found[c]:
                found[c].append(p)
        if all(len(v) >= each for v in found.values()):
            break
    return found


def designed_classes(seed=3):
    """the patterns of the second designed carrier -> (patterns for designed_bits, {class: how many of them}).  Every class
    pattern sits beside two clean copies of its message, its slot rotating through the six; then the election's cases, two
    frames each (m1 and m2 alike): one of three copies decoded; two decoded that disagree; two that agree against a third"""
    found = class_patterns(seed)
    every = [p for c in CLASSES for p in found[c]]
    out = []
    for n, p in enumerate(every):
        group = [(), (), ()]
        group[n % 3] = p
        out += group
    out += [()] * (-len(out) % 6)
    fails, wrong = found["fails"], found["miscorrects"]
    for n in range(2):
        out += [fails[0], fails[1], (), (), fails[2], fails[3]]                     # one decoded
        out += [fails[4], wrong[0], (), wrong[1], (), fails[5]]                     # two decoded, different values
        out += [wrong[2], (), (5, 17), (30,), wrong[3], ()]                         # three decoded, two agree
    return out, {c: len(found[c]) for c in CLASSES}


def census(frames, sent):
    """frames: per decided frame its 240 data bits, polarity applied (run(frames=) collects them); sent: per frame the two
    messages sent (bit strings) -> {class: copies of it met} and {"one", "differ", "outvoted": message groups of that kind}"""
    seen = {c: 0 for c in CLASSES}
    seen.update(one=0, differ=0, outvoted=0)
    for data, ms in zip(frames, sent):
        dec = []
        for c in range(6):
            copy = [int(b) ^ (1 if c in (1, 4) else 0) for b in data[40 * c:40 * c + 40]]
            was = [int(ch) for ch in ms[c // 3]]
            for cl in pattern_classes([b for b in range(40) if copy[b] != was[b]]):
                seen[cl] += 1
            st, bits, _ = bch(copy)
            dec.append((st, tuple(bits)))
        for g in (dec[:3], dec[3:]):
            good = [b for st, b in g if st != 3]
            seen["one"] += len(good) == 1
            seen["differ"] += len(good) >= 2 and elect(g) is None
            seen["outvoted"] += len(good) == 3 and len(set(good)) == 2
    return seen
