"""The P25 trunking stage (rcf_chan_tsbk, include/rcf.h) restated in plain numpy / Python over what the slicer's readers
deliver: the packed words and the (widened) sync hits.  Frames from the hits by the accept rule, status symbols stripped, NID
read, every block deinterleaved, trellis-decoded by the 49-step walk and CRC-checked bit by bit -> records of
native.TSBK_DTYPE and the stage's counters.  `launches` walks the streams as the stage sees them grow, block by block, and
models the two rings' losses."""
import numpy as np

from frames_ref import frame_walk
from rcf import native

W = ((0x2, 0xC, 0x1, 0xF), (0xE, 0x0, 0xD, 0x3), (0x9, 0x7, 0xA, 0x4), (0x5, 0xB, 0x6, 0x8))
ORDER = [i + j + e for i in range(0, 23, 2) for j in (0, 26, 50, 74) for e in (0, 1)] + [24, 25]   # deinterleaved dibit n <- block dibit ORDER[n]
DECIDE = 384                                       # dibits from the frame's start that must be in whole words
WALK = dict(sync=24, accept=24, decide=DECIDE, longest=360, per_word=16, cut=True)     # frames_ref.frame_walk's constants


def dibits_of(words):
    """the dibit stream of packed words (uint32, or their uint8 view)"""
    by = np.ascontiguousarray(words).view(np.uint8)
    bits = np.unpackbits(by)
    return (2 * bits[0::2] + bits[1::2]).astype(np.uint8)


def pos(j):
    """frame dibit of info dibit j"""
    return j + j // 35


def trellis(code_words):
    """-> (states, code words with no exact candidate)"""
    state, out, inexact = 0, [], 0
    for c in code_words:
        same = [4 - bin(W[state][d] ^ c).count("1") for d in range(4)]
        inexact += 4 not in same
        state = same.index(max(same))
        out.append(state)
    return out, inexact


def crc_register(bits):
    reg = 0
    for b in bits:
        reg = (reg << 1) | int(b)
        if reg & 0x10000:
            reg = (reg & 0xffff) ^ 0x1021
    return reg


def decode_block(block):
    """a block's 98 dibits -> (the 96 bits, crc bad, n_inexact)"""
    d = [int(block[at]) for at in ORDER]
    states, inexact = trellis([4 * d[2 * t] + d[2 * t + 1] for t in range(49)])
    bits = [v for s in states[:48] for v in (s >> 1, s & 1)]
    return bits, int(crc_register(bits) != 0xffff), inexact


def frame_records(d, s, fd, k, dist, blocks=None):
    """the records of the frame that starts at stream dibit s and has fd dibits; blocks: a list that takes every decoded
    block's 98 dibits (for census)"""
    info = lambda j: int(d[s + pos(j)])
    nid_bits = [v for j in range(24, 56) for v in (info(j) >> 1, info(j) & 1)]
    nid = np.packbits(np.array(nid_bits, np.uint8))
    nac = int("".join(map(str, nid_bits[:12])), 2)
    duid = int("".join(map(str, nid_bits[12:16])), 2)
    recs = []
    if duid == 7:
        for b in range(3):
            if pos(153 + 98 * b) >= fd:
                break
            block = [info(56 + 98 * b + p) for p in range(98)]
            if blocks is not None:
                blocks.append(block)
            bits, bad, inexact = decode_block(block)
            nxt = pos(154 + 98 * b)
            next_bit = info(154 + 98 * b) >> 1 if nxt < fd else 0
            recs.append((b, bad, next_bit, inexact, np.packbits(np.array(bits, np.uint8))))
    if not recs:
        recs.append((3, 0, 0, 0, np.zeros(12, np.uint8)))
    out = np.zeros(len(recs), native.TSBK_DTYPE)
    for r, (b, bad, next_bit, inexact, octets) in zip(out, recs):
        r["flags"] = b | bad << 2 | next_bit << 3 | inexact << 4 | int(dist) << 10 | duid << 16 | nac << 20
        r["k"] = k & 0xffffffff
        r["octets"] = octets
        r["nid"] = nid
        r["frame_dibits"] = fd
    return out


# ---- the other direction, for the tests' signals: a TSBK's 12 octets -> a block -> a frame's dibits
SYNC_DIBITS = [(0x5575F5FF77FF >> (46 - 2 * i)) & 3 for i in range(24)]


def tsbk_octets(rng):
    """10 random octets and the 2 that make the CRC good"""
    payload = np.unpackbits(rng.integers(0, 256, 10).astype(np.uint8))
    f = crc_register(list(payload) + [0] * 16) ^ 0xffff
    return bytes(np.packbits(np.concatenate([payload, [(f >> (15 - i)) & 1 for i in range(16)]]).astype(np.uint8)))


def encode_block(octets):
    """12 octets -> the block's 98 dibits: the trellis forward from state 0 with a flushing dibit, then the interleaver"""
    bits = np.unpackbits(np.frombuffer(octets, np.uint8))
    coded, state = [], 0
    for d in [2 * int(bits[2 * i]) + int(bits[2 * i + 1]) for i in range(48)] + [0]:
        coded += [W[state][d] >> 2, W[state][d] & 3]
        state = d
    block = [0] * 98
    for n, at in enumerate(ORDER):
        block[at] = coded[n]
    return block


def frame(nac, duid, tsbks, rng, total=None):
    """a data unit's dibits: sync, NID (nac, duid and 48 bits nobody checks), the TSBKs' blocks, null dibits up to `total`
    (default: the TSDU's length for that many blocks), a status dibit behind every 35 info dibits"""
    return frame_of_blocks(nac, duid, [encode_block(t) for t in tsbks], rng, total)


def frame_of_blocks(nac, duid, blocks, rng, total=None):
    """the same around blocks given as their 98 dibits each, whatever they are"""
    total = {0: 180, 1: 180, 2: 288, 3: 360}[len(blocks)] if total is None else total
    nid = (nac << 52) | (duid << 48) | int(rng.integers(0, 1 << 48))
    info = SYNC_DIBITS + [(nid >> (62 - 2 * i)) & 3 for i in range(32)]
    for b in blocks:
        info += [int(v) for v in b]
    info += [0] * (total - total // 36 - len(info))
    out = []
    for j, d in enumerate(info[:total - total // 36]):
        out.append(d)
        if j % 35 == 34:
            out.append(int(rng.integers(0, 4)))
    return np.array(out[:total], np.uint8)


def run(words, k, dist, first_hit=0, launches=None, word_cap=None, hit_cap=None, blocks=None):
    """-> (records, dict(n_records, n_frames, n_blocks, n_crc_bad, n_lost)).  words, k, dist: the slicer's streams from its
    start; first_hit: the slicer's n_hits when the stage was attached; launches: [(n_words, n_hits)] after each block (default:
    one, at the end); word_cap / hit_cap: the rings' capacities (default: nothing is ever overwritten); blocks: a list that
    takes the 98 dibits of every block decoded, in the records' order"""
    d = dibits_of(words)
    k = [int(v) for v in k]
    launches = [(len(d) // 16, len(k))] if launches is None else launches
    out = []
    st = dict(n_records=0, n_frames=0, n_blocks=0, n_crc_bad=0, n_lost=0)
    for i, s, fd in frame_walk(k, launches, st, first_hit, word_cap, hit_cap, **WALK):
        recs = frame_records(d, s, fd, k[i], dist[i], blocks)
        out.append(recs)
        decoded = recs[(recs["flags"] & 3) != 3]
        st["n_blocks"] += len(decoded)
        st["n_crc_bad"] += int(np.count_nonzero(decoded["flags"] & 4))
    recs = np.concatenate(out) if out else np.zeros(0, native.TSBK_DTYPE)
    st["n_records"] = len(recs)
    return recs, st


# ---- designed input: TSDUs whose blocks are wrong, so that the decoder's correcting paths are walked on purpose
def damaged_block(octets, t, n_wrong, rng):
    """a valid TSBK's block with n_wrong (1 .. 4) wrong dibits, the first of them in code word t (0 .. 48; 48 is the
    flushing word, block dibits 24 and 25), the others anywhere else"""
    block = encode_block(octets)
    at = [ORDER[2 * t + int(rng.integers(0, 2))]]
    others = [p for p in range(98) if p not in (ORDER[2 * t], ORDER[2 * t + 1])]
    at += [int(p) for p in rng.choice(others, n_wrong - 1, replace=False)]
    for p in at:
        block[p] ^= int(rng.integers(1, 4))
    return block


def designed_dibits(nac=0x293, seed=49):
    """-> (dibits, the planted frames' starts).  1000 dibits for the loop to settle, then back to back, all with DUID 7:
    set 1, 30 frames of three blocks of 98 random dibits each; set 2, 17 frames of three valid TSBKs with 1 .. 4 wrong dibits,
    block n's first wrong dibit in code word n % 49; set 3, a 180-dibit and a 288-dibit frame of such blocks (the frame that
    follows each cuts it there); a last clean frame and a tail"""
    rng = np.random.default_rng(seed)
    frames = [frame_of_blocks(nac, 7, [rng.integers(0, 4, 98) for _ in range(3)], rng) for _ in range(30)]
    n = 0
    for _ in range(17):
        blocks = []
        for _ in range(3):
            blocks.append(damaged_block(tsbk_octets(rng), n % 49, 1 + n % 4, rng))
            n += 1
        frames.append(frame_of_blocks(nac, 7, blocks, rng))
    frames.append(frame_of_blocks(nac, 7, [damaged_block(tsbk_octets(rng), 48, 2, rng)], rng))
    frames.append(frame_of_blocks(nac, 7, [damaged_block(tsbk_octets(rng), t, 3, rng) for t in (47, 0)], rng))
    frames.append(frame(nac, 7, [tsbk_octets(rng) for _ in range(3)], rng))
    starts = (1000 + np.concatenate([[0], np.cumsum([len(f) for f in frames])[:-1]])).tolist()
    d = np.concatenate([rng.integers(0, 4, 1000)] + frames + [rng.integers(0, 4, 480)]).astype(np.uint8)
    return d, starts


DESIGNED_FRAME_DIBITS = [360] * 47 + [180, 288, 360]


def census(blocks, st):
    """what the decoder went through on these blocks (98 dibits each, as run(blocks=) collects them) and the restatement's
    counters st -> dict: pairs, the (state, code word) pairs met; inexact_lanes, the code words t that had no exact candidate
    in some block; entered[t], the states code word t was decoded from; max_inexact; n_crc_bad, n_crc_good"""
    pairs, lanes, entered, most = set(), set(), [set() for _ in range(49)], 0
    for block in blocks:
        d = [int(block[at]) for at in ORDER]
        state, n = 0, 0
        for t in range(49):
            c = 4 * d[2 * t] + d[2 * t + 1]
            same = [4 - bin(W[state][v] ^ c).count("1") for v in range(4)]
            pairs.add((state, c)); entered[t].add(state)
            if 4 not in same:
                lanes.add(t); n += 1
            state = same.index(max(same))
        most = max(most, n)
    return dict(pairs=pairs, inexact_lanes=lanes, entered=entered, max_inexact=most, n_crc_bad=st["n_crc_bad"],
                n_crc_good=st["n_blocks"] - st["n_crc_bad"])


def check_census(c):
    """the designed input's guarantees: every (state, code word) pair, an inexact word at every lane, lanes 1 .. 48 entered
    from all four states, the 6-bit n_inexact field's upper half, blocks with a bad and with a good CRC"""
    assert len(c["pairs"]) == 64, sorted(c["pairs"])
    assert c["inexact_lanes"] == set(range(49)), sorted(set(range(49)) - c["inexact_lanes"])
    assert all(c["entered"][t] == {0, 1, 2, 3} for t in range(1, 49)) and c["entered"][0] == {0}, c["entered"]
    assert c["max_inexact"] >= 32 and c["n_crc_bad"] > 0 and c["n_crc_good"] > 0, (c["max_inexact"], c["n_crc_bad"], c["n_crc_good"])
