"""The trellis option of the P25 trunking stage (RCF_TRELLIS_VITERBI: rcf_chan_tsbk_opt, include/rcf.h) restated in plain
Python: the sequential form of the rule -- backward costs beta, then a forward walk that takes the lowest state of equals --,
a brute-force decoder over all 4^n paths of a trellis truncated to n code words plus the flushing word (least cost, then the
lexicographic rule, nothing shared with the sequential form), the reference's greedy walk (tsbk_ref.trellis itself) and the
free distance by search.  `run` is tsbk_ref.run / nid_ref.run_tsbk with the rule applied per block: it wraps
tsbk_ref.decode_block and leaves the modules as they are.  Below that the other direction for the tests' signals: blocks
with planted flips, the designed stream and the census of what it guarantees."""
import itertools

import numpy as np

import nid_ref as N
import tsbk_ref as T
from tsbk_ref import trellis as greedy          # the reference's walk: -> (states, code words with no exact candidate)

W = T.W
GREEDY, VITERBI = 0, 1


def pop(v):
    return bin(v).count("1")


def code_words(block):
    """a block's 98 dibits -> its 49 deinterleaved code words"""
    d = [int(block[at]) for at in T.ORDER]
    return [4 * d[2 * t] + d[2 * t + 1] for t in range(len(d) // 2)]


DIST = [[[pop(W[s][d] ^ c) for d in range(4)] for c in range(16)] for s in range(4)]      # DIST[s][c][d]


def sequential(c):
    """the rule's sequential form on n + 1 code words, the last one the flushing word -> (states s_0 .. s_n, cost, n_inexact)"""
    n = len(c) - 1
    beta = [None] * (n + 1)
    beta[n] = [DIST[s][c[n]][0] for s in range(4)]
    for t in range(n - 1, -1, -1):
        nxt = beta[t + 1]
        beta[t] = [min(a + b for a, b in zip(DIST[s][c[t]], nxt)) for s in range(4)]
    s, states, cost, inexact = 0, [], 0, 0
    for t in range(n):
        sums = [a + b for a, b in zip(DIST[s][c[t]], beta[t + 1])]
        d = sums.index(min(sums))
        away = DIST[s][c[t]][d]
        cost += away; inexact += away != 0
        states.append(d)
        s = d
    away = DIST[s][c[n]][0]
    return states + [0], cost + away, inexact + (away != 0)


def sequential_many(c):
    """the same rule over many blocks at once in numpy (c: uint8 [N][n + 1]) -> (states [N][n + 1], cost [N], n_inexact [N]);
    np.argmin takes the first of equals, the lowest state"""
    c = np.asarray(c, np.int64)
    n = c.shape[1] - 1
    table = np.array(DIST, np.int64)                  # [s][c][d]
    at = np.arange(len(c))
    beta = np.zeros((n + 2, len(c), 4), np.int64)
    beta[n] = table[:, c[:, n], 0].T
    for t in range(n - 1, -1, -1):
        beta[t] = (table[:, c[:, t], :] + beta[t + 1][None, :, :]).min(axis=2).T
    s = np.zeros(len(c), np.int64)
    states = np.zeros((len(c), n + 1), np.int64)
    cost = np.zeros(len(c), np.int64)
    inexact = np.zeros(len(c), np.int64)
    for t in range(n + 1):
        branch = table[s, c[:, t], :]                # [N][d]
        d = np.argmin(branch + beta[t + 1], axis=1) if t < n else np.zeros(len(c), np.int64)
        away = branch[at, d]
        cost += away; inexact += away != 0
        states[:, t] = d
        s = d
    return states, cost, inexact


_PATHS = {}


def brute(c):
    """all 4^n paths of n code words plus the flushing word, every one costed: the least cost, the lexicographically smallest
    of equals (the paths stand in lexicographic order and np.argmin takes the first of the least) -> (states, cost, n_inexact)"""
    n = len(c) - 1
    if n not in _PATHS:
        _PATHS[n] = np.array(list(itertools.product(range(4), repeat=n)), np.int64).reshape(-1, n)
    paths = _PATHS[n]
    table = np.array(W, np.int64)
    bits = np.array([pop(v) for v in range(16)], np.int64)
    prev = np.zeros(len(paths), np.int64)
    cost = np.zeros(len(paths), np.int64)
    for t in range(n):
        cost += bits[table[prev, paths[:, t]] ^ c[t]]
        prev = paths[:, t]
    cost += bits[table[prev, 0] ^ c[n]]
    at = int(np.argmin(cost))
    states = paths[at].tolist() + [0]
    before = [0] + states[:-1]
    return states, int(cost[at]), sum(W[p][s] != w for p, s, w in zip(before, states, c))


def free_distance(depth=12):
    """the least Hamming distance between the words of two paths that leave a common state by different dibits and meet
    again, over all start states: a search over the pair of states after the divergence, by increasing depth"""
    best = None
    for s0 in range(4):
        front = {}
        for a in range(4):
            for b in range(a + 1, 4):
                front[(a, b)] = pop(W[s0][a] ^ W[s0][b])
        for _ in range(depth):
            nxt = {}
            for (a, b), dist in front.items():
                for x in range(4):
                    for y in range(4):
                        dd = dist + pop(W[a][x] ^ W[b][y])
                        if x == y:
                            best = dd if best is None else min(best, dd)
                        elif dd < nxt.get((x, y), 1 << 30):
                            nxt[(x, y)] = dd
            front = {k: v for k, v in nxt.items() if best is None or v < best}
    return best


def decode_block(block, trellis=VITERBI):
    """a block's 98 dibits -> (the 96 bits, crc bad, n_inexact, cost; cost None under GREEDY)"""
    if trellis == GREEDY:
        return T.decode_block(block) + (None,)
    states, cost, inexact = sequential(code_words(block))
    bits = [v for s in states[:48] for v in (s >> 1, s & 1)]
    return bits, int(T.crc_register(bits) != 0xffff), inexact, cost


def octets_of(bits):
    return bytes(np.packbits(np.array(bits, np.uint8)))


def empty_state():
    return dict(n_decoded=0, n_clean=0, n_bits=0, n_words=0)


def run(words, k, dist, trellis=VITERBI, nid=0, **kw):
    """tsbk_ref.run (nid=1: nid_ref.run_tsbk) under RCF_TRELLIS_VITERBI -> (records, the five counters, rcf_nid_state_t's
    four, rcf_trellis_state_t's four).  trellis=GREEDY: those restatements themselves"""
    vst = empty_state()
    if trellis == GREEDY:
        return N.run_tsbk(words, k, dist, nid=nid, **kw) + (vst,)
    plain_block, plain_frame = T.decode_block, T.frame_records
    costs = []

    def block_rule(block):
        bits, bad, inexact, cost = decode_block(block, VITERBI)
        costs.append(cost)
        vst["n_decoded"] += 1; vst["n_clean"] += cost == 0; vst["n_bits"] += cost; vst["n_words"] += inexact
        return bits, bad, inexact

    def frame_records(d, s, fd, kk, dd, blocks=None):
        del costs[:]
        recs = plain_frame(d, s, fd, kk, dd, blocks)
        for r, cost in zip(recs, costs):              # (a frame record has no block and so no cost)
            r["frame_dibits"] |= cost << 21 | 1 << 29
        return recs

    T.decode_block, T.frame_records = block_rule, frame_records
    try:
        out = N.run_tsbk(words, k, dist, nid=nid, **kw)
    finally:
        T.decode_block, T.frame_records = plain_block, plain_frame
    # the rule reaches the restatements through their module attributes: should one of them ever bind decode_block another
    # way, this yardstick must fail, not turn back into the greedy rule
    assert vst["n_decoded"] == out[1]["n_blocks"], (vst, out[1])
    assert int(np.count_nonzero(out[0]["frame_dibits"] >> 29 & 1)) == np.count_nonzero((out[0]["flags"] & 3) != 3)
    return out + (vst,)


# ---- the other direction
def flipped(block, places):
    """a block's 98 dibits with the channel bits `places` (0 .. 195: bit 2 p + e is bit e, the higher first, of block dibit p)
    flipped"""
    block = [int(v) for v in block]
    for q in places:
        block[q // 2] ^= 2 >> (q % 2)
    return block


def bit_of(t, e):
    """the channel bit that carries bit e (0 .. 3, the first one highest) of code word t"""
    return 2 * T.ORDER[2 * t + e // 2] + e % 2


def ties(octets, t, e):
    """flipping bit e of code word t of this block leaves the greedy walk two candidates tied at three equal bits"""
    c = code_words(T.encode_block(octets))
    s = 0 if t == 0 else c_state(octets, t - 1)
    got = c[t] ^ (8 >> e)
    same = sorted(4 - pop(W[s][d] ^ got) for d in range(4))
    return same[-1] == same[-2] == 3


def c_state(octets, t):
    bits = np.unpackbits(np.frombuffer(octets, np.uint8))
    return (2 * int(bits[2 * t]) + int(bits[2 * t + 1])) if t < 48 else 0


def designed_blocks(seed=77):
    """-> list of dict(what, octets, places, block): valid TSBKs with planted channel-bit flips (places: channel bits 0 .. 195
    of the block), kind by kind"""
    rng = np.random.default_rng(seed)
    out = []

    def add(what, places, octets=None):
        octets = T.tsbk_octets(rng) if octets is None else octets
        out.append(dict(what=what, octets=octets, places=sorted(int(p) for p in places), block=flipped(T.encode_block(octets), places)))

    for _ in range(3):
        add("clean", [])
    for want in (True, False):                       # single flips that do and do not tie two candidates
        for t0 in (0, 1, 17, 30, 47):
            octets = T.tsbk_octets(rng)
            found = [(t, e) for t in list(range(t0, 48)) + list(range(t0)) for e in range(4) if ties(octets, t, e) == want]
            add("single tie" if want else "single no tie", [bit_of(*found[0])], octets)
    for e in range(4):
        add("flush", [bit_of(48, e)])
    for t in (0, 11, 47):
        add("double one word", [bit_of(t, 0), bit_of(t, 3)])
        add("double two words", [bit_of(t, 1), bit_of((t + 1) % 49, 2)])
        add("double far", [bit_of(t, 2), bit_of((t + 20) % 49, 0)])
    for at in (0, 51, 192):
        add("burst 4", range(at, at + 4))
    for n in (3, 4, 8):
        for _ in range(3):
            add("%d flips" % n, rng.choice(196, n, replace=False))
    return out


def designed_dibits(nac=0x293, seed=77):
    """-> (dibits, plan).  1000 dibits to settle, then back to back, all with DUID 7: the designed blocks three to a frame
    of 360 dibits, then a 288-dibit and a 180-dibit frame of clean blocks, then a frame cut short by an early next sync after
    one whole block (its second block never ends: total 200 dibits), a last clean frame and a tail.  plan: per decoded block
    dict(what, octets, places) in the records' order, a dict(what="frame record") for the frame without a block"""
    rng = np.random.default_rng(seed)
    blocks = designed_blocks(seed)
    while len(blocks) % 3:
        octets = T.tsbk_octets(rng)
        blocks.append(dict(what="clean", octets=octets, places=[], block=T.encode_block(octets)))
    frames, plan = [], []
    for i in range(0, len(blocks), 3):
        frames.append(T.frame_of_blocks(nac, 7, [b["block"] for b in blocks[i:i + 3]], rng))
        plan += blocks[i:i + 3]
    for n in (2, 1):
        extra = [dict(what="clean", octets=T.tsbk_octets(rng), places=[]) for _ in range(n)]
        frames.append(T.frame(nac, 7, [b["octets"] for b in extra], rng))
        plan += extra
    cut = [dict(what="cut", octets=T.tsbk_octets(rng), places=[bit_of(5, 1)]), dict(what="never ends", octets=T.tsbk_octets(rng), places=[])]
    frames.append(T.frame_of_blocks(nac, 7, [flipped(T.encode_block(b["octets"]), b["places"]) for b in cut], rng, total=288)[:200])
    plan.append(cut[0])
    frames.append(T.frame_of_blocks(nac, 7, [], rng, total=180)[:100])           # cut before its first block ends: a frame record
    plan.append(dict(what="frame record"))
    last = [dict(what="clean", octets=T.tsbk_octets(rng), places=[]) for _ in range(3)]
    frames.append(T.frame(nac, 7, [b["octets"] for b in last], rng))
    plan += last
    starts = (1000 + np.concatenate([[0], np.cumsum([len(f) for f in frames])[:-1]])).tolist()
    d = np.concatenate([rng.integers(0, 4, 1000)] + frames + [rng.integers(0, 4, 480)]).astype(np.uint8)
    return d, plan, starts


DESIGNED_KINDS = {"clean", "single tie", "single no tie", "flush", "double one word", "double two words", "double far", "burst 4",
                  "3 flips", "4 flips", "8 flips", "cut", "frame record"}


def check_census(recs, twin, plan, fields, trellis_fields):
    """the designed input's guarantees, on the records with the option (recs) and the twin's without (twin), record i being
    plan[i]: every kind is there; every block with at most 2 flips carries the sent octets, a good CRC and its flips as the
    cost on the option's channel, with n_inexact the code words those flips lie in; no block costs more than its flips (the
    sent path is a path); at least one block with at most 2 flips has a bad CRC on the twin; the frame record's new bits are
    0; the twin has no new bit at all -> dict of counts"""
    assert len(recs) == len(twin) == len(plan), (len(recs), len(twin), len(plan))
    f, g, v, u = fields(recs), fields(twin), trellis_fields(recs), trellis_fields(twin)
    assert not np.any(u["cost"]) and not np.any(u["viterbi"])
    assert {p["what"] for p in plan} == DESIGNED_KINDS, {p["what"] for p in plan} ^ DESIGNED_KINDS
    twin_bad = right = 0
    for i, p in enumerate(plan):
        if p["what"] == "frame record":
            assert f["b"][i] == 3 and g["b"][i] == 3 and v["cost"][i] == 0 and v["viterbi"][i] == 0, p
            continue
        assert f["b"][i] != 3 and v["viterbi"][i] == 1, p
        n = len(p["places"])
        assert v["cost"][i] <= n, (i, p)
        if n <= 2:
            assert bytes(recs["octets"][i]) == p["octets"] and not f["crc_bad"][i] and v["cost"][i] == n, (i, p)
            assert f["n_inexact"][i] == len({q for q in words_hit(p["places"])}), (i, p)
            twin_bad += int(g["crc_bad"][i])
        right += bytes(recs["octets"][i]) == p["octets"]
    assert twin_bad > 0
    return dict(blocks=len(plan) - 1, twin_bad_within_2=twin_bad, right=right)


def words_hit(places):
    """the code words that the channel bits `places` belong to"""
    where = {}
    for t in range(49):
        for e in range(4):
            where[bit_of(t, e)] = t
    return [where[q] for q in places]
