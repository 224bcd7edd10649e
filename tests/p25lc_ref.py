"""The P25 voice-channel stage (rcf_chan_p25lc, include/rcf.h) restated in plain numpy / Python over what the slicer's readers
deliver: the packed words and the (widened) sync hits.  Frames from the hits by the TSBK stage's accept rule, status symbols
stripped, NID read, and for an HDU, an LDU1 or a TLC the inner words decoded -- Hamming by its syndrome table, Golay by a
search for the nearest of all 4096 code words -- and the Reed-Solomon word by a sequential Berlekamp-Massey / Chien / Forney
walk -> records of native.P25LC_DTYPE and the stage's counters.  `launches` walks the streams as the stage sees them grow,
block by block, and models the two rings' losses.  Below that the other direction, for the tests' signals: the encoders,
the frames, the designed streams and what they guarantee."""
import numpy as np

from frames_ref import frame_walk
from rcf import native
from tsbk_ref import SYNC_DIBITS, dibits_of, pos

DECIDE = 888                                       # dibits from the frame's start that must be in whole words
FRAME = 864
WALK = dict(sync=24, accept=24, decide=DECIDE, longest=FRAME, per_word=16, cut=True)   # frames_ref.frame_walk's constants
HDU, LDU1, TLC, NONE = 0, 1, 2, 3
DUID_OF = {HDU: 0x0, LDU1: 0x5, TLC: 0xF}
LAST_DIBIT = {HDU: 389, LDU1: 788, TLC: 204}
N_WORDS = {HDU: 36, LDU1: 24, TLC: 12}
WORD_BITS = {HDU: 18, LDU1: 10, TLC: 24}
RS_NK = {HDU: (36, 20), LDU1: (24, 12), TLC: (24, 12)}
LENGTH = {HDU: 396, LDU1: 864, TLC: 216}           # dibits of the data units
LSD_BIT = 1504


def word_bit0(kind, w):
    return 112 + 18 * w if kind == HDU else 112 + (288, 472, 656, 840, 1024, 1208)[w // 4] + 10 * (w % 4) if kind == LDU1 else 112 + 24 * w


def kind_of(duid, fd):
    for kind, d in DUID_OF.items():
        if duid == d and LAST_DIBIT[kind] < fd:
            return kind
    return NONE


# ---- Hamming (10,6,3)
H_ROWS = (0b1110011000, 0b1101010100, 0b1011100010, 0b0111100001)
H_SYNDROMES = (0b1110, 0b1101, 0b1011, 0b0111, 0b0011, 0b1100, 0b1000, 0b0100, 0b0010, 0b0001)


def hamming_decode(w):
    """-> (6 data bits, 0 good / 1 fixed / 2 bad)"""
    syn = 0
    for row in H_ROWS:
        syn = syn << 1 | bin(row & w).count("1") & 1
    if syn == 0:
        return w >> 4, 0
    if syn in H_SYNDROMES:
        return (w ^ 1 << (9 - H_SYNDROMES.index(syn))) >> 4, 1
    return w >> 4, 2


def hamming_encode(d):
    w = d
    for col in (0b111001, 0b110101, 0b101110, 0b011110):
        w = w << 1 | bin(col & d).count("1") & 1
    return w


# ---- Golay (23,12,7), generator 0xC75
def golay_rem(v):
    for i in range(22, 10, -1):
        if v >> i & 1:
            v ^= 0xC75 << (i - 11)
    return v


GOLAY23 = np.array([d << 11 | golay_rem(d << 11) for d in range(4096)], np.uint32)      # code word of data d at index d
POP = np.array([bin(v).count("1") for v in range(2048)], np.uint8)


def weight23(v):
    v = np.asarray(v, np.uint32)
    return POP[v >> 12] + POP[v & 0x7ff] + ((v >> 11) & 1).astype(np.uint8)


def golay23_nearest(r):
    """the code word nearest to the 23 bits (unique, at most 3 away) -> (code word, distance)"""
    dist = weight23(GOLAY23 ^ np.uint32(r))
    at = int(np.argmin(dist))
    assert dist[at] <= 3 and np.count_nonzero(dist == dist[at]) == 1
    return int(GOLAY23[at]), int(dist[at])


def golay24_decode(w):
    """-> (12 data bits, 0 good / 1 fixed, bits changed)"""
    c, dist = golay23_nearest(w >> 1)
    return c >> 11, int(dist > 0), dist


def golay18_decode(w):
    """-> (6 data bits, 0 good / 1 fixed / 2 bad, bits changed)"""
    c, dist = golay23_nearest(w >> 1)
    if c >> 17:
        return w >> 12, 2, dist
    return c >> 11, int(dist > 0), dist


def golay24_encode(d):
    c = int(GOLAY23[d])
    return c << 1 | bin(c).count("1") & 1


def golay18_encode(d):
    return golay24_encode(d)                       # six leading zero data bits


# ---- GF(64), x^6 + x + 1, and RS(n, k) with the roots alpha^1 .. alpha^(n - k)
EXP, LOG = [0] * 126, [0] * 64
_v = 1
for _e in range(63):
    EXP[_e] = EXP[_e + 63] = _v
    LOG[_v] = _e
    _v <<= 1
    if _v & 0x40:
        _v ^= 0x43


def gmul(a, b):
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def gdiv(a, b):
    return EXP[LOG[a] + 63 - LOG[b]] if a else 0


def poly_eval(p, x):
    """p[0] + p[1] x + ..."""
    v = 0
    for c in reversed(p):
        v = gmul(v, x) ^ c
    return v


def rs_syndromes(sym, n, k):
    return [poly_eval(list(reversed(sym)), EXP[j]) for j in range(1, n - k + 1)]


def rs_decode(sym, n, k):
    """-> (symbols, rs_bad, n_rs): the code word within t of sym, or sym as it is"""
    sym = [int(v) for v in sym]
    t = (n - k) // 2
    S = rs_syndromes(sym, n, k)
    C, B, L, m, b = [1], [1], 0, 1, 1
    for r in range(2 * t):
        d = S[r]
        for i in range(1, L + 1):
            if i < len(C):
                d ^= gmul(C[i], S[r - i])
        if d == 0:
            m += 1
            continue
        T = list(C)
        f = gdiv(d, b)
        C = C + [0] * (len(B) + m - len(C))
        for i, c in enumerate(B):
            C[i + m] ^= gmul(f, c)
        if 2 * L <= r:
            L, B, b, m = r + 1 - L, T, d, 1
        else:
            m += 1
    if L > t:
        return sym, 1, 0
    roots = [i for i in range(n) if poly_eval(C, EXP[(63 - (n - 1 - i)) % 63]) == 0]
    if len(roots) != L:
        return sym, 1, 0
    omega = [0] * (2 * t)
    for i, c in enumerate(C):
        for j, s in enumerate(S):
            if i + j < 2 * t:
                omega[i + j] ^= gmul(c, s)
    deriv = [C[i] if i % 2 else 0 for i in range(1, len(C))]          # d/dx: the odd coefficients, one degree down
    out, n_rs = list(sym), 0
    for i in roots:
        x = EXP[(63 - (n - 1 - i)) % 63]
        den = poly_eval(deriv, x)
        e = gdiv(poly_eval(omega, x), den) if den else 0
        out[i] ^= e
        n_rs += e != 0
    if any(rs_syndromes(out, n, k)):
        return sym, 1, 0
    return out, 0, n_rs


def rs_generator(n, k):
    g = [1]                                        # g[0] + g[1] x + ...
    for j in range(1, n - k + 1):
        g = [(g[i - 1] if i else 0) ^ (gmul(g[i], EXP[j]) if i < len(g) else 0) for i in range(len(g) + 1)]
    return g


def rs_encode(data, n, k):
    """k data symbols -> the n symbols of the code word, data first"""
    g = rs_generator(n, k)
    rem = [int(v) for v in data] + [0] * (n - k)   # the highest power first
    for i in range(k):
        c = rem[i]
        if c:
            for j in range(1, n - k + 1):
                rem[i + j] ^= gmul(c, g[n - k - j])
    return [int(v) for v in data] + rem[k:]


# ---- a frame's records
def bits_int(bits):
    v = 0
    for b in bits:
        v = v << 1 | int(b)
    return v


def frame_words(d, s, kind):
    """the inner words of the unit in the frame at stream dibit s"""
    out = []
    for w in range(N_WORDS[kind]):
        j0, nd = word_bit0(kind, w) // 2, WORD_BITS[kind] // 2
        out.append(bits_int(v for j in range(j0, j0 + nd) for v in (int(d[s + pos(j)]) >> 1, int(d[s + pos(j)]) & 1)))
    return out


def decode_words(kind, words, correct):
    """-> (payload octets (16), rs_bad, n_rs, n_fixed, n_bad)"""
    n, k = RS_NK[kind]
    fixed = bad = 0
    data = []
    for w in words:
        if not correct:
            v, status = w >> (WORD_BITS[kind] - (12 if kind == TLC else 6)), 0
        elif kind == LDU1:
            v, status = hamming_decode(w)
        elif kind == HDU:
            v, status, _ = golay18_decode(w)
        else:
            v, status, _ = golay24_decode(w)
        fixed += status == 1
        bad += status == 2
        data += [v >> 6, v & 63] if kind == TLC else [v]
    rs_bad = n_rs = 0
    if correct:
        data, rs_bad, n_rs = rs_decode(data, n, k)
    bits = [(v >> (5 - i)) & 1 for v in data[:k] for i in range(6)]
    return np.packbits(np.array(bits + [0] * (128 - len(bits)), np.uint8)), rs_bad, n_rs, fixed, bad


def frame_record(d, s, fd, k, dist, correct, units=None):
    info = lambda j: int(d[s + pos(j)])
    nid_bits = [v for j in range(24, 32) for v in (info(j) >> 1, info(j) & 1)]
    nac, duid = bits_int(nid_bits[:12]), bits_int(nid_bits[12:16])
    kind = kind_of(duid, fd)
    r = np.zeros(1, native.P25LC_DTYPE)
    rs_bad = n_rs = fixed = bad = 0
    if kind != NONE:
        words = frame_words(d, s, kind)
        if units is not None:
            units.append((kind, words))
        r["payload"][0], rs_bad, n_rs, fixed, bad = decode_words(kind, words, correct)
        if kind == LDU1:
            lsd = [v for j in range(LSD_BIT // 2, LSD_BIT // 2 + 16) for v in (info(j) >> 1, info(j) & 1)]
            r["lsd"][0] = np.packbits(np.array(lsd, np.uint8))
    r["flags"] = kind | rs_bad << 2 | n_rs << 4 | int(dist) << 10 | duid << 16 | nac << 20
    r["k"] = k & 0xffffffff
    r["tail"] = fd | fixed << 16 | bad << 22
    return r


def run(words, k, dist, correct=1, first_hit=0, launches=None, word_cap=None, hit_cap=None, units=None):
    """-> (records, dict(n_records, n_frames, n_decoded, n_rs_bad, n_lost)).  words, k, dist: the slicer's streams from its
    start; first_hit: the slicer's n_hits when the stage was attached; launches: [(n_words, n_hits)] after each block (default:
    one, at the end); word_cap / hit_cap: the rings' capacities (default: nothing is ever overwritten); units: a list that
    takes (kind, inner words) of every unit decoded, in the records' order"""
    d = dibits_of(words)
    k = [int(v) for v in k]
    launches = [(len(d) // 16, len(k))] if launches is None else launches
    out = []
    st = dict(n_records=0, n_frames=0, n_decoded=0, n_rs_bad=0, n_lost=0)
    for i, s, fd in frame_walk(k, launches, st, first_hit, word_cap, hit_cap, **WALK):
        r = frame_record(d, s, fd, k[i], dist[i], correct, units)
        out.append(r)
        st["n_decoded"] += int(r["flags"][0] & 3) != NONE
        st["n_rs_bad"] += int(r["flags"][0] >> 2 & 1)
    recs = np.concatenate(out) if out else np.zeros(0, native.P25LC_DTYPE)
    st["n_records"] = len(recs)
    return recs, st


# ---- the other direction: octets -> inner words -> a data unit's dibits
def unit_words(kind, octets):
    """the clean inner words of a unit that carries these octets (15 for an HDU, 9 for an LDU1 or a TLC)"""
    n, k = RS_NK[kind]
    bits = np.unpackbits(np.frombuffer(bytes(octets), np.uint8))[:6 * k]
    sym = rs_encode([bits_int(bits[6 * i:6 * i + 6]) for i in range(k)], n, k)
    if kind == HDU:
        return [golay18_encode(v) for v in sym]
    if kind == LDU1:
        return [hamming_encode(v) for v in sym]
    return [golay24_encode(sym[2 * i] << 6 | sym[2 * i + 1]) for i in range(12)]


def word_symbols(kind, words):
    """the systematic hexbits of inner words"""
    if kind == TLC:
        return [v for w in words for v in (w >> 18, w >> 12 & 63)]
    return [w >> (WORD_BITS[kind] - 6) for w in words]


def frame(nac, duid, total, rng, kind=NONE, words=(), lsd=None, fill=True):
    """a data unit's dibits: sync, NID (nac, duid and 48 bits nobody checks), random bits (fill=False: nulls) with the unit's
    inner words and the LSD octets at their places, a status dibit behind every 35 info dibits; `total` dibits in all"""
    n_info = 2 * (total - total // 36)
    bits = rng.integers(0, 2, n_info).astype(np.uint8) if fill else np.zeros(n_info, np.uint8)
    head = [v for d in SYNC_DIBITS for v in (d >> 1, d & 1)]
    nid = (nac << 52) | (duid << 48) | int(rng.integers(0, 1 << 48))
    head += [(nid >> (63 - i)) & 1 for i in range(64)]
    bits[:112] = head
    for w, word in enumerate(words):
        b0, nb = word_bit0(kind, w), WORD_BITS[kind]
        bits[b0:b0 + nb] = [(word >> (nb - 1 - i)) & 1 for i in range(nb)]
    if lsd is not None:
        bits[LSD_BIT:LSD_BIT + 32] = np.unpackbits(np.frombuffer(bytes(lsd), np.uint8))
    info = 2 * bits[0::2] + bits[1::2]
    out = []
    for j, v in enumerate(info):
        out.append(int(v))
        if j % 35 == 34:
            out.append(int(rng.integers(0, 4)))
    assert len(out) == total
    return np.array(out, np.uint8)


def unit_frame(nac, kind, octets, rng, words=None, lsd=None):
    return frame(nac, DUID_OF[kind], LENGTH[kind], rng, kind, unit_words(kind, octets) if words is None else words, lsd if kind == LDU1 else None)


def lc_group_voice(tgid, source_id, emergency=0):
    """the 9 octets of a Group Voice Channel User link control word"""
    return bytes([0x00, 0x00, emergency << 7, 0x00]) + tgid.to_bytes(2, "big") + source_id.to_bytes(3, "big")


LC_TERMINATION = bytes([0x15, 0x00]) + bytes(7)    # Call Termination / Cancellation


def hdu_octets(mi, mfid, algid, kid, tgid):
    return bytes(mi) + bytes([mfid, algid]) + kid.to_bytes(2, "big") + tgid.to_bytes(2, "big")


def other_symbol_word(kind, word, rng):
    """a valid inner word for another hexbit (a TLC word: another first hexbit): a Reed-Solomon symbol error that the inner
    decoder cannot hide"""
    if kind == TLC:
        d = word >> 12
        return golay24_encode(((d >> 6) ^ int(rng.integers(1, 64))) << 6 | d & 63)
    d = (word >> (WORD_BITS[kind] - 6)) ^ int(rng.integers(1, 64))
    return golay18_encode(d) if kind == HDU else hamming_encode(d)


def with_symbol_errors(kind, words, n_errors, rng):
    words = list(words)
    for w in rng.choice(len(words), n_errors, replace=False):
        words[int(w)] = other_symbol_word(kind, words[int(w)], rng)
    return words


def flip_bits(word, places):
    for p in places:
        word ^= 1 << p
    return word


def settle_dibits():
    """1000 dibits for the C4FM loop to settle on.  How long the loop takes depends on the dibits: over random runs of 1000
    its restatement (tests/fsk4_ref.py) stands after 150 to 1250 of them; on this run it stands after 300"""
    return np.random.default_rng(25).integers(0, 4, 1000).astype(np.uint8)


CALL = dict(nac=0x293, tgid=0x1234, source_id=0xABCDEF, mi=bytes(range(1, 10)), mfid=0x00, algid=0x80, kid=0x0000, lsd=bytes([0xC3, 0x5A, 0x0F, 0x99]))


def call_dibits(seed=53):
    """-> (dibits, starts, shorts).  A voice call of about 7700 dibits: 1000 for the loop to settle, then back to back an HDU,
    three times (LDU1, LDU2) and a TLC, and a tail of 888.  The second LDU1 carries two Reed-Solomon symbol errors and four
    single-bit errors in other Hamming words; everything else is clean."""
    rng = np.random.default_rng(seed)
    c = CALL
    lc = lc_group_voice(c["tgid"], c["source_id"])
    frames = [unit_frame(c["nac"], HDU, hdu_octets(c["mi"], c["mfid"], c["algid"], c["kid"], c["tgid"]), rng)]
    shorts = ["HDU"]
    for n in range(3):
        words = unit_words(LDU1, lc)
        if n == 1:
            words = with_symbol_errors(LDU1, words, 2, np.random.default_rng(3))
            sent = unit_words(LDU1, lc)
            clean = [w for w in range(24) if words[w] == sent[w]]
            for w in clean[:4]:
                words[w] = flip_bits(words[w], [w % 10])
        frames.append(unit_frame(c["nac"], LDU1, lc, rng, words=words, lsd=c["lsd"]))
        frames.append(frame(c["nac"], 0xA, 864, rng))
        shorts += ["LDU1", "LDU2"]
    frames.append(unit_frame(c["nac"], TLC, LC_TERMINATION, rng))
    shorts.append("TLC")
    starts = (1000 + np.concatenate([[0], np.cumsum([len(f) for f in frames])[:-1]])).tolist()
    d = np.concatenate([settle_dibits()] + frames + [rng.integers(0, 4, 888)]).astype(np.uint8)
    return d, starts, shorts


def designed_dibits(nac=0x293, seed=57):
    """-> (dibits, plan).  1000 dibits for the loop to settle, then back to back the frames of `plan`, a list of dict(start,
    kind, duid, octets, what, n): units whose inner words are wrong on purpose, so that the decoders' correcting paths are
    walked -- what = 'rs': n symbol errors (1 .. t + 1) planted as valid inner words of other hexbits; 'inner': inner words
    with 1, 2, 3 flipped bits (Golay) or one and two (Hamming; the two are the first and the last bit, whose syndrome is no
    column's); 'lead': an (18,6) word that lies within 3 of a code word with leading data bits set; 'short': an HDU that the
    next frame cuts at 300 dibits; 'plain': a data unit without link control (LDU2, TnoLC, TSDU, PDU) -- and a tail of 888"""
    rng = np.random.default_rng(seed)
    plan, frames = [], []

    def add(kind, duid, what, n, f, octets=None):
        plan.append(dict(kind=kind, duid=duid, what=what, n=n, octets=octets))
        frames.append(f)

    for kind in (HDU, LDU1, TLC):
        t = (RS_NK[kind][0] - RS_NK[kind][1]) // 2
        for n in range(1, t + 2):
            octets = bytes(rng.integers(0, 256, 15 if kind == HDU else 9).astype(np.uint8))
            words = with_symbol_errors(kind, unit_words(kind, octets), n, rng)
            add(kind, DUID_OF[kind], "rs", n, unit_frame(nac, kind, octets, rng, words=words, lsd=bytes(4)), octets)
        octets = bytes(rng.integers(0, 256, 15 if kind == HDU else 9).astype(np.uint8))
        words = unit_words(kind, octets)
        if kind == LDU1:
            for w in range(10):
                words[w] = flip_bits(words[w], [w])
            words[10] = flip_bits(words[10], [0, 9])
        else:
            nb = WORD_BITS[kind]
            for w in range(9):                       # 1, 2, 3 bits of the first 23 (bit 0 of the word is the 24th)
                words[w] = flip_bits(words[w], [int(p) for p in 1 + rng.choice(nb - 1, 1 + w % 3, replace=False)])
            words[9] = flip_bits(words[9], [0])      # the 24th bit alone: nothing to fix
        add(kind, DUID_OF[kind], "inner", 0, unit_frame(nac, kind, octets, rng, words=words, lsd=bytes([1, 2, 3, 4])), octets)
    octets = bytes(rng.integers(0, 256, 15).astype(np.uint8))
    words = unit_words(HDU, octets)
    for w, lead in ((3, 0b000001), (7, 0b010100), (11, 0b100011)):
        c = int(GOLAY23[lead << 6 | (words[w] >> 12)])
        words[w] = (c & 0x1ffff) << 1 | 1
    add(HDU, 0x0, "lead", 3, unit_frame(nac, HDU, octets, rng, words=words), octets)
    add(NONE, 0x0, "short", 300, unit_frame(nac, HDU, octets, rng)[:300])
    for duid, total in ((0xA, 864), (0x3, 72), (0x7, 360), (0xC, 216), (0xA, 864)):
        add(NONE, duid, "plain", total, frame(nac, duid, total, rng))
    at = 1000
    for p, f in zip(plan, frames):
        p["start"] = at
        at += len(f)
    d = np.concatenate([settle_dibits()] + frames + [rng.integers(0, 4, 888)]).astype(np.uint8)
    return d, plan


def check_census(recs, units, plan):
    """the designed input's guarantees, on the restatement's records (correct = 1) and the units it decoded: every planted
    frame is there; n symbol errors come back as n_rs = n with the sent octets for n = 1 .. t, as rs_bad for n = t + 1, for
    both Reed-Solomon codes; Hamming words fixed and bad; Golay words fixed with 1, 2 and 3 bits, in both word lengths; an
    (18,6) word given up for its leading bits; every kind of record"""
    f = native.p25lc_fields(recs)
    by_k = {int(k): i for i, k in enumerate(recs["k"])}
    seen_rs = {HDU: set(), LDU1: set(), TLC: set()}
    seen_bad = set()
    for p in plan:
        i = by_k[p["start"] + 23]
        assert f["kind"][i] == p["kind"] and f["duid"][i] == p["duid"], p
        if p["what"] == "rs":
            t = (RS_NK[p["kind"]][0] - RS_NK[p["kind"]][1]) // 2
            if p["n"] <= t:
                assert (f["rs_bad"][i], f["n_rs"][i]) == (0, p["n"]) and bytes(recs["payload"][i])[:len(p["octets"])] == p["octets"], p
                seen_rs[p["kind"]].add(p["n"])
            else:
                assert (f["rs_bad"][i], f["n_rs"][i]) == (1, 0), p
                seen_bad.add(p["kind"])
        if p["what"] == "inner":
            assert f["rs_bad"][i] == 0 and f["n_rs"][i] == (1 if p["kind"] == LDU1 else 0), p   # the Hamming word given up is a symbol error
            assert bytes(recs["payload"][i])[:len(p["octets"])] == p["octets"]
            assert (f["n_fixed"][i], f["n_bad"][i]) == ((10, 1) if p["kind"] == LDU1 else (9, 0)), p
        if p["what"] == "lead":
            assert (f["n_bad"][i], f["n_rs"][i], f["rs_bad"][i]) == (3, 0, 0), p
        if p["what"] == "short":
            assert f["frame_dibits"][i] == 300
    assert seen_rs == {HDU: set(range(1, 9)), LDU1: set(range(1, 7)), TLC: set(range(1, 7))} and seen_bad == {HDU, LDU1, TLC}
    assert set(f["kind"].tolist()) == {0, 1, 2, 3}
    golay_bits = {HDU: set(), TLC: set()}
    hamming = set()
    lead = 0
    for kind, words in units:
        for w in words:
            if kind == LDU1:
                hamming.add(hamming_decode(w)[1])
            else:
                _, status, dist = golay18_decode(w) if kind == HDU else golay24_decode(w)
                if status == 1:
                    golay_bits[kind].add(dist)
                lead += status == 2
    assert hamming == {0, 1, 2} and golay_bits == {HDU: {1, 2, 3}, TLC: {1, 2, 3}} and lead >= 3
