"""The NID option of the two P25 stages (RCF_NID_BCH: rcf_chan_tsbk_ex, rcf_chan_p25lc_ex, include/rcf.h) restated in plain
numpy / Python by a method the kernel does not share: the nearest code word of BCH(63,16,23) by exhaustive search over all
65536 code words, xor and popcount -- complete and obviously right.  A word is an int of 63 bits, code bit 0 (the nac's first
bit) highest.  `run_tsbk` and `run_voice` are tsbk_ref.run and p25es_ref.run with the rule applied per frame: they wrap those
restatements' per-frame functions and leave the modules as they are.  Below that the other direction for the tests'
signals: the encoder `nid(nac, duid)`, frames with a given NID, the designed stream and the census of what it guarantees."""
import numpy as np

from rcf import native
import p25es_ref as E
import p25lc_ref as R
import tsbk_ref as T

GENERATOR = 0o6331141367235453          # degree 47
T_MAX, BAD = 11, 15
MASK63 = (1 << 63) - 1


def encode(data16):
    """the systematic code word of 16 data bits: the data, then the remainder of data x^47 by the generator"""
    v = rem = (data16 & 0xffff) << 47
    for e in range(62, 46, -1):
        if rem >> e & 1:
            rem ^= GENERATOR << (e - 47)
    return v | rem


def nid(nac, duid):
    return encode((nac & 0xfff) << 4 | (duid & 15))


def _all_words():
    words = np.zeros(1, np.uint64)
    for b in range(16):
        words = np.concatenate([words, words ^ np.uint64(encode(1 << b))])
    return words


def popcount(x):
    return np.unpackbits(np.ascontiguousarray(x, dtype=np.uint64).view(np.uint8)).reshape(-1, 64).sum(axis=1)


WORDS = _all_words()                    # all 65536 code words (index i is NOT the data; the data are a word's top 16 bits)
WEIGHTS = popcount(WORDS)


def decode(r):
    """the 63 received bits -> (the word to read nac and duid from, nid_fix): the code word within 11 bits, or r and 15"""
    r = int(r) & MASK63
    dist = popcount(WORDS ^ np.uint64(r))
    at = int(np.argmin(dist))
    return (int(WORDS[at]), int(dist[at])) if dist[at] <= T_MAX else (r, BAD)


def flip(word, places):
    """code bits `places` (0 .. 62, bit 0 the first) flipped"""
    for p in places:
        word ^= 1 << (62 - int(p))
    return word


def support(word):
    return [i for i in range(63) if word >> (62 - i) & 1]


# ---- the rule on top of the two restatements
def nid_places(s):
    """the stream dibits of a frame's 32 NID dibits (frame start s)"""
    return [s + T.pos(24 + j) for j in range(32)]


def received64(d, s):
    v = 0
    for p in nid_places(s):
        v = v << 2 | int(d[p])
    return v


def _with_rule(d, s, st, call):
    """call() with the frame's NID dibits replaced by the decoded word's (the 64th bit as received) -> (its result, received
    64 bits, nid_fix); the stream is put back"""
    r64 = received64(d, s)
    word, fix = decode(r64 >> 1)
    st["n_decoded"] += 1
    st["n_bad"] += fix == BAD
    st["n_fixed"] += 0 < fix < BAD
    st["n_bits"] += fix if fix < BAD else 0
    places = nid_places(s)
    old = [int(d[p]) for p in places]
    new64 = word << 1 | (r64 & 1)
    for j, p in enumerate(places):
        d[p] = (new64 >> (62 - 2 * j)) & 3
    try:
        out = call()
    finally:
        for p, v in zip(places, old):
            d[p] = v
    return out, r64, fix


def _empty_state():
    return dict(n_decoded=0, n_fixed=0, n_bits=0, n_bad=0)


def run_tsbk(words, k, dist, nid=1, **kw):
    """tsbk_ref.run under RCF_NID_BCH (nid=0: tsbk_ref.run itself) -> (records, the five counters, rcf_nid_state_t's four)"""
    st = _empty_state()
    if not nid:
        return T.run(words, k, dist, **kw) + (st,)
    plain = T.frame_records

    def frame_records(d, s, fd, kk, dd, blocks=None):
        recs, r64, fix = _with_rule(d, s, st, lambda: plain(d, s, fd, kk, dd, blocks))
        recs["nid"] = np.frombuffer(r64.to_bytes(8, "big"), np.uint8)          # words 5-6 keep the bits as received
        recs["frame_dibits"] |= fix << 16 | 1 << 20
        return recs

    T.frame_records = frame_records
    try:
        recs, tst = T.run(words, k, dist, **kw)
    finally:
        T.frame_records = plain
    return recs, tst, st


def run_voice(words, k, dist, nid=1, **kw):
    """p25es_ref.run under RCF_NID_BCH (nid=0: p25es_ref.run itself) -> (records, the five counters, the NID's four)"""
    st = _empty_state()
    if not nid:
        return E.run(words, k, dist, **kw) + (st,)
    plain = E.frame_record

    def frame_record(d, s, fd, kk, dd, correct, options=0, units=None):
        r, _, fix = _with_rule(d, s, st, lambda: plain(d, s, fd, kk, dd, correct, options, units))
        r["flags"] |= 1 << 9
        r["tail"] |= fix << 28
        return r

    E.frame_record = frame_record
    try:
        recs, vst = E.run(words, k, dist, **kw)
    finally:
        E.frame_record = plain
    return recs, vst, st


# ---- the other direction
def set_nid(frame, nid64):
    """a frame's dibits (from its sync word on) with these 64 NID bits"""
    frame = np.array(frame, np.uint8)
    for j, p in enumerate(nid_places(0)):
        frame[p] = (nid64 >> (62 - 2 * j)) & 3
    return frame


def beyond_every_word(word, rng, weight=12):
    """`word` with `weight` flipped bits so that no code word lies within 11 bits (searched; most patterns of 12 do)"""
    for _ in range(200):
        places = sorted(int(p) for p in rng.choice(63, weight, replace=False))
        if decode(flip(word, places))[1] == BAD:
            return places
    raise AssertionError("no pattern found")


def toward_another_word(rng, n_flips):
    """places: n_flips of the support of a random weight-23 code word"""
    other = int(WORDS[rng.choice(np.flatnonzero(WEIGHTS == 23))])
    return sorted(int(p) for p in rng.choice(support(other), n_flips, replace=False)), other


# what the designed frames carry, per stage: (name, sent duid, flipped code bits or a callable(word, rng) -> places,
# flip the 64th bit) -- the weights 0 .. 11 among them, bit 0, bit 62 and the bits 21 and 22 either side of the status symbol
def _weights_plan(rng):
    plan = [("w0", []), ("w1 first", [0]), ("w1 last", [62]), ("w2 status", [21, 22])]
    for w in range(3, 12):
        fixed = [0, 62] if w % 2 else [21, 22]
        rest = [p for p in range(63) if p not in fixed and not 12 <= p < 16]       # (the duid stays: these frames decode either way)
        plan.append(("w%d" % w, sorted(fixed + [int(p) for p in rng.choice(rest, w - len(fixed), replace=False)])))
    return plan


def designed_dibits(stage, nac=0x293, seed=71):
    """-> (dibits, plan) for stage 'tsbk' or 'voice'.  1000 dibits to settle, then back to back frames whose NID carries a
    planned pattern -- plan: list of dict(start, what, sent_duid, places, bit64, fix: the nid_fix the rule gives, read_duid,
    kind) -- and a tail.  tsbk: every frame a TSDU (sent duid 7 unless said) of one valid block.  voice: HDU, LDU1, LDU2, TLC
    in turn."""
    rng = np.random.default_rng(seed)
    items = [dict(what=w, places=p) for w, p in _weights_plan(rng)]
    items.append(dict(what="bit64", places=[], bit64=1))
    items.append(dict(what="beyond", places=None))
    items.append(dict(what="other word", places=None))
    if stage == "tsbk":
        items.append(dict(what="duid 3 -> 7", places=[13]))                  # 0111 read as 0011
        items.append(dict(what="duid 7 -> 5", sent_duid=5, places=[14]))     # 0101 read as 0111
    else:
        for kind in (E.HDU, E.LDU1, E.LDU2, E.TLC):
            items.append(dict(what="broken duid", kind=kind, places=[12 + int(rng.integers(0, 4)), 40]))
    frames, at = [], 1000
    for n, it in enumerate(items):
        kind = it.get("kind", (E.HDU, E.LDU1, E.LDU2, E.TLC)[n % 4]) if stage == "voice" else None
        sent_duid = it.get("sent_duid", E.DUID_OF[kind] if stage == "voice" else 7)
        word = nid(nac, sent_duid)
        if it["what"] == "beyond":
            it["places"] = beyond_every_word(word, rng)
        if it["what"] == "other word":
            it["places"], other = toward_another_word(rng, 12)
            it["other"] = other
        r63 = flip(word, it["places"])
        bit64 = int(rng.integers(0, 2))
        nid64 = r63 << 1 | bit64 ^ it.get("bit64", 0)
        if stage == "tsbk":
            f = T.frame(nac, 7, [T.tsbk_octets(rng)], rng)
        else:
            octets = bytes(rng.integers(0, 256, E.N_OCTETS[kind]).astype(np.uint8))
            f = E.unit_frame(nac, kind, octets, rng, lsd=bytes([n, 0x5A, 0xC3, 0x0F]))
            it["octets"] = octets
        f = set_nid(f, nid64)
        got, fix = decode(r63)
        it.update(start=at, kind=kind, nac=nac, sent_duid=sent_duid, fix=fix, read_duid=r63 >> 47 & 15, decoded_duid=got >> 47 & 15,
                  decoded_nac=got >> 51, read_nac=r63 >> 51)
        frames.append(f)
        at += len(f)
    d = np.concatenate([R.settle_dibits()] + frames + [rng.integers(0, 4, 888)]).astype(np.uint8)
    return d, items


def check_census(stage, recs, raw, plan):
    """the designed input's guarantees, on the restatement's records with the option (recs) and without (raw): every planted
    frame is there; nid_fix is the planned one -- every weight 0 .. 11, the 64th bit alone 0, the word beyond every code word
    15 with its fields as read, the crafted word 11 toward the other code word --; every frame with a broken duid decodes
    with the option and is a bare frame record without; the TSDU that reads 7 and decodes to 5 has no block with the option"""
    n = native.nid_fields(recs)
    f = native.tsbk_fields(recs) if stage == "tsbk" else native.p25lc_fields(recs)
    g = native.tsbk_fields(raw) if stage == "tsbk" else native.p25lc_fields(raw)
    bare = (lambda x, i: x["b"][i] == 3) if stage == "tsbk" else (lambda x, i: x["kind"][i] == 3)
    first = {}
    for i, kk in enumerate(recs["k"]):
        first.setdefault(int(kk), i)
    first_raw = {}
    for i, kk in enumerate(raw["k"]):
        first_raw.setdefault(int(kk), i)
    assert len(first) == len(first_raw) == len(plan) and np.all(n["nid_decoded"] == 1) and not np.any(native.nid_fields(raw)["nid_decoded"])
    seen = set()
    for p in plan:
        i, j = first[p["start"] + 23], first_raw[p["start"] + 23]
        assert int(n["nid_fix"][i]) == p["fix"], p
        assert (int(f["duid"][i]), int(f["nac"][i])) == (p["decoded_duid"], p["decoded_nac"]), p
        assert (int(g["duid"][j]), int(g["nac"][j])) == (p["read_duid"], p["read_nac"]), p
        seen.add(p["fix"])
        what = p["what"]
        if what == "beyond":
            assert p["fix"] == BAD and len(p["places"]) == 12 and (p["decoded_duid"], p["decoded_nac"]) == (p["read_duid"], p["read_nac"])
        elif what == "other word":
            sent = nid(p["nac"], p["sent_duid"]) ^ p["other"]
            assert p["fix"] == 11 and len(p["places"]) == 12 and (p["decoded_nac"], p["decoded_duid"]) == (sent >> 51, sent >> 47 & 15), p
        elif what == "bit64":
            assert p["fix"] == 0
        else:
            assert p["fix"] == len(p["places"]) and p["decoded_duid"] == p["sent_duid"], p
        if what == "duid 3 -> 7":
            assert p["read_duid"] == 3 and not bare(f, i) and not f["crc_bad"][i] and bare(g, j), p
        if what == "duid 7 -> 5":
            assert p["read_duid"] == 7 and bare(f, i) and not bare(g, j), p
        if what == "broken duid":
            assert p["read_duid"] != p["sent_duid"] and int(f["kind"][i]) == p["kind"] and not f["rs_bad"][i] and bare(g, j), p
            assert bytes(recs["payload"][i])[:len(p["octets"])] == p["octets"], p
    assert seen >= set(range(12)) | {BAD}, seen
    if stage == "voice":
        assert {p["kind"] for p in plan if p["what"] == "broken duid"} == {E.HDU, E.LDU1, E.LDU2, E.TLC}
    places = {q for p in plan if p["fix"] not in (0, BAD) for q in p["places"]}
    assert {0, 62, 21, 22} <= places
