"""The options of the P25 voice-channel stage (rcf_chan_p25lc_opt, include/rcf.h) restated in plain Python on top of
tests/p25lc_ref.py, which stays the restatement of everything else: RCF_P25LC_ES -- an LDU2 is a unit of kind 4, 24 Hamming
words at the LDU1's places, RS(24,16,9), 12 octets of encryption sync -- and RCF_P25LC_ERASURES -- the (24,12) word's 24th
bit detects four errors, the inner words given up are the erased set of a sequential errors-and-erasures Berlekamp-Massey /
Chien / Forney walk.  `run` is p25lc_ref.run with `options`; with options 0 it gives p25lc_ref.run's records.  Below that the
other direction for the tests' signals: the LDU2's encoder, a call with a known encryption sync, the designed stream whose
units sit on and beyond every bound, and the census of what that stream guarantees."""
import numpy as np

from frames_ref import frame_walk
from rcf import native
import p25lc_ref as R
from p25lc_ref import EXP, HDU, LDU1, NONE, TLC, gdiv, gmul, poly_eval

LDU2 = 4
ES, ERASURES = native.P25LC_ES, native.P25LC_ERASURES
RS_NK = {HDU: (36, 20), LDU1: (24, 12), TLC: (24, 12), LDU2: (24, 16)}
WORDS_KIND = {HDU: HDU, LDU1: LDU1, TLC: TLC, LDU2: LDU1}        # whose places and inner code a unit's words have
DUID_OF = dict(R.DUID_OF)
DUID_OF[LDU2] = 0xA
N_OCTETS = {HDU: 15, LDU1: 9, TLC: 9, LDU2: 12}


def kind_of(duid, fd, options):
    return LDU2 if options & ES and duid == 0xA and fd > 788 else R.kind_of(duid, fd)


def golay24_detect(w):
    """the (24,12,8) word with its 24th bit taking part -> (12 data bits, 0 good / 1 fixed / 2 bad, bits changed of the 23)"""
    c, dist = R.golay23_nearest(w >> 1)
    if dist == 3 and bin(c).count("1") & 1 != w & 1:
        return w >> 12, 2, dist
    return c >> 11, int(dist > 0), dist


def erasure_locator(erased, n):
    """prod (1 + X_i x) over the erased symbols, X_i = alpha^(n - 1 - i): c[0] + c[1] x + ..."""
    c = [1]
    for i in erased:
        x = EXP[(n - 1 - i) % 63]
        c = [(c[j] if j < len(c) else 0) ^ (gmul(x, c[j - 1]) if j else 0) for j in range(len(c) + 1)]
    return c


def rs_decode(sym, n, k, erased=()):
    """-> (symbols, rs_bad, n_rs): the code word that agrees with sym outside `erased` in all but v symbols, 2 v + |erased|
    <= n - k, or sym as it is; n_rs: the symbols changed, erased ones included"""
    sym = [int(v) for v in sym]
    erased = sorted(set(int(i) for i in erased))
    d1, e = n - k, len(erased)
    if e > d1:
        return sym, 1, 0
    S = R.rs_syndromes(sym, n, k)
    C = erasure_locator(erased, n)
    B, L, m, b = list(C), e, 1, 1
    for r in range(e, d1):
        d = 0
        for i in range(min(len(C), r + 1)):
            d ^= gmul(C[i], S[r - i])
        if d == 0:
            m += 1
            continue
        T = list(C)
        f = gdiv(d, b)
        C = C + [0] * (len(B) + m - len(C))
        for i, c in enumerate(B):
            C[i + m] ^= gmul(f, c)
        if 2 * L <= r + e:
            L, B, b, m = r + 1 - L + e, T, d, 1
        else:
            m += 1
    if 2 * (L - e) + e > d1:
        return sym, 1, 0
    roots = [i for i in range(n) if poly_eval(C, EXP[(63 - (n - 1 - i)) % 63]) == 0]
    if len(roots) != L or not set(erased) <= set(roots):
        return sym, 1, 0
    omega = [0] * d1
    for i, c in enumerate(C):
        for j, s in enumerate(S):
            if i + j < d1:
                omega[i + j] ^= gmul(c, s)
    deriv = [C[i] if i % 2 else 0 for i in range(1, len(C))]
    out, n_rs = list(sym), 0
    for i in roots:
        x = EXP[(63 - (n - 1 - i)) % 63]
        den = poly_eval(deriv, x)
        v = gdiv(poly_eval(omega, x), den) if den else 0
        out[i] ^= v
        n_rs += v != 0
    if any(R.rs_syndromes(out, n, k)):
        return sym, 1, 0
    return out, 0, n_rs


def inner_decode(kind, w, options):
    """-> (data, status) of one inner word under correct = 1"""
    if WORDS_KIND[kind] == LDU1:
        return R.hamming_decode(w)
    if kind == HDU:
        return R.golay18_decode(w)[:2]
    return golay24_detect(w)[:2] if options & ERASURES else R.golay24_decode(w)[:2]


def decode_words(kind, words, correct, options=0):
    """-> (payload octets (16), rs_bad, n_rs, n_fixed, n_bad)"""
    n, k = RS_NK[kind]
    wk = WORDS_KIND[kind]
    fixed = bad = 0
    data, erased = [], []
    for w in words:
        if not correct:
            v, status = w >> (R.WORD_BITS[wk] - (12 if kind == TLC else 6)), 0
        else:
            v, status = inner_decode(kind, w, options)
        fixed += status == 1
        bad += status == 2
        if status == 2 and options & ERASURES:
            erased += [len(data), len(data) + 1] if kind == TLC else [len(data)]
        data += [v >> 6, v & 63] if kind == TLC else [v]
    rs_bad = n_rs = 0
    if correct:
        data, rs_bad, n_rs = rs_decode(data, n, k, erased)
    bits = [(v >> (5 - i)) & 1 for v in data[:k] for i in range(6)]
    return np.packbits(np.array(bits + [0] * (128 - len(bits)), np.uint8)), rs_bad, n_rs, fixed, bad


def frame_record(d, s, fd, k, dist, correct, options=0, units=None):
    info = lambda j: int(d[s + R.pos(j)])
    nid_bits = [v for j in range(24, 32) for v in (info(j) >> 1, info(j) & 1)]
    nac, duid = R.bits_int(nid_bits[:12]), R.bits_int(nid_bits[12:16])
    kind = kind_of(duid, fd, options)
    r = np.zeros(1, native.P25LC_DTYPE)
    rs_bad = n_rs = fixed = bad = 0
    if kind != NONE:
        words = R.frame_words(d, s, WORDS_KIND[kind])
        if units is not None:
            units.append((kind, words))
        r["payload"][0], rs_bad, n_rs, fixed, bad = decode_words(kind, words, correct, options)
        if kind in (LDU1, LDU2):
            lsd = [v for j in range(R.LSD_BIT // 2, R.LSD_BIT // 2 + 16) for v in (info(j) >> 1, info(j) & 1)]
            r["lsd"][0] = np.packbits(np.array(lsd, np.uint8))
    r["flags"] = (kind & 3) | (kind & 4) << 1 | rs_bad << 2 | (n_rs & 15) << 4 | (n_rs & 16) << 4 | int(dist) << 10 | duid << 16 | nac << 20
    r["k"] = k & 0xffffffff
    r["tail"] = fd | fixed << 16 | bad << 22
    return r


def run(words, k, dist, correct=1, options=0, first_hit=0, launches=None, word_cap=None, hit_cap=None, units=None):
    """p25lc_ref.run with the stage's options (ES, ERASURES) -> (records, dict of the five counters)"""
    d = R.dibits_of(words)
    k = [int(v) for v in k]
    launches = [(len(d) // 16, len(k))] if launches is None else launches
    out = []
    st = dict(n_records=0, n_frames=0, n_decoded=0, n_rs_bad=0, n_lost=0)
    for i, s, fd in frame_walk(k, launches, st, first_hit, word_cap, hit_cap, **R.WALK):
        r = frame_record(d, s, fd, k[i], dist[i], correct, options, units)
        out.append(r)
        st["n_decoded"] += int(native.p25lc_fields(r)["kind"][0]) != NONE
        st["n_rs_bad"] += int(r["flags"][0] >> 2 & 1)
    recs = np.concatenate(out) if out else np.zeros(0, native.P25LC_DTYPE)
    st["n_records"] = len(recs)
    return recs, st


# ---- the other direction
def es_octets(mi, algid, kid):
    """the 12 octets of an LDU2's encryption sync"""
    return bytes(mi) + bytes([algid]) + kid.to_bytes(2, "big")


def unit_symbols(kind, octets):
    n, k = RS_NK[kind]
    bits = np.unpackbits(np.frombuffer(bytes(octets), np.uint8))[:6 * k]
    return R.rs_encode([R.bits_int(bits[6 * i:6 * i + 6]) for i in range(k)], n, k)


def unit_words(kind, octets):
    """the clean inner words of a unit that carries these octets (N_OCTETS[kind] of them)"""
    return [R.hamming_encode(v) for v in unit_symbols(LDU2, octets)] if kind == LDU2 else R.unit_words(kind, octets)


def unit_frame(nac, kind, octets, rng, words=None, lsd=None):
    wk = WORDS_KIND[kind]
    return R.frame(nac, DUID_OF[kind], R.LENGTH[wk], rng, wk, unit_words(kind, octets) if words is None else words, lsd if wk == LDU1 else None)


CALL_ES = dict(R.CALL, mi=bytes([0xDE, 0xAD, 0xBE, 0xEF, 1, 2, 3, 4, 5]), algid=0x84, kid=0x1A2B, lsd2=bytes([0x11, 0x22, 0x33, 0x44]))


def call_dibits(seed=61):
    """-> (dibits, starts, shorts): p25lc_ref.call_dibits' call -- settle run, HDU, three times (LDU1, LDU2), TLC, a tail of
    888 -- of an encrypted transmission: HDU and every LDU2 carry CALL_ES's MI, ALGID and KID.  The second LDU2 has one
    Reed-Solomon symbol error and three single-bit errors in other Hamming words"""
    rng = np.random.default_rng(seed)
    c = CALL_ES
    lc = R.lc_group_voice(c["tgid"], c["source_id"])
    es = es_octets(c["mi"], c["algid"], c["kid"])
    frames = [unit_frame(c["nac"], HDU, R.hdu_octets(c["mi"], c["mfid"], c["algid"], c["kid"], c["tgid"]), rng)]
    shorts = ["HDU"]
    for n in range(3):
        frames.append(unit_frame(c["nac"], LDU1, lc, rng, lsd=c["lsd"]))
        words = unit_words(LDU2, es)
        if n == 1:
            words[5] = R.other_symbol_word(LDU1, words[5], rng)
            for w in (0, 11, 23):
                words[w] = R.flip_bits(words[w], [w % 10])
        frames.append(unit_frame(c["nac"], LDU2, es, rng, words=words, lsd=c["lsd2"]))
        shorts += ["LDU1", "LDU2"]
    frames.append(unit_frame(c["nac"], TLC, R.LC_TERMINATION, rng))
    shorts.append("TLC")
    starts = (1000 + np.concatenate([[0], np.cumsum([len(f) for f in frames])[:-1]])).tolist()
    d = np.concatenate([R.settle_dibits()] + frames + [rng.integers(0, 4, 888)]).astype(np.uint8)
    return d, starts, shorts


def bad_word(kind, word, rng, wrong=True):
    """an inner word that its decoder gives up (under ERASURES), made from the clean `word`; wrong: its data as read are not
    the sent ones.  Hamming: two flipped bits whose syndrome is no single bit's -- the first and the last bit, or two check
    bits (1010); (18,6): the code word of data with up to three leading bits set; (24,12): four flipped bits of the first 23,
    among the data bits or among the check bits"""
    wk = WORDS_KIND[kind]
    if wk == LDU1:
        return R.flip_bits(word, [0, 9] if wrong else [1, 3])
    if wk == HDU:
        data = (word >> 12) ^ (int(rng.integers(1, 64)) if wrong else 0)
        lead = int(rng.choice([v for v in range(1, 64) if bin(v).count("1") <= 3]))      # (within 3 of the word: the nearest)
        return (int(R.GOLAY23[lead << 6 | data]) & 0x1ffff) << 1 | 1
    places = rng.choice(12, 4, replace=False) + 12 if wrong else 1 + rng.choice(11, 4, replace=False)
    return R.flip_bits(word, [int(p) for p in places])


def with_erasures_and_errors(kind, words, e, v, rng, wrong=True):
    """e erased symbols (inner words given up; a (24,12) word is two: e even) and v symbol errors in other words"""
    words = list(words)
    per = 2 if kind == TLC else 1
    assert e % per == 0
    at = [int(w) for w in rng.choice(len(words), e // per + v, replace=False)]
    for w in at[:e // per]:
        words[w] = bad_word(kind, words[w], rng, wrong)
    for w in at[e // per:]:
        words[w] = R.other_symbol_word(WORDS_KIND[kind], words[w], rng)
    return words


def symbol_error_word(kind, word, value, half=0):
    """the valid inner word whose hexbit is `word`'s xor `value` (1 .. 63); half: which of a (24,12) word's two hexbits"""
    assert 1 <= value <= 63
    wk = WORDS_KIND[kind]
    if wk == TLC:
        return R.golay24_encode((word >> 12) ^ value << (0 if half else 6))
    d = (word >> (R.WORD_BITS[wk] - 6)) ^ value
    return R.golay18_encode(d) if wk == HDU else R.hamming_encode(d)


def with_erasures_and_errors_at(kind, words, erased, errors, rng, wrong=True):
    """with_erasures_and_errors with the places given: `erased`, the symbol positions whose inner words are given up (both
    symbols of a (24,12) word or neither), and `errors`, {symbol position: the value added to it}, outside the erased words"""
    words = list(words)
    per = 2 if kind == TLC else 1
    erased_words = sorted({i // per for i in erased})
    assert len(erased_words) * per == len(set(erased)) and not {i // per for i in errors} & set(erased_words)
    for w in erased_words:
        words[w] = bad_word(kind, words[w], rng, wrong)
    for i, value in errors.items():
        words[i // per] = symbol_error_word(kind, words[i // per], value, i % per)
    return words


# the designed stream's units: kind -> (|E|, v) pairs that decode, and pairs beyond the bound
DESIGN_OK = {LDU2: [(0, 4), (2, 3), (4, 2), (6, 1), (8, 0)], LDU1: [(0, 6), (6, 3), (12, 0)], HDU: [(0, 8), (8, 4), (16, 0)],
             TLC: [(2, 5), (8, 2), (12, 0)]}
DESIGN_BAD = {LDU2: [(0, 5), (1, 4), (9, 0)], LDU1: [(13, 0), (11, 1)], HDU: [(17, 0), (1, 8)], TLC: [(14, 0), (2, 6)]}


def designed_dibits(nac=0x293, seed=67):
    """-> (dibits, plan).  1000 dibits for the loop to settle, then back to back the units of DESIGN_OK and DESIGN_BAD --
    plan: a list of dict(start, kind, octets, e, v, what) with what = 'ok' (e erased symbols that are all wrong and v symbol
    errors, inside the bound: comes back with n_rs = e + v), 'bad' (beyond it), 'right' (an LDU2 with four erased symbols
    whose data are right: n_rs = 0) and 'clean' (an LDU2 without errors) -- and a tail of 888.  Erased Hamming words carry
    the first and the last bit flipped; the HDU with e = 16 needs n_rs's fifth bit; a TLC's erased words have four errors
    among their 12 data bits, so at least one of a word's two symbols is wrong"""
    rng = np.random.default_rng(seed)
    plan, frames = [], []

    def add(kind, e, v, what, wrong=True):
        octets = bytes(rng.integers(0, 256, N_OCTETS[kind]).astype(np.uint8))
        words = with_erasures_and_errors(kind, unit_words(kind, octets), e, v, rng, wrong)
        plan.append(dict(kind=kind, octets=octets, e=e, v=v, what=what))
        frames.append(unit_frame(nac, kind, octets, rng, words=words, lsd=bytes([e, v, 0x5A, 0xC3])))

    for kind in (LDU2, LDU1, HDU, TLC):
        for e, v in DESIGN_OK[kind]:
            add(kind, e, v, "ok")
        for e, v in DESIGN_BAD[kind]:
            add(kind, e, v, "bad")
    add(LDU2, 4, 0, "right", wrong=False)
    add(LDU2, 0, 0, "clean")
    at = 1000
    for p, f in zip(plan, frames):
        p["start"] = at
        at += len(f)
    d = np.concatenate([R.settle_dibits()] + frames + [rng.integers(0, 4, 888)]).astype(np.uint8)
    return d, plan


def check_census(recs, plain, plan):
    """the designed input's guarantees, on the restatement's records with ES | ERASURES (recs) and with ES alone (plain):
    every planted frame is there and none is lost; every 'ok' unit comes back with the sent octets, n_bad as planted and
    n_rs = e + v (a TLC: at least e / 2 + v, its erased words have at least one wrong symbol), every 'bad' one as rs_bad;
    every class of DESIGN_OK and DESIGN_BAD occurs, among them n_rs = 16; and at least one TLC with an erased four-error word
    that is repaired gives rs_bad or other octets without the option"""
    f, g = native.p25lc_fields(recs), native.p25lc_fields(plain)
    assert len(recs) == len(plain) == len(plan)
    by_k = {int(k): i for i, k in enumerate(recs["k"])}
    seen_ok, seen_bad, tlc_differs = set(), set(), 0
    for p in plan:
        i = by_k[p["start"] + 23]
        kind, per = p["kind"], 2 if p["kind"] == TLC else 1
        assert int(plain["k"][i]) == p["start"] + 23 and f["kind"][i] == g["kind"][i] == kind and f["duid"][i] == DUID_OF[kind], p
        assert f["n_bad"][i] == p["e"] // per and (kind == TLC or g["n_bad"][i] == f["n_bad"][i]), p
        sent = bytes(recs["payload"][i])[:len(p["octets"])] == p["octets"]
        if p["what"] == "bad":
            assert (f["rs_bad"][i], f["n_rs"][i]) == (1, 0), p
            seen_bad.add((kind, p["e"], p["v"]))
            continue
        assert f["rs_bad"][i] == 0 and sent and bytes(recs["payload"][i])[len(p["octets"]):] == bytes(16 - len(p["octets"])), p
        if p["what"] == "ok":
            n_rs = int(f["n_rs"][i])
            assert n_rs == p["e"] + p["v"] if kind != TLC else p["e"] // 2 + p["v"] <= n_rs <= p["e"] + p["v"], (p, n_rs)
            seen_ok.add((kind, p["e"], p["v"]))
            if kind == TLC and p["e"]:
                tlc_differs += bool(g["rs_bad"][i]) or bytes(plain["payload"][i]) != bytes(recs["payload"][i])
        if p["what"] == "right":
            assert (f["n_rs"][i], f["n_bad"][i]) == (0, 4), p
        if kind in (LDU1, LDU2):
            assert bytes(recs["lsd"][i]) == bytes([p["e"], p["v"], 0x5A, 0xC3]), p
    assert seen_ok == {(k, e, v) for k, pairs in DESIGN_OK.items() for e, v in pairs}
    assert seen_bad == {(k, e, v) for k, pairs in DESIGN_BAD.items() for e, v in pairs}
    assert 16 in f["n_rs"].tolist() and tlc_differs >= 1
