"""Dense code words for the wave-form algebraic decoders of the P25 stages (rs_decode<false>, rs_decode<true> in p25lc.hip,
nid_decode_wave in nid_wave.hpp): streams whose units walk Chien, Forney and the re-check on words that decode, at every
(|E|, v) pair inside the bound, at every symbol position and at both ends of the word, and NIDs with every single wrong bit
and a dozen patterns per weight.  The generators stand on tests/p25lc_ref.py, tests/p25es_ref.py and tests/nid_ref.py; the
censuses say what the streams guarantee, on the restatements' records.  tests/test_codewords_cpu.py holds both without a
device, tests/test_gpu_codewords.py sends the streams through the kernels."""
import numpy as np

from rcf import native
import nid_ref as N
import p25es_ref as E
import p25lc_ref as R
import tsbk_ref as T

HDU, LDU1, TLC, LDU2 = E.HDU, E.LDU1, E.TLC, E.LDU2
SERIES = (HDU, LDU1, TLC, LDU2)                    # one per code path: (18,6) words, Hamming words, (24,12) words, RS(24,16,9)
CLASSES = ("inside", "right", "pos_err", "pos_era", "full", "beyond")


def _per(kind):
    return 2 if kind == TLC else 1                 # symbols of an inner word


def inside_pairs(kind):
    """every (|E|, v) with 2 v + |E| <= d - 1 (a (24,12) word is two symbols: |E| even)"""
    n, k = E.RS_NK[kind]
    return [(e, v) for v in range((n - k) // 2 + 1) for e in range(0, n - k - 2 * v + 1, _per(kind))]


def beyond_pairs(kind):
    """every (|E|, v) with 2 v + |E| = d.  d is odd and a TLC's |E| is even, so no such pair exists there: a TLC takes the
    pairs with 2 v + |E| = d + 1, the nearest it can stand beyond its bound"""
    n, k = E.RS_NK[kind]
    total = n - k + _per(kind)
    return [(total - 2 * v, v) for v in range(total // 2 + 1)]


def right_pairs(kind):
    n, k = E.RS_NK[kind]
    return [(n - k, 0), (2, (n - k) // 2 - 1), (4, 1)]


def _series_units(kind, rng):
    """the units of one series -> list of dict(what, e, v, erased: symbol positions, errors: {symbol position: value}, wrong)"""
    n, k = E.RS_NK[kind]
    d1, per = n - k, _per(kind)
    t = d1 // 2
    units = []

    def add(what, erased, errors, wrong=True):
        units.append(dict(what=what, e=len(erased), v=len(errors), erased=sorted(int(i) for i in erased),
                          errors={int(i): int(x) for i, x in errors.items()}, wrong=wrong))

    def drawn(what, e, v, wrong=True):
        at = [int(w) for w in rng.choice(n // per, e // per + v, replace=False)]
        erased = [per * w + h for w in at[:e // per] for h in range(per)]
        add(what, erased, {per * w + int(rng.integers(0, per)): int(rng.integers(1, 64)) for w in at[e // per:]}, wrong)

    for e, v in inside_pairs(kind):
        drawn("inside", e, v)
    for e, v in right_pairs(kind):
        drawn("right", e, v, wrong=False)
    for j in range(n // 2):                        # errors only: every position once, the values 1 and 63 among them
        a, b = (1, 63) if j == 0 else (int(rng.integers(1, 64)), int(rng.integers(1, 64)))
        add("pos_err", [], {j: a, j + n // 2: b})
    ends = list(range(per)) + list(range(n - per, n))
    add("pos_era", ends, {per: int(rng.integers(1, 64)), n - 1 - per: int(rng.integers(1, 64))})
    rest = [i for i in range(n) if i not in ends]
    for a in range(0, len(rest), d1 - 2):          # every other position erased once, with one error elsewhere
        erased = rest[a:a + d1 - 2]
        free = [w for w in range(n // per) if per * w not in erased]
        add("pos_era", erased, {per * int(rng.choice(free)) + int(rng.integers(0, per)): int(rng.integers(1, 64))})
    add("full", [], {i: int(rng.integers(1, 64)) for i in range(t)})
    add("full", [], {n - 1 - i: int(rng.integers(1, 64)) for i in range(t)})          # all in the parity part: t <= n - k
    for e, v in beyond_pairs(kind):
        drawn("beyond", e, v)
    return units


def dense_rs_dibits(nac=0x293, seed=73, series=SERIES):
    """-> (dibits, plan).  1000 dibits for the loop to settle, the units of the series back to back, a tail of 888.  plan: a
    list of dict(start, kind, octets, what, e, v, erased, errors, wrong, n_diff) -- what: 'inside', every (|E|, v) inside the
    bound, the erased symbols wrong; 'right', erased symbols that carry the sent data; 'pos_err', two errors at j and
    j + n / 2; 'pos_era', erasures that cover every position, symbols 0 and n - 1 in one unit with an error next to each;
    'full', t errors at the word's first and at its last t symbols; 'beyond', beyond_pairs -- n_diff: the symbols, as the inner
    decoders read them, that differ from the sent ones"""
    rng = np.random.default_rng(seed)
    plan, frames = [], []
    for kind in series:
        wk = E.WORDS_KIND[kind]
        for u in _series_units(kind, rng):
            octets = bytes(rng.integers(0, 256, E.N_OCTETS[kind]).astype(np.uint8))
            clean = E.unit_words(kind, octets)
            words = E.with_erasures_and_errors_at(kind, clean, u["erased"], u["errors"], rng, u["wrong"])
            n_diff = sum(a != b for a, b in zip(R.word_symbols(wk, clean), R.word_symbols(wk, words)))
            plan.append(dict(u, kind=kind, octets=octets, n_diff=n_diff))
            frames.append(E.unit_frame(nac, kind, octets, rng, words=words, lsd=bytes([u["e"], u["v"], 0x5A, 0xC3])))
    at = 1000
    for p, f in zip(plan, frames):
        p["start"] = at
        at += len(f)
    d = np.concatenate([R.settle_dibits()] + frames + [rng.integers(0, 4, 888)]).astype(np.uint8)
    return d, plan


def check_rs_census(recs, plain, plan, series=SERIES):
    """the dense stream's guarantees, on the restatement's records with ES | ERASURES (recs) and with ES alone (plain): every
    planted frame is there, at k = start + 23, and nothing else; every unit that is not 'beyond' comes back with rs_bad = 0,
    the sent octets, n_bad as planted and n_rs = n_diff, the symbols that differ from the sent ones -- e + v where the erased
    symbols are wrong (a TLC: e / 2 + v .. e + v, an erased word has at least one wrong symbol of two), v where they are
    right; about the 'beyond' units it claims nothing but the frame: the restatement decides.  Every class occurs in every
    series: every pair inside the bound, three 'right' pairs, every position as an error's and as an erasure's, the values 1
    and 63, both ends at full weight, every pair of beyond_pairs"""
    f, g = native.p25lc_fields(recs), native.p25lc_fields(plain)
    assert len(recs) == len(plain) == len(plan), (len(recs), len(plain), len(plan))
    by_k = {int(k): i for i, k in enumerate(recs["k"])}
    assert len(by_k) == len(plan)
    seen = {kind: {c: [] for c in CLASSES} for kind in series}
    for p in plan:
        assert p["start"] + 23 in by_k, p                        # no planted frame is missing
        i = by_k[p["start"] + 23]
        kind, per = p["kind"], _per(p["kind"])
        assert int(plain["k"][i]) == p["start"] + 23 and f["kind"][i] == g["kind"][i] == kind and f["duid"][i] == E.DUID_OF[kind], p
        assert f["n_bad"][i] == p["e"] // per and (kind == TLC or g["n_bad"][i] == f["n_bad"][i]), p
        if kind in (LDU1, LDU2):
            assert bytes(recs["lsd"][i]) == bytes([p["e"], p["v"], 0x5A, 0xC3]), p
        seen[kind][p["what"]].append(p)
        if p["what"] == "beyond":
            continue
        pad = 16 - len(p["octets"])
        assert f["rs_bad"][i] == 0 and bytes(recs["payload"][i]) == p["octets"] + bytes(pad), p
        n_rs = int(f["n_rs"][i])
        assert n_rs == p["n_diff"], (p, n_rs)
        if not p["wrong"]:
            assert n_rs == p["v"], (p, n_rs)
        elif kind == TLC:
            assert p["e"] // 2 + p["v"] <= n_rs <= p["e"] + p["v"], (p, n_rs)
        else:
            assert n_rs == p["e"] + p["v"], (p, n_rs)
    for kind in series:
        n, k = E.RS_NK[kind]
        t, s = (n - k) // 2, seen[kind]
        pairs = lambda c: sorted((p["e"], p["v"]) for p in s[c])
        assert pairs("inside") == sorted(inside_pairs(kind)) and pairs("beyond") == sorted(beyond_pairs(kind)), kind
        assert pairs("right") == sorted(right_pairs(kind)) and not any(p["wrong"] for p in s["right"]), kind
        at = sorted(i for p in s["pos_err"] for i in p["errors"])
        assert at == list(range(n)) and all(sorted(p["errors"]) == [j, j + n // 2] for j, p in enumerate(s["pos_err"])), kind
        assert {1, 63} <= {x for p in s["pos_err"] for x in p["errors"].values()}, kind
        assert sorted(i for p in s["pos_era"] for i in p["erased"]) == list(range(n)), kind
        ends = s["pos_era"][0]
        assert {0, n - 1} <= set(ends["erased"]) and sorted(ends["errors"]) == [_per(kind), n - 1 - _per(kind)], kind
        assert [sorted(p["errors"]) for p in s["full"]] == [list(range(t)), list(range(n - t, n))], kind
    n_inside = sum(len(inside_pairs(kind)) for kind in series)
    assert series != SERIES or n_inside == 183


# ---- the NID
NID_WEIGHTS = tuple(range(2, 12))
BEYOND_WEIGHTS = (12, 13)
DATA_UNITS = ("tsdu", "hdu", "ldu1")


def _nid_patterns(rng):
    """-> list of dict(what, places): every single bit, the 64th bit alone, per weight 2 .. 11 twelve random patterns and a
    burst at either end, per weight 12 and 13 ten random patterns and two that lie toward another code word"""
    items = [dict(what="single", places=[i]) for i in range(63)] + [dict(what="bit64", places=[], bit64=1)]
    for w in NID_WEIGHTS:
        for _ in range(12):
            items.append(dict(what="random", places=sorted(int(p) for p in rng.choice(63, w, replace=False))))
        items.append(dict(what="top", places=list(range(w))))
        items.append(dict(what="bottom", places=list(range(63 - w, 63))))
    for w in BEYOND_WEIGHTS:
        for _ in range(10):
            items.append(dict(what="beyond", places=sorted(int(p) for p in rng.choice(63, w, replace=False))))
        for _ in range(2):
            items.append(dict(what="toward", places=N.toward_another_word(rng, w)[0]))
    return items


def dense_nid_dibits(nac=0x293, seed=79):
    """-> (dibits, plan), one stream for both stages.  1000 dibits to settle, then back to back TDUs (72 dibits, DUID 3: a
    frame record from either stage) whose NIDs carry _nid_patterns, every fifth with the 64th bit flipped as well; among them
    two TSDUs of three valid blocks, two HDUs and two LDU1s whose DUID is broken by one and by three bits, so that the decoded
    DUID is what a stage acts on; a tail of 888.  plan: list of dict(start, what, unit, places, bit64, weight, fix: the nid_fix
    the rule gives, sent_duid, read_duid, read_nac, decoded_duid, decoded_nac, octets)"""
    rng = np.random.default_rng(seed)
    items = _nid_patterns(rng)
    for n, it in enumerate(items):
        it.setdefault("bit64", int(n % 5 == 4))
        it["unit"] = "tdu"
    for unit in DATA_UNITS:
        for broken in (1, 3):
            places = sorted(12 + int(p) for p in rng.choice(4, broken, replace=False))
            items.insert(int(rng.integers(1, len(items))), dict(what="broken duid", unit=unit, places=places, bit64=0))
    frames, at = [], 1000
    for it in items:
        unit = it["unit"]
        sent_duid = {"tdu": 3, "tsdu": 7, "hdu": 0, "ldu1": 5}[unit]
        if unit == "tdu":
            f = R.frame(nac, 3, 72, rng)
        elif unit == "tsdu":
            f = T.frame(nac, 7, [T.tsbk_octets(rng) for _ in range(3)], rng)
        else:
            kind = HDU if unit == "hdu" else LDU1
            it["octets"] = bytes(rng.integers(0, 256, E.N_OCTETS[kind]).astype(np.uint8))
            f = E.unit_frame(nac, kind, it["octets"], rng, lsd=bytes([1, 0x5A, 0xC3, 0x0F]))
        r63 = N.flip(N.nid(nac, sent_duid), it["places"])
        got, fix = N.decode(r63)
        it.update(start=at, nac=nac, weight=len(it["places"]), fix=fix, sent_duid=sent_duid, read_duid=r63 >> 47 & 15, read_nac=r63 >> 51,
                  decoded_duid=got >> 47 & 15, decoded_nac=got >> 51)
        frames.append(N.set_nid(f, r63 << 1 | it["bit64"]))
        at += len(f)
    d = np.concatenate([R.settle_dibits()] + frames + [rng.integers(0, 4, 888)]).astype(np.uint8)
    return d, items


def nid_counters(plan):
    """rcf_nid_state_t of a stage that decided every planted frame and nothing else"""
    fixes = [p["fix"] for p in plan]
    return dict(n_decoded=len(fixes), n_fixed=sum(0 < x < N.BAD for x in fixes), n_bits=sum(x for x in fixes if x < N.BAD), n_bad=fixes.count(N.BAD))


def check_nid_census(stage, recs, raw, plan, nst):
    """the dense NID stream's guarantees for stage 'tsbk' or 'voice', on the restatement's records with the option (recs), without
    (raw) and its NID counters (nst): every planted frame is there and nothing else; every pattern of weight <= 11 gives
    nid_fix = its weight, whatever the 64th bit, and the sent nac and duid; the single-bit set is complete, the 64th bit alone
    gives 0; per weight 2 .. 11 twelve random patterns and a burst at either end; weights 12 and 13 give what the rule says,
    15 with the fields as read and a word toward another code word both among them; the counters are the sums over the
    frames' records; the stage's own data units with a broken duid decode with the option and are bare records without"""
    n = native.nid_fields(recs)
    f = native.tsbk_fields(recs) if stage == "tsbk" else native.p25lc_fields(recs)
    g = native.tsbk_fields(raw) if stage == "tsbk" else native.p25lc_fields(raw)
    bare = (lambda x, i: x["b"][i] == 3) if stage == "tsbk" else (lambda x, i: x["kind"][i] == 3)
    first, first_raw = {}, {}
    for i, kk in enumerate(recs["k"]):
        first.setdefault(int(kk), i)
    for i, kk in enumerate(raw["k"]):
        first_raw.setdefault(int(kk), i)
    assert len(first) == len(first_raw) == len(plan), (len(first), len(first_raw), len(plan))
    assert np.all(n["nid_decoded"] == 1) and not np.any(native.nid_fields(raw)["nid_decoded"])
    seen = {}
    for p in plan:
        assert p["start"] + 23 in first and p["start"] + 23 in first_raw, p
        i, j = first[p["start"] + 23], first_raw[p["start"] + 23]
        w, what = p["weight"], p["what"]
        assert int(n["nid_fix"][i]) == p["fix"], p
        assert (int(f["duid"][i]), int(f["nac"][i])) == (p["decoded_duid"], p["decoded_nac"]), p
        assert (int(g["duid"][j]), int(g["nac"][j])) == (p["read_duid"], p["read_nac"]), p
        seen.setdefault((what, w), []).append(p)
        if w <= N.T_MAX:
            assert p["fix"] == w and (p["decoded_duid"], p["decoded_nac"]) == (p["sent_duid"], p["nac"]), p
        elif p["fix"] == N.BAD:
            assert (p["decoded_duid"], p["decoded_nac"]) == (p["read_duid"], p["read_nac"]), p
        else:
            assert what == "toward" and p["fix"] == 23 - w, p
        if what == "broken duid":
            assert p["read_duid"] != p["sent_duid"] and w in (1, 3), p
            if stage == "tsbk" and p["unit"] == "tsdu":
                rows = np.flatnonzero(recs["k"] == p["start"] + 23)
                assert f["b"][rows].tolist() == [0, 1, 2] and not np.any(f["crc_bad"][rows]) and bare(g, j), p
            if stage == "voice" and p["unit"] != "tsdu":
                assert int(f["kind"][i]) == (HDU if p["unit"] == "hdu" else LDU1) and not f["rs_bad"][i] and bare(g, j), p
                assert bytes(recs["payload"][i])[:len(p["octets"])] == p["octets"], p
    assert sorted(p["places"][0] for p in seen[("single", 1)]) == list(range(63))
    assert [(p["bit64"], p["fix"]) for p in seen[("bit64", 0)]] == [(1, 0)]
    for w in NID_WEIGHTS:
        assert len(seen[("random", w)]) == 12 and len(seen[("top", w)]) == len(seen[("bottom", w)]) == 1, w
        assert seen[("top", w)][0]["places"][0] == 0 and seen[("bottom", w)][0]["places"][-1] == 62
    for w in BEYOND_WEIGHTS:
        assert len(seen[("beyond", w)]) == 10 and len(seen[("toward", w)]) == 2, w
        assert N.BAD in {p["fix"] for p in seen[("beyond", w)]}
    assert {(p["unit"], p["weight"]) for ps in seen.values() for p in ps if p["what"] == "broken duid"} == {(u, b) for u in DATA_UNITS for b in (1, 3)}
    flipped = [p for p in plan if p["bit64"] and p["weight"]]
    assert len(flipped) >= len(plan) // 6 and {p["weight"] for p in flipped} >= set(range(1, 12))
    assert nst == nid_counters(plan), (nst, nid_counters(plan))
    fix_of = [int(n["nid_fix"][i]) for i in first.values()]
    assert nst == dict(n_decoded=len(fix_of), n_fixed=sum(0 < x < N.BAD for x in fix_of), n_bits=sum(x for x in fix_of if x < N.BAD), n_bad=fix_of.count(N.BAD))
