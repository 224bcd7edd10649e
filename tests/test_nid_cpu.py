"""The NID option of the two P25 stages (RCF_NID_BCH: BCH(63,16,23) decoded before the DUID is acted on) without a GPU: the
code itself -- generator, minimum weight --, the restatement (tests/nid_ref.py, exhaustive search) against what the
reference's rs64.Codec(23) returned for the words of tests/golden/p25_nid.npz (made by tests/golden/make_nid_goldens.py, which
runs the reference), the kernel's arithmetic header compiled for the host (tests/native/nid_core_check.cpp, once more under
AddressSanitizer and UBSan, as programs of their own) against the restatement, and the binding's new names."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nid_ref as N
import p25es_ref as E
import p25lc_ref as R
import slicer_ref as S
import tsbk_ref as T
from rcf import native, p25

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOFT = np.array([1.0, 3.0, -1.0, -3.0], np.float32)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "p25_nid.npz"))


def slicer_streams(dibits, max_errors=4):
    r = S.run(SOFT[np.asarray(dibits)], S.FSK4, sync_word=p25.FRAME_SYNC, sync_bits=48, max_errors=max_errors)
    return r["words"], r["k"], r["dist"]


# ------------------------------------------------------------------------------------------------ the code
def _polymul2(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return r


def test_generator_is_the_lcm_of_the_minimal_polynomials_and_the_minimum_weight_is_23():
    exp = [1]
    for _ in range(62):
        v = exp[-1] << 1
        exp.append(v ^ 0x43 if v & 0x40 else v)
    log = {v: i for i, v in enumerate(exp)}
    gmul = lambda a, b: 0 if not a or not b else exp[(log[a] + log[b]) % 63]
    gen, done = 1, set()
    for m in range(1, 23):
        if m in done:
            continue
        coset, e = [], m
        while e not in coset:
            coset.append(e)
            e = 2 * e % 63
        done |= set(coset)
        poly = [1]                                     # prod (x + alpha^e) over the coset, coefficients in GF(64), lowest first
        for e in coset:
            poly = [(poly[i - 1] if i else 0) ^ (gmul(poly[i], exp[e]) if i < len(poly) else 0) for i in range(len(poly) + 1)]
        assert set(poly) <= {0, 1}                     # a minimal polynomial is binary
        gen = _polymul2(gen, sum(c << i for i, c in enumerate(poly)))
    assert gen == N.GENERATOR == p25.NID_GENERATOR == 0o6331141367235453 and gen.bit_length() == 48
    assert len(set(N.WORDS.tolist())) == 65536 and int(N.WEIGHTS[1:].min()) == 23 and int(np.sum(N.WEIGHTS == 23)) == 1890
    assert all(N.encode(int(w) >> 47) == int(w) for w in N.WORDS[::97])
    assert p25.nid_encode(0x293, 7) == N.nid(0x293, 7)


# ------------------------------------------------------------------------------------------------ the reference's results
def test_restatement_equals_the_reference_on_every_golden_word(golden):
    g = golden
    assert len(g["nid_w"]) >= 18 * 200 + 63 + 150
    per = {}
    inside = differs = answered = 0
    for w, sent, flips, cls, other, ref in zip(*[g[n].tolist() for n in ("nid_w", "nid_sent", "nid_flips", "nid_class", "nid_other", "nid_ref")]):
        word, fix = N.decode(w)
        per[(cls, flips)] = per.get((cls, flips), 0) + 1
        assert ref != -2                               # the reference never answered with symbols other than 0 / 1
        if cls in (0, 1, 3) and flips <= 11:           # inside the bound: the sent word, from both
            inside += 1
            assert (word, fix) == (N.encode(sent), flips) and ref == sent, (cls, flips)
        else:
            rule = word >> 47 if fix != N.BAD else -1
            answered += ref != -1
            differs += ref != rule
            if cls == 2:
                assert (word, fix) == (N.encode(sent) ^ other, 11)
            if cls == 4:
                assert (word, fix) == (N.encode(sent) ^ other, 10)
        h = p25.nid_decode(w)
        assert (h["nac"] << 4 | h["duid"], h["nid_fix"]) == (word >> 47, fix)
    print("NID goldens: %d inside the bound; beyond it the reference answered %d times, %d of them not the rule's word" % (inside, answered, differs))
    assert differs == 0 and answered > 50 and g["counts"].tolist()[1] == 0 and g["counts"].tolist()[5] == 0
    assert all(per[(0, w)] >= 200 for w in list(range(15)) + [16, 20, 31]) and per[(1, 1)] == 63
    assert per[(2, 12)] == per[(3, 11)] == per[(4, 13)] == 50
    places = {w: set() for w in range(1, 32)}
    for w, sent, flips, cls in zip(g["nid_w"].tolist(), g["nid_sent"].tolist(), g["nid_flips"].tolist(), g["nid_class"].tolist()):
        if cls == 0 and flips:
            places[flips] |= set(N.support(w ^ N.encode(sent))) & {0, 62}
    assert all(places[w] == {0, 62} for w in list(range(1, 15)) + [16, 20, 31])


# ------------------------------------------------------------------------------------------------ the header on the host
@pytest.fixture(scope="module")
def check_programs():
    """nid_core.hpp and the wave form's walk compiled for the host, plain and with the sanitizers: stand-alone programs"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(HERE, "native", "nid_core_check.cpp")
    exes = []
    for name, extra in (("nid_core_check", ["-O2"]), ("nid_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(out, name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable"] + extra + [src, "-o", exe])
        exes.append(exe)
    return exes


def both(exes, args):
    outs = []
    for exe in exes:
        p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, (exe, p.stdout.decode()[-2000:])
        outs.append(p.stdout.decode())
    assert outs[0] == outs[1]
    return outs[0]


def test_header_decoder_equals_the_restatement_on_goldens_and_on_all_single_and_double_flips(check_programs, tmp_path, golden):
    word = N.nid(0x293, 7)
    flips = [N.flip(word, [a]) for a in range(63)] + [N.flip(word, [a, b]) for a in range(63) for b in range(a + 1, 63)]
    rng = np.random.default_rng(12)
    noise = [int(v) >> 1 for v in rng.integers(0, 1 << 63, 300, dtype=np.uint64)]
    words = golden["nid_w"].tolist() + flips + noise
    path = str(tmp_path / "w.u64")
    np.array(words, "<u8").tofile(path)
    lines = both(check_programs, ["words", path]).strip().split("\n")
    assert len(lines) == len(words)
    n_bad = 0
    for ln, w in zip(lines, words):
        fix, c = (int(v) for v in ln.split())
        assert (c, fix) == N.decode(w), hex(w)
        n_bad += fix == N.BAD
    assert n_bad > 1000
    for ln in lines[len(golden["nid_w"]):len(golden["nid_w"]) + len(flips)]:
        assert int(ln.split()[1]) == word and int(ln.split()[0]) in (1, 2)


def through_header(exes, tmp_path, stage, words, k, dist, cuts, n_symbols, nid, correct=1, options=0, first_hit=0, word_cap=1 << 20, hit_cap=1 << 20):
    """the stand-alone programs over the streams, a launch after each cut (a symbol count) -> (records, counters, the NID's, launches)"""
    wp, hp = str(tmp_path / "words.u32"), str(tmp_path / "hits.u32")
    np.asarray(words, "<u4").tofile(wp)
    S.hit_items(k, dist).astype("<u4").tofile(hp)
    launches, args, before = [], [], 0
    for c in list(cuts) + [n_symbols]:
        launches.append((c // 16, int(np.count_nonzero(np.asarray(k) < c))))
        args += [c // 16, launches[-1][1], c, c - before]
        before = c
    lines = both(exes, ["stream", stage, wp, hp, correct, options, nid, first_hit, word_cap, hit_cap] + args).strip().split("\n")
    v = lines[0].split()
    names = ("n_records", "n_frames", "n_blocks", "n_crc_bad", "n_lost") if stage == "tsbk" else ("n_records", "n_frames", "n_decoded", "n_rs_bad", "n_lost")
    st = {n: int(x) for n, x in zip(names, v[:5])}
    nst = {n: int(x) for n, x in zip(("n_decoded", "n_fixed", "n_bits", "n_bad"), v[6:10])}
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1:]], dtype="<u4").reshape(-1, 8)
    return recs.view(native.TSBK_DTYPE if stage == "tsbk" else native.P25LC_DTYPE).reshape(-1), st, nst, launches


def restate(stage, words, k, dist, nid, **kw):
    if stage == "tsbk":
        return N.run_tsbk(words, k, dist, nid=nid, **kw)
    return N.run_voice(words, k, dist, nid=nid, options=E.ES | E.ERASURES, **kw)


@pytest.mark.parametrize("stage", ["tsbk", "voice"])
def test_designed_dibits_meet_their_census_and_header_equals_restatement_under_ragged_cuts(check_programs, tmp_path, stage):
    """the input of the GPU suite's designed carrier without a device: the generator alone meets the census, and header,
    restatement and kernel stand on one input; with nid = 0 the header gives tsbk_ref's and p25es_ref's records"""
    d, plan = N.designed_dibits(stage)
    words, k, dist = slicer_streams(d)
    assert (np.asarray(k) - 23).tolist() == [p["start"] for p in plan] and not np.any(dist)       # every planted frame, and nothing else
    recs, st, nst = restate(stage, words, k, dist, 1)
    raw, raw_st, raw_nst = restate(stage, words, k, dist, 0)
    N.check_census(stage, recs, raw, plan)
    fixes = [p["fix"] for p in plan]
    assert nst == dict(n_decoded=len(plan), n_fixed=sum(0 < f < 15 for f in fixes), n_bits=sum(f for f in fixes if f < 15), n_bad=fixes.count(15))
    assert raw_nst == dict(n_decoded=0, n_fixed=0, n_bits=0, n_bad=0) and nst["n_bad"] == 1 and st["n_frames"] == raw_st["n_frames"] == len(plan)
    plain = T.run(words, k, dist) if stage == "tsbk" else E.run(words, k, dist, options=E.ES | E.ERASURES)
    assert raw.tobytes() == plain[0].tobytes() and raw_st == plain[1]
    rng = np.random.default_rng(3)
    opt = 0 if stage == "tsbk" else E.ES | E.ERASURES
    for nid, want in ((1, (recs, st, nst)), (0, (raw, raw_st, raw_nst))):
        for cuts in ([], sorted(rng.choice(len(d), 40).tolist()), [5, 5, 5, 6, 1500, 1500, 1501] + list(range(1600, len(d), 211))):
            got, got_st, got_nst, launches = through_header(check_programs, tmp_path, stage, words, k, dist, cuts, len(d), nid, options=opt)
            assert got.tobytes() == want[0].tobytes() and (got_st, got_nst) == want[1:], (nid, cuts[:6])
            again = restate(stage, words, k, dist, nid, launches=launches)
            assert again[0].tobytes() == want[0].tobytes() and again[1:] == want[1:]


@pytest.mark.parametrize("stage", ["tsbk", "voice"])
def test_noise_hits_small_rings_and_a_late_attach_through_the_header(check_programs, tmp_path, stage):
    """random dibits under the loosened search: NIDs that are mostly beyond every code word, frames that cut each other, a
    word ring of 64, a hit ring of 16 and a stage attached at hit 2"""
    d = np.random.default_rng(9).integers(0, 4, 30000).astype(np.uint8)
    words, k, dist = slicer_streams(d, max_errors=18)
    assert len(k) > 100
    opt = 0 if stage == "tsbk" else E.ES | E.ERASURES
    want = restate(stage, words, k, dist, 1)
    got, st, nst, _ = through_header(check_programs, tmp_path, stage, words, k, dist, [], len(d), 1, options=opt)
    assert got.tobytes() == want[0].tobytes() and (st, nst) == want[1:] and nst["n_bad"] > 50
    cuts = list(range(2000, len(d), 96))
    got, st, nst, launches = through_header(check_programs, tmp_path, stage, words, k, dist, cuts, len(d), 1, options=opt, first_hit=2, word_cap=64, hit_cap=16)
    want = restate(stage, words, k, dist, 1, first_hit=2, launches=launches, word_cap=64, hit_cap=16)
    assert got.tobytes() == want[0].tobytes() and (st, nst) == want[1:] and st["n_lost"] >= 1


# ------------------------------------------------------------------------------------------------ names, constants, fields
def test_binding_names_constants_and_fields():
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RCF_\w+)\s+(-?\d+)", hdr)}
    assert (defs["RCF_NID_RAW"], defs["RCF_NID_BCH"]) == (0, 1)
    for name in ("rcf_chan_tsbk_ex", "rcf_chan_p25lc_ex", "rcf_chan_nid_state"):
        assert name in native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr)
    assert ctypes.sizeof(native.NidState) == 32 and [n for n, _ in native.NidState._fields_] == ["n_decoded", "n_fixed", "n_bits", "n_bad"]
    t = np.zeros(1, native.TSBK_DTYPE)
    t["frame_dibits"] = 360 | 11 << 16 | 1 << 20
    assert {n: int(v[0]) for n, v in native.nid_fields(t).items()} == dict(nid_fix=11, nid_decoded=1, frame_dibits=360)
    fr = p25.tsdu_frames(t)[0]
    assert (fr["frame_dibits"], fr["nid_fix"], fr["nid_decoded"]) == (360, 11, 1)
    v = np.zeros(1, native.P25LC_DTYPE)
    v["flags"] = 1 << 9 | 3
    v["tail"] = 864 | 15 << 28
    assert {n: int(x[0]) for n, x in native.nid_fields(v).items()} == dict(nid_fix=15, nid_decoded=1, frame_dibits=864)
    u = p25.voice_units(v)[0]
    assert (u["frame_dibits"], u["nid_fix"], u["nid_decoded"], u["decoded"]) == (864, 15, 1, False)
    import inspect
    assert inspect.signature(native.Frontend.chan_tsbk).parameters["nid"].default is False
    assert inspect.signature(native.Frontend.chan_p25lc_ex).parameters["nid"].default is False
    for fn in (p25.c4fm_demod, p25.cqpsk_demod):
        assert inspect.signature(fn).parameters["nid"].default is False
    assert p25.nid_decode([0] * 63) == dict(nac=0, duid=0, nid_fix=0) and p25.nid_decode([1] + [0] * 63)["nid_fix"] == 1
