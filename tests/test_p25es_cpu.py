"""The options of the P25 voice-channel stage (rcf_chan_p25lc_opt: LDU2's encryption sync, inner words given up as
Reed-Solomon erasures) without a GPU: the restatement (tests/p25es_ref.py) against what the reference's rs64.Codec(9) / (13) /
(17) with and without `erasures`, golay.py and p25_general's stubs returned for the cases of tests/golden/p25_es.npz (made by
tests/golden/make_p25es_goldens.py, which runs the reference); the kernel's arithmetic header compiled for the host
(tests/native/p25es_core_check.cpp, once more under AddressSanitizer and UBSan, as programs of their own) against the
restatement; with options 0 the restatement against p25lc_ref's; and the binding's new names."""
import os
import re
import subprocess

import numpy as np
import pytest

import p25es_ref as E
import p25lc_ref as R
import slicer_ref as S
from rcf import native, p25

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOFT = np.array([1.0, 3.0, -1.0, -3.0], np.float32)
CODES = (("9", 24, 16), ("13", 24, 12), ("17", 36, 20))
OPTION_SETS = ((1, 0), (1, E.ES), (1, E.ES | E.ERASURES), (1, E.ERASURES), (0, E.ES))         # (correct, options)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "p25_es.npz"))


def slicer_streams(dibits, max_errors=4):
    r = S.run(SOFT[np.asarray(dibits)], S.FSK4, sync_word=p25.FRAME_SYNC, sync_bits=48, max_errors=max_errors)
    return r["words"], r["k"], r["dist"]


def rs_rows(g, name):
    return zip(*[g["rs%s_%s" % (name, f)].tolist() for f in ("w", "sent", "erased", "e", "v", "none", "data")])


# ------------------------------------------------------------------------------------------------ the reference's results
@pytest.mark.parametrize("name,n,k", CODES)
def test_reed_solomon_with_erasures_against_the_reference_on_every_golden(golden, name, n, k):
    """inside the bound the restatement returns the sent word, which is the reference's answer wherever it gave one; beyond
    it: where the reference answered with a word inside the rule's bound (|E| = d - 1 and an error outside) the restatement
    gives that word; the reference's other answers change more symbols than the rule allows (|E| = d - 2 and one error, a
    word the bound does not make unique) and the restatement gives rs_bad like everywhere else beyond"""
    d = int(name)
    t = (d - 1) // 2
    pairs = {(e, v) for total in range(d - 2, d + 2) for v in range(total // 2 + 1) for e in (total - 2 * v,)}
    assert {(e, v) for _, _, _, e, v, _, _ in rs_rows(golden, name)} == pairs
    inside = none_inside = answered_beyond = beyond_bound = other = 0
    edges = {(0, t): 0, (d - 1, 0): 0}
    for w, sent, mask, e, v, none, data in rs_rows(golden, name):
        erased = [i for i in range(n) if mask[i]]
        assert len(erased) == e
        out, rs_bad, n_rs = E.rs_decode(w, n, k, erased)
        if (e, v) in edges and {0, n - 1} <= {i for i in range(n) if w[i] != sent[i]}:
            edges[(e, v)] += 1
        if e + 2 * v <= d - 1:
            inside += 1
            none_inside += none
            assert (out, rs_bad) == (sent, 0) and n_rs == sum(a != b for a, b in zip(w, sent)), (e, v)
            assert none or data == sent[:k]
        elif none and rs_bad:
            assert (out, n_rs) == (w, 0), (e, v)
        elif none:                                     # another code word lies inside the bound of what was received
            other += 1
            assert not any(R.rs_syndromes(out, n, k)) and e + 2 * sum(out[i] != w[i] for i in range(n) if not mask[i]) <= d - 1, (e, v)
            assert n_rs == sum(a != b for a, b in zip(out, w)) and out != sent
        else:
            answered_beyond += 1
            cw = R.rs_encode(data, n, k)
            changed_outside = sum(cw[i] != w[i] for i in range(n) if not mask[i])
            if e + 2 * changed_outside <= d - 1:
                assert (out, rs_bad) == (cw, 0), (e, v)
            else:
                beyond_bound += 1
                assert (e, v) == (d - 2, 1) and (out, rs_bad, n_rs) == (w, 1, 0), (e, v)
    print("RS d = %s: %d words inside the bound, the reference answered None on %d of them; beyond the bound it answered %d, %d "
          "of them beyond the rule; %d words beyond the bound lie inside another code word's" % (name, inside, none_inside, answered_beyond, beyond_bound, other))
    assert inside > 250 and none_inside > 0 and min(edges.values()) >= 16


def test_uncorrected_ldu2_gives_what_p25_generals_stubs_returned_for_every_golden_frame(golden):
    g = golden
    assert len(g["ldu2_frames"]) == 70 and set(g["ldu2_flips"].tolist()) == {0, 1, 2, 4, 8, 16}
    for by, nid, es, lsd in zip(g["ldu2_frames"], g["ldu2_nid"], g["ldu2_es"], g["ldu2_lsd"]):
        stream = np.concatenate([by, np.zeros(4 * ((R.DECIDE + 15) // 16) - len(by), np.uint8)])
        recs, st = E.run(stream, [23, 23 + 864], [0, 0], correct=0, options=E.ES)
        assert len(recs) == 1 and st == dict(n_records=1, n_frames=1, n_decoded=1, n_rs_bad=0, n_lost=0)
        u = p25.voice_units(recs)[0]
        if (int(nid) >> 48) & 15 != 0xA:               # (a flipped bit in the duid: no LDU2)
            continue
        assert (u["short"], u["decoded"], u["nac"], u["frame_dibits"]) == ("LDU2", True, int(nid) >> 52, 864)
        assert u["mi"] + bytes([u["algid"]]) + u["kid"].to_bytes(2, "big") == es.tobytes() and u["lsd"] == lsd.tobytes()
        assert bytes(recs["payload"][0])[12:] == bytes(4) and (u["rs_bad"], u["n_rs"], u["n_fixed"], u["n_bad"]) == (0, 0, 0, 0)
        plain, _ = E.run(stream, [23, 23 + 864], [0, 0], correct=0)
        assert plain.tobytes() == R.run(stream, [23, 23 + 864], [0, 0], correct=0)[0].tobytes() and not p25.voice_units(plain)[0]["decoded"]


def test_the_24th_bit_rule_stands_on_the_parity_golay_py_encodes(golden):
    g = golden
    n_bad = n_ref = 0
    for w, ref, bit in zip(g["golay_par_w"].tolist(), g["golay_par_ref"].tolist(), g["golay_par_bit"].tolist()):
        data, status, dist = E.golay24_detect(w)
        c, _ = R.golay23_nearest(w >> 1)
        if ref >= 0:
            n_ref += 1
            assert ref == c >> 11 and bit == bin(c).count("1") & 1
            assert (status == 2) == (dist == 3 and bit != w & 1)
        assert (data, status) == ((w >> 12, 2) if status == 2 else R.golay24_decode(w)[:2])
        n_bad += status == 2
    assert len(g["golay_par_w"]) == 3000 and n_ref > 1500 and n_bad > 1000


# ------------------------------------------------------------------------------------------------ the header on the host
@pytest.fixture(scope="module")
def check_programs():
    """p25lc_core.hpp's new functions compiled for the host, plain and with the sanitizers: stand-alone programs"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(HERE, "native", "p25es_core_check.cpp")
    exes = []
    for name, extra in (("p25es_core_check", ["-O2"]), ("p25es_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(out, name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable"] + extra + [src, "-o", exe])
        exes.append(exe)
    return exes


def both(exes, args):
    outs = []
    for exe in exes:
        p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert p.returncode == 0, (exe, p.stdout.decode()[-2000:])
        outs.append(p.stdout.decode())
    assert outs[0] == outs[1]
    return outs[0]


def through_header(exes, tmp_path, words, k, dist, cuts, n_symbols, correct=1, options=0, first_hit=0, word_cap=1 << 20, hit_cap=1 << 20):
    """the stand-alone programs over the streams, a launch after each cut (a symbol count) -> (records, counters, launches)"""
    wp, hp = str(tmp_path / "words.u32"), str(tmp_path / "hits.u32")
    np.asarray(words, "<u4").tofile(wp)
    S.hit_items(k, dist).astype("<u4").tofile(hp)
    launches, args, before = [], [], 0
    for c in list(cuts) + [n_symbols]:
        launches.append((c // 16, int(np.count_nonzero(np.asarray(k) < c))))
        args += [c // 16, launches[-1][1], c, c - before]
        before = c
    lines = both(exes, ["stream", wp, hp, correct, options, first_hit, word_cap, hit_cap] + args).strip().split("\n")
    names = lines[0].split()
    st = {"n_" + names[i]: int(names[i + 1]) for i in range(0, 10, 2)}
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1:]], dtype="<u4").reshape(-1, 8)
    return recs.view(native.P25LC_DTYPE).reshape(-1), st, launches


def test_header_decoders_equal_the_restatement_on_every_golden(check_programs, tmp_path, golden):
    g = golden
    path = str(tmp_path / "golay.u32")
    words = np.concatenate([g["golay_par_w"], np.random.default_rng(5).integers(0, 1 << 24, 3000).astype(np.uint32)]).astype("<u4")
    words.tofile(path)
    got = [tuple(int(v) for v in ln.split()) for ln in both(check_programs, ["golay", path]).strip().split("\n")]
    assert got == [E.golay24_detect(int(w))[:2] for w in words]
    for name, n, k in CODES:
        path = str(tmp_path / "rs.u8")
        np.concatenate([g["rs%s_w" % name], g["rs%s_erased" % name]], axis=1).astype(np.uint8).tofile(path)
        for erasures in (1, 0):
            lines = both(check_programs, ["rs", n, (n - k) // 2, path, erasures]).strip().split("\n")
            assert len(lines) == len(g["rs%s_w" % name])
            for ln, w, mask in zip(lines, g["rs%s_w" % name].tolist(), g["rs%s_erased" % name].tolist()):
                v = [int(x) for x in ln.split()]
                out, rs_bad, n_rs = E.rs_decode(w, n, k, [i for i in range(n) if mask[i]] if erasures else [])
                assert (v[0], v[1], v[2:]) == (rs_bad, n_rs, out), (name, erasures)
            if not erasures:                           # ... which without erasures is p25lc_ref's decoder
                assert all(E.rs_decode(w, n, k) == R.rs_decode(w, n, k) for w in g["rs%s_w" % name].tolist())


def test_options_0_give_p25lc_refs_records_on_the_call_and_on_noise_hits():
    d, _, _ = R.call_dibits()
    words, k, dist = slicer_streams(d)
    lw, lk, ldist = slicer_streams(np.random.default_rng(9).integers(0, 4, 30000).astype(np.uint8), max_errors=18)
    assert len(lk) > 100
    for correct in (1, 0):
        for w, kk, dd in ((words, k, dist), (lw, lk, ldist)):
            want, want_st = R.run(w, kk, dd, correct=correct)
            got, st = E.run(w, kk, dd, correct=correct)
            assert got.tobytes() == want.tobytes() and st == want_st and len(got) > 7
    # and with ES only the LDU2s' records differ
    got, st = E.run(words, k, dist, options=E.ES)
    want, want_st = R.run(words, k, dist)
    ldu2 = native.p25lc_fields(want)["duid"] == 0xA
    assert ldu2.sum() == 3 and got[~ldu2].tobytes() == want[~ldu2].tobytes() and st["n_decoded"] == want_st["n_decoded"] + 3
    assert native.p25lc_fields(got)["kind"][ldu2].tolist() == [4, 4, 4]


def test_the_es_call_through_the_header_ragged_cuts_rings_and_a_late_attach(check_programs, tmp_path):
    d, starts, shorts = E.call_dibits()
    words, k, dist = slicer_streams(d)
    rng = np.random.default_rng(4)
    c = E.CALL_ES
    for correct, options in OPTION_SETS:
        want, want_st = E.run(words, k, dist, correct=correct, options=options)
        units = p25.voice_units(want)
        assert [u["short"] for u in units] == shorts and [u["k"] - 23 for u in units] == starts
        for i, u in enumerate(units):
            if u["short"] == "LDU2":
                assert u["decoded"] == bool(options & E.ES)
                if u["decoded"] and (correct or i != 4):       # (the second LDU2 carries the planted errors)
                    assert (u["mi"], u["algid"], u["kid"], u["lsd"], u["rs_bad"]) == (c["mi"], c["algid"], c["kid"], c["lsd2"], 0)
        if correct and options & E.ES:
            assert [(u["n_rs"], u["n_fixed"]) for u in units if u["short"] == "LDU2"] == [(0, 0), (1, 3), (0, 0)]
        for cuts in ([], sorted(rng.choice(len(d), 60).tolist()), list(range(0, len(d), 7)), [5, 5, 5, 6, 1500, 1500, 1501]):
            got, st, launches = through_header(check_programs, tmp_path, words, k, dist, cuts, len(d), correct=correct, options=options)
            assert got.tobytes() == want.tobytes() and st == want_st, (options, cuts[:8])
            again, again_st = E.run(words, k, dist, correct=correct, options=options, launches=launches)
            assert again.tobytes() == want.tobytes() and again_st == want_st
    # a ring of 64 words, a hit ring of 16 and a stage attached at hit 2 with the loosened search, all options on
    cuts = [2000, 5200] + list(range(5296, len(d), 96))
    got, st, launches = through_header(check_programs, tmp_path, words, k, dist, cuts, len(d), options=3, word_cap=64)
    want, want_st = E.run(words, k, dist, options=3, launches=launches, word_cap=64)
    assert got.tobytes() == want.tobytes() and st == want_st and st["n_lost"] >= 1 and st["n_records"] > 0
    lw, lk, ldist = slicer_streams(d, max_errors=18)
    assert len(lk) > 40
    got, st, launches = through_header(check_programs, tmp_path, lw, lk, ldist, [900], len(d), options=3, first_hit=2, hit_cap=16)
    want, want_st = E.run(lw, lk, ldist, options=3, first_hit=2, launches=launches, hit_cap=16)
    assert got.tobytes() == want.tobytes() and st == want_st and st["n_lost"] >= 1


def test_designed_dibits_guarantee_their_census_and_header_equals_restatement_on_them(check_programs, tmp_path):
    """the input of the GPU suite's designed carrier (E.designed_dibits) without a device: the generator alone meets the
    census, and header, restatement and kernel stand on one input"""
    d, plan = E.designed_dibits()
    assert len(plan) == 25 and 15000 < len(d) < 20000
    words, k, dist = slicer_streams(d)
    assert (np.asarray(k) - 23).tolist() == [p["start"] for p in plan] and not np.any(dist)     # every planted frame, and nothing else
    recs, st = E.run(words, k, dist, options=E.ES | E.ERASURES)
    plain, plain_st = E.run(words, k, dist, options=E.ES)
    E.check_census(recs, plain, plan)
    assert st == dict(n_records=25, n_frames=25, n_decoded=25, n_rs_bad=9, n_lost=0) and plain_st["n_rs_bad"] > 9
    for correct, options in OPTION_SETS:
        want, want_st = E.run(words, k, dist, correct=correct, options=options)
        for cuts in ([], list(range(0, len(d), 997))):
            got, got_st, _ = through_header(check_programs, tmp_path, words, k, dist, cuts, len(d), correct=correct, options=options)
            assert got.tobytes() == want.tobytes() and got_st == want_st, (options, cuts[:4])
    # the parent's designed stream with its own census, under the erasures option: header == restatement there too
    d, plan = R.designed_dibits()
    words, k, dist = slicer_streams(d)
    want, want_st = E.run(words, k, dist, options=E.ES | E.ERASURES)
    got, got_st, _ = through_header(check_programs, tmp_path, words, k, dist, [], len(d), options=E.ES | E.ERASURES)
    assert got.tobytes() == want.tobytes() and got_st == want_st and want_st["n_decoded"] == 29


# ------------------------------------------------------------------------------------------------ names, constants, fields
def test_binding_names_constants_and_fields():
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RCF_\w+)\s+(-?\d+)", hdr)}
    assert (native.P25LC_ES, native.P25LC_ERASURES) == (defs["RCF_P25LC_ES"], defs["RCF_P25LC_ERASURES"]) == (1, 2)
    assert "rcf_chan_p25lc_opt" in native.SYMBOLS and re.search(r"\brcf_chan_p25lc_opt\s*\(", hdr)
    f = native.p25lc_fields(np.array([(0xABCA_0000 | 1 << 8 | 0 << 4 | 8, 0, [0] * 16, [0] * 4, 864 | 16 << 22)], native.P25LC_DTYPE))
    assert {n: int(v[0]) for n, v in f.items()} == dict(kind=4, rs_bad=0, n_rs=16, dist=0, duid=0xA, nac=0xABC, frame_dibits=864, n_fixed=0, n_bad=16)
    recs = np.zeros(1, native.P25LC_DTYPE)
    recs["flags"] = 8 | 0xA << 16
    recs["payload"][0, :12] = list(range(1, 13))
    recs["lsd"][0] = [9, 8, 7, 6]
    u = p25.voice_units(recs)[0]
    assert (u["short"], u["decoded"], u["mi"], u["algid"], u["kid"], u["lsd"]) == ("LDU2", True, bytes(range(1, 10)), 10, 0x0B0C, bytes([9, 8, 7, 6]))
    import inspect
    sig = inspect.signature(native.Frontend.chan_p25lc)
    assert [(n, p.default) for n, p in sig.parameters.items()][1:] == [("cid", inspect.Parameter.empty), ("capacity", 0), ("correct", True), ("on", True),
                                                                       ("es", False), ("erasures", False)]
    for fn in (p25.c4fm_demod, p25.cqpsk_demod):
        assert [inspect.signature(fn).parameters[n].default for n in ("es", "erasures")] == [False, False]
