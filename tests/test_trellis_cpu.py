"""The trellis option of the P25 trunking stage (RCF_TRELLIS_VITERBI: the least-cost path that ends in state 0 instead of the
reference's word-by-word walk) without a GPU: the restatement's greedy form against what the reference's own
trellis_1_2_decode and crc16 returned for the blocks of tests/golden/p25_trellis.npz (made by
tests/golden/make_trellis_goldens.py, which runs the reference); the rule's sequential form against brute force over all
paths; the free distance; what the rule recovers; the kernel's arithmetic header compiled for the host
(tests/native/trellis_core_check.cpp, once more under AddressSanitizer and UBSan, as programs of their own) against the
restatement; and the binding's new names."""
import ctypes
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import slicer_ref as S
import trellis_ref as V
import tsbk_ref as T
from rcf import native, p25

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOFT = np.array([1.0, 3.0, -1.0, -3.0], np.float32)


@pytest.fixture(scope="module")
def golden():
    """-> list of dict(sent: 12 octets, block: the 98 received dibits, ref: the reference's 12 octets, crc, flips, cls), and
    per block the restatement's answer under the new rule (computed once, shared)"""
    g = np.load(os.path.join(HERE, "golden", "p25_trellis.npz"))
    rows = []
    for sent, rec, ref, crc, flips, cls in zip(g["sent"], g["received"], g["ref"], g["crc"].tolist(), g["flips"].tolist(), g["cls"].tolist()):
        bits = np.unpackbits(rec)[:196]
        block = (2 * bits[0::2] + bits[1::2]).tolist()
        rows.append(dict(sent=bytes(sent), block=block, ref=bytes(ref), crc=crc, flips=flips, cls=cls, words=V.code_words(block)))
    for r in rows:
        states, r["cost"], r["n_inexact"] = V.sequential(r["words"])
        r["states"] = states
        r["octets"] = V.octets_of([v for s in states[:48] for v in (s >> 1, s & 1)])
    return rows


def slicer_streams(dibits, max_errors=4):
    r = S.run(SOFT[np.asarray(dibits)], S.FSK4, sync_word=p25.FRAME_SYNC, sync_bits=48, max_errors=max_errors)
    return r["words"], r["k"], r["dist"]


# ------------------------------------------------------------------------------------------------ the baseline
def test_greedy_restatement_equals_the_reference_on_every_golden_block(golden):
    per = {}
    for r in golden:
        bits, bad, _ = T.decode_block(r["block"])
        assert V.octets_of(bits) == r["ref"] and bad == r["crc"], (r["cls"], r["flips"])
        states, cost, inexact = p25.trellis_decode(r["words"], viterbi=False)
        assert V.octets_of([v for s in states for v in (s >> 1, s & 1)]) == r["ref"] and inexact == V.greedy(r["words"])[1]
        per[(r["cls"], r["flips"])] = per.get((r["cls"], r["flips"]), 0) + 1
    assert per == {(0, 0): 12, (1, 1): 392, (2, 2): 2000, (3, 3): 500, (3, 4): 500, (3, 6): 500, (3, 8): 500, (4, 4): 100, (4, 8): 100}, per


# ------------------------------------------------------------------------------------------------ the rule
def test_sequential_form_equals_brute_force_on_every_sequence_of_three_words_and_flush():
    n = 0
    for c in itertools.product(range(16), repeat=4):
        assert V.sequential(list(c)) == V.brute(list(c)), c
        n += 1
    assert n == 16 ** 4


@pytest.mark.parametrize("n", [5, 6, 8])
def test_sequential_form_equals_brute_force_on_random_sequences(n):
    rng = np.random.default_rng(100 + n)
    for i in range(300):
        if i % 2:                                    # a valid path with a few flips: where ties between paths are met
            s, c = 0, []
            for d in rng.integers(0, 4, n).tolist() + [0]:
                c.append(V.W[s][d]); s = d
            for t in rng.integers(0, n + 1, int(rng.integers(0, 4))).tolist():
                c[t] ^= 1 << int(rng.integers(0, 4))
        else:
            c = rng.integers(0, 16, n + 1).tolist()
        assert V.sequential(c) == V.brute(c), c


def test_free_distance_is_at_least_five():
    d = V.free_distance()
    print("free distance of the trellis: %d" % d)
    assert d >= 5 and V.free_distance(depth=20) == d


def test_every_single_and_double_flip_of_three_blocks_decodes_to_the_sent_octets():
    """2 = floor((d_free - 1) / 2): the one pass condition that is a guarantee"""
    rng = np.random.default_rng(8)
    for _ in range(3):
        octets = T.tsbk_octets(rng)
        block = T.encode_block(octets)
        sent = np.array([2 * b0 + b1 for b0, b1 in np.unpackbits(np.frombuffer(octets, np.uint8)).reshape(48, 2).tolist()] + [0])
        assert not T.decode_block(block)[1]                                          # the sent octets' CRC is good
        all_places = [[a] for a in range(196)] + [[a, b] for a in range(196) for b in range(a + 1, 196)]
        words = np.array([V.code_words(V.flipped(block, places)) for places in all_places], np.uint8)
        states, cost, inexact = V.sequential_many(words)
        assert len(words) == 196 + 19110 and np.all(states == sent[None, :]) and cost.tolist() == [len(p) for p in all_places]
        for i in range(0, len(words), 41):           # the numpy form is the sequential form
            assert (states[i].tolist(), int(cost[i]), int(inexact[i])) == V.sequential(words[i].tolist())


def test_new_rule_recovers_every_golden_block_within_two_flips_where_the_reference_fails_on_some(golden):
    """fails without the feature: p25.trellis_decode and the option do not exist there"""
    table = {}
    for r in golden:
        states, cost, inexact = p25.trellis_decode(r["words"])
        assert (states + [0], cost, inexact) == (r["states"], r["cost"], r["n_inexact"])
        key = (r["cls"], r["flips"])
        row = table.setdefault(key, [0, 0, 0])
        row[0] += 1; row[1] += r["ref"] == r["sent"]; row[2] += r["octets"] == r["sent"]
        if r["flips"] <= 2:
            assert r["octets"] == r["sent"] and r["cost"] == r["flips"], key
    for key, (n, ref, new) in sorted(table.items()):
        print("golden class %d, %d flips: %d blocks, recovered by the reference %d, by the new rule %d" % (key + (n, ref, new)))
    within = [v for k, v in table.items() if k[1] <= 2]
    ref_failed = sum(n - ref for n, ref, _ in within)
    print("within 2 flips: the reference fails on %d of %d, the new rule on %d" % (ref_failed, sum(n for n, _, _ in within), sum(n - new for n, _, new in within)))
    assert ref_failed > 0 and all(n == new for n, _, new in within)


def test_blocks_beyond_two_flips_follow_the_brute_force_checked_form_and_identity_where_the_walk_is_exact(golden):
    """beyond the guarantee nothing is promised but the rule: the cost never exceeds the flips (the sent path is a path), and
    wherever the greedy walk finds an exact candidate at all 49 words both rules give the same bits"""
    exact = 0
    for r in golden:
        assert r["cost"] <= r["flips"] and r["states"][48] == 0
        gs, inexact = V.greedy(r["words"])
        if inexact == 0:
            exact += 1
            assert gs[:48] == r["states"][:48] and r["cost"] == 0
    rng = np.random.default_rng(5)
    for _ in range(200):                             # other cost-0 inputs: valid paths that do not end in a flush from state 0
        s, c = 0, []
        for d in rng.integers(0, 4, 48).tolist() + [0]:
            c.append(V.W[s][d]); s = d
        gs, inexact = V.greedy(c)
        assert inexact == 0 and V.sequential(c) == (gs, 0, 0)
    assert exact >= 12


# ------------------------------------------------------------------------------------------------ the header on the host
@pytest.fixture(scope="module")
def check_programs():
    """tsbk_core.hpp's trellis pieces and the wave form's walk compiled for the host, plain and with the sanitizers: stand-alone programs"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(HERE, "native", "trellis_core_check.cpp")
    exes = []
    for name, extra in (("trellis_core_check", ["-O2"]), ("trellis_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
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


def test_min_plus_composition_is_associative(check_programs):
    assert both(check_programs, ["assoc", 7, 20000]).strip() == "ok 20000"


def test_wave_form_equals_the_sequential_form_on_goldens_the_exhaustive_trellis_and_random_blocks(check_programs, tmp_path, golden):
    path = str(tmp_path / "c.u8")
    np.array([r["words"] for r in golden], np.uint8).tofile(path)
    lines = both(check_programs, ["blocks", 48, path]).strip().split("\n")
    assert len(lines) == len(golden)
    for ln, r in zip(lines, golden):
        states, cost, inexact = ln.split()
        assert ([int(ch) for ch in states], int(cost), int(inexact)) == (r["states"], r["cost"], r["n_inexact"])
    seqs = list(itertools.product(range(16), repeat=4))
    np.array(seqs, np.uint8).tofile(path)
    lines = both(check_programs, ["blocks", 3, path]).strip().split("\n")
    assert len(lines) == 16 ** 4
    for ln, c in zip(lines[::7], seqs[::7]):         # (the program holds every row to its own sequential form; these to the restatement's)
        states, cost, inexact = ln.split()
        assert ([int(ch) for ch in states], int(cost), int(inexact)) == V.sequential(list(c))
    assert both(check_programs, ["random", 11, 20000]).startswith("ok 20000 ")


def through_header(exes, tmp_path, words, k, dist, cuts, n_symbols, nid, trellis, first_hit=0, word_cap=1 << 20, hit_cap=1 << 20):
    """the stand-alone programs over the streams, a launch after each cut (a symbol count) -> (records, counters, the NID's,
    the trellis decoder's, launches)"""
    wp, hp = str(tmp_path / "words.u32"), str(tmp_path / "hits.u32")
    np.asarray(words, "<u4").tofile(wp)
    S.hit_items(k, dist).astype("<u4").tofile(hp)
    launches, args, before = [], [], 0
    for c in list(cuts) + [n_symbols]:
        launches.append((c // 16, int(np.count_nonzero(np.asarray(k) < c))))
        args += [c // 16, launches[-1][1], c, c - before]
        before = c
    lines = both(exes, ["stream", wp, hp, nid, trellis, first_hit, word_cap, hit_cap] + args).strip().split("\n")
    v = lines[0].split()
    st = {n: int(x) for n, x in zip(("n_records", "n_frames", "n_blocks", "n_crc_bad", "n_lost"), v[:5])}
    nst = {n: int(x) for n, x in zip(("n_decoded", "n_fixed", "n_bits", "n_bad"), v[6:10])}
    vst = {n: int(x) for n, x in zip(("n_decoded", "n_clean", "n_bits", "n_words"), v[11:15])}
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1:]], dtype="<u4").reshape(-1, 8)
    return recs.view(native.TSBK_DTYPE).reshape(-1), st, nst, vst, launches


def test_designed_dibits_meet_their_census_and_header_equals_restatement_under_ragged_cuts(check_programs, tmp_path):
    """the input of the GPU suite's designed carrier without a device: the generator alone meets the census, and header,
    restatement and kernel stand on one input; word 0, word 7 and the counters are as defined for both option values"""
    d, plan, starts = V.designed_dibits()
    words, k, dist = slicer_streams(d)
    assert (np.asarray(k) - 23).tolist() == starts and not np.any(dist)          # every planted frame, and nothing else
    rng = np.random.default_rng(3)
    for nid in (0, 1):
        recs, st, nst, vst = V.run(words, k, dist, V.VITERBI, nid=nid)
        twin, twin_st, twin_nst, twin_vst = V.run(words, k, dist, V.GREEDY, nid=nid)
        census = V.check_census(recs, twin, plan, native.tsbk_fields, native.trellis_fields)
        print("designed stream, nid %d: %s; %s; twin %s" % (nid, census, vst, twin_st))
        f, v = native.tsbk_fields(recs), native.trellis_fields(recs)
        blocks = f["b"] != 3
        assert vst == dict(n_decoded=int(blocks.sum()), n_clean=int(np.sum(blocks & (v["cost"] == 0))), n_bits=int(v["cost"].sum()),
                           n_words=int(f["n_inexact"][blocks].sum()))
        assert twin_vst == V.empty_state() and st["n_frames"] == twin_st["n_frames"] == len(starts) and st["n_crc_bad"] < twin_st["n_crc_bad"]
        assert not np.any(recs["frame_dibits"] >> 30) and np.all(v["viterbi"] == blocks)
        for trellis, want in ((V.VITERBI, (recs, st, nst, vst)), (V.GREEDY, (twin, twin_st, twin_nst, twin_vst))):
            for cuts in ([], sorted(rng.choice(len(d), 40).tolist()), [5, 5, 5, 6, 1500, 1500, 1501] + list(range(1600, len(d), 211))):
                got = through_header(check_programs, tmp_path, words, k, dist, cuts, len(d), nid, trellis)
                assert got[0].tobytes() == want[0].tobytes() and got[1:4] == want[1:], (nid, trellis, cuts[:6])
                again = V.run(words, k, dist, trellis, nid=nid, launches=got[4])
                assert again[0].tobytes() == want[0].tobytes() and again[1:] == want[1:]


def test_option_off_gives_the_existing_designed_stream_its_existing_records(check_programs, tmp_path):
    d, _ = T.designed_dibits()
    words, k, dist = slicer_streams(d)
    want, want_st = T.run(words, k, dist)
    got = through_header(check_programs, tmp_path, words, k, dist, [], len(d), 0, V.GREEDY)
    assert got[0].tobytes() == want.tobytes() and got[1] == want_st and got[3] == V.empty_state() and len(want) > 100
    on = through_header(check_programs, tmp_path, words, k, dist, list(range(700, len(d), 333)), len(d), 0, V.VITERBI)
    rule = V.run(words, k, dist, V.VITERBI)
    assert on[0].tobytes() == rule[0].tobytes() and (on[1], on[3]) == (rule[1], rule[3]) and on[3]["n_decoded"] == want_st["n_blocks"]
    assert int(native.tsbk_fields(on[0])["n_inexact"].max()) > 16 and int(native.trellis_fields(on[0])["cost"].max()) > 30     # noise blocks: large costs


def test_noise_hits_small_rings_and_a_late_attach_through_the_header(check_programs, tmp_path):
    d = np.random.default_rng(9).integers(0, 4, 30000).astype(np.uint8)
    words, k, dist = slicer_streams(d, max_errors=18)
    assert len(k) > 100
    cuts = list(range(2000, len(d), 96))
    got = through_header(check_programs, tmp_path, words, k, dist, cuts, len(d), 1, V.VITERBI, first_hit=2, word_cap=64, hit_cap=16)
    want = V.run(words, k, dist, V.VITERBI, nid=1, first_hit=2, launches=got[4], word_cap=64, hit_cap=16)
    assert got[0].tobytes() == want[0].tobytes() and got[1:4] == want[1:] and got[1]["n_lost"] >= 1


# ------------------------------------------------------------------------------------------------ names, constants, fields
def test_binding_names_constants_and_fields():
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RCF_\w+)\s+(-?\d+)", hdr)}
    assert (defs["RCF_TRELLIS_GREEDY"], defs["RCF_TRELLIS_VITERBI"]) == (0, 1)
    for name in ("rcf_chan_tsbk_opt", "rcf_chan_trellis_state"):
        assert name in native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr)
    assert ctypes.sizeof(native.TrellisState) == 32 and [n for n, _ in native.TrellisState._fields_] == ["n_decoded", "n_clean", "n_bits", "n_words"]
    t = np.zeros(2, native.TSBK_DTYPE)
    t["frame_dibits"] = [360 | 11 << 16 | 1 << 20 | 196 << 21 | 1 << 29, 288]
    assert {n: v.tolist() for n, v in native.trellis_fields(t).items()} == dict(cost=[196, 0], viterbi=[1, 0])
    assert {n: v.tolist() for n, v in native.nid_fields(t).items()} == dict(nid_fix=[11, 0], nid_decoded=[1, 0], frame_dibits=[360, 288])
    assert p25.tsdu_frames(t[:1])[0]["frame_dibits"] == 360
    assert inspect.signature(native.Frontend.chan_tsbk).parameters["viterbi"].default is False
    assert list(inspect.signature(native.Frontend.chan_tsbk).parameters)[1:] == ["cid", "capacity", "on", "nid", "viterbi"]
    for fn in (p25.c4fm_demod, p25.cqpsk_demod):
        assert inspect.signature(fn).parameters["viterbi"].default is False
    assert inspect.signature(p25.trellis_decode).parameters["viterbi"].default is True
    assert p25.TRELLIS == T.W
    clean = V.code_words(T.encode_block(bytes(range(12))))
    states, cost, inexact = p25.trellis_decode(clean)
    assert (V.octets_of([v for s in states for v in (s >> 1, s & 1)]), cost, inexact) == (bytes(range(12)), 0, 0)
    with pytest.raises(ValueError):
        p25.trellis_decode(clean[:48])
