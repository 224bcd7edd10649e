"""The EDACS control-frame stage (rcf_chan_edacs) without a GPU: the numpy restatement (tests/edacs_ref.py) against what the
reference's own packet_framer, message_election, bch_decode and get_next_frame returned for the frames of
tests/golden/edacs_frames.npz (made by tests/golden/make_edacs_goldens.py, which runs the reference); the kernel's arithmetic
header (radiocapture-rf_amd/csrc/edacs_core.hpp) compiled for the host and walked over the same streams as the restatement --
once more under AddressSanitizer and UBSan, as a stand-alone program --: all 2^12 syndrome pairs against the Chien walk,
every single and double error position 0 .. 62, frames at every start mod 32, ragged cuts, k across the 26-bit wrap, the
accept rule, both rings' losses, the slicer's hit rule with sync_both for every dist 0 .. 48; and the binding's names,
constants and struct sizes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edacs_ref as E
import slicer_ref as S
from rcf import control, native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "edacs_frames.npz"))


def soft_of(bits):
    return np.where(np.asarray(bits) != 0, 1.0, -1.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the reference's results
def test_restatement_gives_what_the_reference_returned_for_every_golden_frame(golden):
    g = golden
    assert len(g["kind"]) >= 300 and set(g["kind"].tolist()) == {0, 1, 2, 3, 4} and set(g["esk"].tolist()) == {0, 1}
    seen = dict(stands=0, failed=0, colour=0, none=0, single=0)
    for n in range(len(g["kind"])):
        data = np.unpackbits(g["data"][n])
        statuses, m1, m2 = E.decode_frame(data, bool(g["esk"][n]))
        for c in range(6):
            copy = data[40 * c:40 * c + 40] ^ (1 if c in (1, 4) else 0)
            st, bits, pos = E.bch(copy)
            assert st == statuses[c]
            assert (st != 3) == bool(g["copy_ok"][n, c]), (n, c)
            loc = g["loc"][n, c][:g["n_loc"][n, c]].tolist()
            if st != 3:                                        # the decoded string, and loc = 47 - position, in the walk's order
                assert np.packbits(np.array(bits, np.uint8)).tolist() == g["copy"][n, c].tolist(), (n, c)
                assert loc == [47 - p for p in pos], (n, c)
                seen["stands"] += st == 0 and bits != E.encode(bits[:28])
                seen["colour"] += any(p >= 40 for p in pos)
                seen["single"] += st == 1
            else:                                              # [-100]: the walk did not end with two; else a position past 47
                assert loc in ([-100], [47 - p for p in pos]), (n, c, loc, pos)
                assert loc == [-100] or any(p > 47 for p in pos)
                assert len(pos) != 2 or loc != [-100]
                seen["failed"] += 1
        for m, name, q in ((m1, "m1", 0), (m2, "m2", 1)):
            assert (m is not None) == bool(g["has_m"][n, q]), (n, name)
            if m is not None:
                assert np.packbits(np.array(m, np.uint8)).tolist() == g["m"][n, q].tolist(), (n, name)
            else:
                seen["none"] += 1
        # ... and as the stage writes it: one frame in a stream of words
        bits = np.concatenate([E.frame([0] * 40, [0] * 40)[:48], data, np.zeros(32, np.uint8)])
        recs, st = E.run(np.packbits(bits).view("<u4"), [47], [0], esk=bool(g["esk"][n]))
        assert control.edacs_messages(recs) == [(47, False, E.bitstr(m1), E.bitstr(m2))]
        assert native.edacs_fields(recs)["status"][0].tolist() == statuses
    assert min(seen.values()) > 0, seen                        # the fall-through, failures, colour-bit positions, "no message"
    few = g["kind"] <= 1                                       # at most two flips per copy: every message
    assert np.all(g["has_m"][few] == 1) and np.count_nonzero(few) >= 150


def test_frames_the_reference_cut_out_of_buffers_of_either_polarity(golden):
    g = golden
    assert set(g["gnf_inverted"].tolist()) == {0, 1} and len(set((g["gnf_offset"] % 32).tolist())) >= 6
    at = 0
    for n in range(len(g["gnf_bits"])):
        n_bytes = (int(g["gnf_bits"][n]) + 7) // 8
        buf = np.unpackbits(g["gnf_buf"][at:at + n_bytes])[:g["gnf_bits"][n]]
        at += n_bytes
        off = int(g["gnf_offset"][n])
        pad = (-len(buf)) % 32 + 32
        r = E.slicer(soft_of(np.concatenate([buf, np.zeros(pad, np.uint8)])))
        recs, st = E.run(r["words"], r["k"], r["dist"])
        statuses, m1, m2 = E.decode_frame(np.unpackbits(g["gnf_frame"][n]))
        got = [m for m in control.edacs_messages(recs) if m[0] == off + 47]
        assert got == [(off + 47, bool(g["gnf_inverted"][n]), E.bitstr(m1), E.bitstr(m2))] and m1 is not None and m2 is not None
        assert len(buf) - (off + 288) == g["gnf_rest"][n]      # buf[find + 288:]: the accept rule's distance
    assert at == len(g["gnf_buf"])


# ------------------------------------------------------------------------------------------------ the header on the host
@pytest.fixture(scope="module")
def check_programs():
    """edacs_core.hpp compiled for the host, plain and with the sanitizers: stand-alone programs"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(HERE, "native", "edacs_core_check.cpp")
    exes = []
    for name, extra in (("edacs_core_check", ["-O2"]), ("edacs_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(out, name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable"] + extra + [src, "-o", exe])
        exes.append(exe)
    return exes


def lines_of(exes, *args):
    outs = []
    for exe in exes:
        p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert p.returncode == 0, (exe, p.stdout.decode()[-2000:])
        outs.append(p.stdout.decode())
    assert outs[0] == outs[1]
    return outs[0].strip().split("\n")


def through_header(exes, tmp_path, words, k, dist, cuts, n_symbols, first_hit=0, word_cap=1 << 20, hit_cap=1 << 20, flags=1,
                   base_words=0, base_hits=0):
    """the stand-alone programs over the streams, a launch after each cut (a symbol count) -> (records, counters, launches)"""
    wp, hp = str(tmp_path / "words.u32"), str(tmp_path / "hits.u32")
    np.asarray(words, "<u4").tofile(wp)
    S.hit_items(k, dist).astype("<u4").tofile(hp)
    launches, args, before = [], [], 32 * base_words
    for c in list(cuts) + [n_symbols]:
        launches.append((c // 32, base_hits + int(np.count_nonzero(np.asarray(k) < c))))
        args += [c // 32, launches[-1][1], c, c - before]
        before = c
    lines = lines_of(exes, "stream", wp, hp, first_hit, word_cap, hit_cap, flags, base_words, base_hits, *args)
    names = lines[0].split()
    st = {"n_" + names[i]: int(names[i + 1]) for i in range(0, 10, 2)}
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1:]], dtype="<u4").reshape(-1, 8)
    return recs.view(native.EDACS_DTYPE).reshape(-1), st, launches


def planted(seed, starts, flips=2, inverted=()):
    """random bits with frames planted at the given starts, up to `flips` flipped bits in every copy -> (bits, the two
    messages sent per frame)"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, starts[-1] + 640).astype(np.uint8)
    sent = []
    for n, s in enumerate(starts):
        m1, m2 = E.encode(rng.integers(0, 2, 28)), E.encode(rng.integers(0, 2, 28))
        f = E.frame(m1, m2, inverted=n in inverted)
        for c in range(6):
            for at in rng.choice(40, int(rng.integers(0, flips + 1)), replace=False):
                f[48 + 40 * c + at] ^= 1
        bits[s:s + 288] = f
        sent.append((E.bitstr(m1), E.bitstr(m2)))
    return bits, sent


def test_planted_frames_at_every_start_mod_32_through_the_header(check_programs, tmp_path):
    starts = [100 + 321 * n for n in range(32)]                    # 321 = 1 mod 32: every start mod 32 once
    assert sorted(s % 32 for s in starts) == list(range(32))
    bits, sent = planted(7, starts, inverted=set(range(1, 32, 3)))
    r = E.slicer(soft_of(bits))
    want, want_st = E.run(r["words"], r["k"], r["dist"])
    got, st, _ = through_header(check_programs, tmp_path, r["words"], r["k"], r["dist"], [], len(bits))
    assert got.tobytes() == want.tobytes() and st == want_st
    msgs = {m[0]: m for m in control.edacs_messages(want)}
    for n, (s, (m1, m2)) in enumerate(zip(starts, sent)):         # at most two flips per copy: every sent message comes back
        assert msgs[s + 47] == (s + 47, n % 3 == 1, m1, m2)
    assert want_st["n_msgs"] >= 64 and want_st["n_lost"] == 0
    # esk, and a slicer that searches one polarity: the inverted frames are not there
    got, st, _ = through_header(check_programs, tmp_path, r["words"], r["k"], r["dist"], [], len(bits), flags=3)
    want_e, want_e_st = E.run(r["words"], r["k"], r["dist"], esk=True)
    assert got.tobytes() == want_e.tobytes() and st == want_e_st and got.tobytes() != want.tobytes()
    one = E.slicer(soft_of(bits), sync_both=0)
    got, st, _ = through_header(check_programs, tmp_path, one["words"], one["k"], one["dist"], [], len(bits), flags=0)
    want_1, want_1_st = E.run(one["words"], one["k"], one["dist"], sync_both=False)
    assert got.tobytes() == want_1.tobytes() and st == want_1_st and not np.any(want_1["flags"] & 1)
    assert st["n_frames"] == len([n for n in range(32) if n % 3 != 1])


def test_back_to_back_frames_ragged_cuts_and_both_rings_losses_through_the_header(check_programs, tmp_path):
    starts = [37, 325, 613, 901, 1200, 1488, 1801]                 # three back to back, then gaps, not aligned to a word
    bits, sent = planted(8, starts)
    loose = E.slicer(soft_of(bits), max_errors=12)                 # many more hits than frames: most are rejected or garbage
    assert len(loose["k"]) > 3 * len(starts)
    for r in (E.slicer(soft_of(bits)), loose):
        want, want_st = E.run(r["words"], r["k"], r["dist"])
        rng = np.random.default_rng(9)
        for cuts in ([], sorted(rng.choice(len(bits), 60).tolist()), list(range(0, len(bits), 7)), [5, 5, 5, 6, 1500, 1500, 1501]):
            got, st, launches = through_header(check_programs, tmp_path, r["words"], r["k"], r["dist"], cuts, len(bits))
            assert got.tobytes() == want.tobytes() and st == want_st, cuts[:8]
            again, again_st = E.run(r["words"], r["k"], r["dist"], launches=launches)      # the restatement under the same cuts
            assert again.tobytes() == want.tobytes() and again_st == want_st
    r = E.slicer(soft_of(bits))
    want, want_st = E.run(r["words"], r["k"], r["dist"])
    assert [m[1:] for m in control.edacs_messages(want) if m[0] - 47 in starts] == [(False,) + s for s in sent]
    # a word ring of 16 words and launches longer than it: lost frames as in the restatement, and decoding goes on afterwards
    got, st, launches = through_header(check_programs, tmp_path, r["words"], r["k"], r["dist"], [300, 1700], len(bits), word_cap=16)
    want_l, want_l_st = E.run(r["words"], r["k"], r["dist"], launches=launches, word_cap=16)
    assert got.tobytes() == want_l.tobytes() and st == want_l_st and st["n_lost"] >= 1 and 0 < st["n_records"] < want_st["n_records"]
    # a hit ring of 16 and a stage attached at hit 2
    got, st, launches = through_header(check_programs, tmp_path, loose["words"], loose["k"], loose["dist"], [900], len(bits), first_hit=2, hit_cap=16)
    want_h, want_h_st = E.run(loose["words"], loose["k"], loose["dist"], first_hit=2, launches=launches, hit_cap=16)
    assert got.tobytes() == want_h.tobytes() and st == want_h_st and st["n_lost"] >= 1


def test_designed_bits_guarantee_their_census_and_header_equals_restatement_on_them(check_programs, tmp_path):
    """the inputs of the GPU suite's designed carriers (E.designed_bits) without a device: what they guarantee, and the header
    on the same streams -- header, restatement and kernel stand on one input"""
    singles, pairs = E.flip_patterns()
    assert len(singles) == 40 and len(pairs) == 780 and len(set(pairs)) == 780
    classes, found = E.designed_classes()
    assert all(found[c] >= 10 for c in E.CLASSES), found       # the bounded search finds every class
    n_frames = 0
    for patterns, inverted, seed in ((singles, True, 61), (pairs, False, 62), (classes, False, 62)):
        bits, sent, starts, planted = E.designed_bits(patterns, seed, inverted=inverted)
        bits = np.concatenate([bits, np.zeros(-len(bits) % 32, np.uint8)])
        r = E.slicer(soft_of(bits))
        assert (np.asarray(r["k"]) - 47).tolist() == starts and np.all(r["dist"] == (48 if inverted else 0))
        frames = []
        want, want_st = E.run(r["words"], r["k"], r["dist"], frames=frames)
        f = native.edacs_fields(want)
        assert want_st["n_records"] == len(starts) and np.all(f["inverted"] == inverted)
        n_frames += len(starts)
        if patterns is not classes:                            # per copy status == number of flips; every message as sent
            assert f["status"].tolist() == [[len(p) for p in six] for six in planted]
            assert sorted(p for six in planted for p in six if p) == patterns
            assert [(m[2], m[3]) for m in control.edacs_messages(want)] == sent
            slots = {(len(p), c) for six in planted for c, p in enumerate(six) if p}
            assert slots == {(len(patterns[0]), c) for c in range(6)}                        # every slot gets the kind
        else:
            seen = E.census(frames, sent)
            assert all(seen[c] >= 10 for c in E.CLASSES) and min(seen["one"], seen["differ"], seen["outvoted"]) >= 2, seen
            assert want_st["n_msgs_none"] == seen["differ"]
            slots = {c for six in planted for c, p in enumerate(six) if len(p) > 2}
            assert slots == set(range(6))
        for cuts in ([], list(range(0, len(bits), 997))):
            got, st, _ = through_header(check_programs, tmp_path, r["words"], r["k"], r["dist"], cuts, len(bits))
            assert got.tobytes() == want.tobytes() and st == want_st, (seed, cuts[:4])
    assert n_frames == 137 + len(classes) // 6


def test_accept_rule_with_hits_280_to_296_bits_apart(check_programs, tmp_path):
    rng = np.random.default_rng(10)
    gaps = list(range(280, 297))
    bits = rng.integers(0, 2, 1024 * (len(gaps) + 1)).astype(np.uint8)
    words = np.packbits(bits).view("<u4")
    k, accepted = [], []
    for n, gap in enumerate(gaps):                                 # a pair of hits `gap` apart, then one 5 behind the second
        base = 1000 * n + 100
        k += [base, base + gap, base + gap + 5]
        accepted += [base] + ([base + gap] if gap >= 288 else [base + gap + 5] if gap + 5 >= 288 else [])
    dist = list(rng.integers(0, 5, len(k)))
    want, want_st = E.run(words, k, dist)
    assert want["k"].tolist() == accepted and want_st["n_frames"] == len(accepted)
    for cuts in ([], list(range(0, len(bits), 11))):
        got, st, _ = through_header(check_programs, tmp_path, words, k, dist, cuts, len(bits))
        assert got.tobytes() == want.tobytes() and st == want_st


def test_k_across_the_26_bit_wrap(check_programs, tmp_path):
    starts = [40 + 300 * n for n in range(8)]
    bits, sent = planted(11, starts, inverted={2, 5})
    r = E.slicer(soft_of(bits))
    base_words, base_hits = ((1 << 26) - 1100) // 32, 5
    k = r["k"] + 32 * base_words
    assert k[0] < (1 << 26) < k[-1]
    want, want_st = E.run(r["words"], k, r["dist"], first_hit=base_hits, base_words=base_words, base_hits=base_hits)
    assert [(m[0] - 32 * base_words - 47, m[2], m[3]) for m in control.edacs_messages(want) if m[0] - 32 * base_words - 47 in starts] == \
        [(s,) + m for s, m in zip(starts, sent)]
    for cuts in ([], [32 * base_words + c for c in range(3, len(bits), 97)]):
        got, st, _ = through_header(check_programs, tmp_path, r["words"], k, r["dist"], cuts, 32 * base_words + len(bits),
                                    first_hit=base_hits, base_words=base_words, base_hits=base_hits)
        assert got.tobytes() == want.tobytes() and st == want_st
    n = (1 << 26) + 1000
    for true_k in (n - (1 << 26), (1 << 26) - 1, 1 << 26, n - 1):
        item = int(S.hit_items([true_k], [3])[0])
        assert [int(v) for v in lines_of(check_programs, "widen", "%x" % item, n)] == [true_k] == [int(native.widen_hits([item], n)[0][0])]


def test_all_syndrome_pairs_and_all_single_and_double_errors(check_programs):
    lines = lines_of(check_programs, "syn")
    assert len(lines) == 4096
    kinds = [0, 0, 0, 0]
    for ln in lines:
        s1, s3, cls, status, pos, flip = ln.split()
        want_status, want_pos = E.solve(int(s1), int(s3))
        want_mask = sum(1 << p for p in want_pos)
        assert (int(status), int(pos, 16)) == (want_status, want_mask), ln
        assert int(flip, 16) == (want_mask & ((1 << 40) - 1) if want_status in (1, 2) else 0), ln
        assert int(cls) == (0 if int(s1) == 0 else 1 if len(want_pos) == 1 and E.ALPHA[3 * E.LOG[int(s1)] % 63] == int(s3) else 2)
        kinds[want_status] += 1
    assert kinds[0] == 64 and kinds[1] == 48 and min(kinds) > 0   # S1 = 0 stands whatever S3 is; 48 correctable single positions
    lines = lines_of(check_programs, "errors")
    assert len(lines) == 63 * 64 // 2
    for ln in lines:
        p, q, status, pos, flip = ln.split()
        p, q = int(p), int(q)
        where = {p, q}
        assert E.solve(*E.syndromes(sorted(where)))[0] == int(status)
        assert int(pos, 16) == sum(1 << v for v in where), ln     # the positions are found wherever they are ...
        if q > 47:                                                 # ... and past the word they fail the copy
            assert int(status) == 3 and int(flip, 16) == 0
        else:
            assert int(status) == len(where) and int(flip, 16) == sum(1 << v for v in where if v < 40)


def test_slicer_hit_rule_with_sync_both_for_every_dist(check_programs):
    lines = lines_of(check_programs, "hits")
    assert len(lines) == 3 * 48
    for ln in lines:
        v = [int(x) for x in ln.split()]
        both, me, ok, hits = v[0], v[1], v[2], v[3:]
        assert ok == (both == 0 or (both == 1 and 2 * me < 48))
        assert hits == [int(d <= me or (both != 0 and d >= 48 - me)) for d in range(49)] == [int(E.is_hit(d, me, both)) for d in range(49)]
        if both == 0:
            assert hits == [int(d <= me) for d in range(49)]      # as before


def test_edacs_messages_gives_the_references_strings():
    m1, m2 = E.encode([1, 0] * 14), E.encode([0, 1, 1] * 9 + [1])
    bits = np.concatenate([np.zeros(17, np.uint8), E.frame(m1, m2), np.ones(300, np.uint8), E.frame(m1, [b ^ 1 for b in m2], inverted=True), np.zeros(64, np.uint8)])
    bits[17 + 48 + 120:17 + 48 + 240] ^= np.random.default_rng(0).integers(0, 2, 120).astype(np.uint8)      # all three copies of m2 beyond repair
    assert E.decode_frame(bits[17 + 48:17 + 288])[0] == [0, 0, 0, 3, 3, 3]
    r = E.slicer(soft_of(bits[:len(bits) // 32 * 32]))
    recs, st = E.run(r["words"], r["k"], r["dist"], esk=True)
    esk = lambda m: E.bitstr([m[0] | 1, m[1], m[2] | 1, m[3]] + m[4:])
    got = control.edacs_messages(recs)
    assert got[0] == (17 + 47, False, esk(m1), -1) and got[1][:3] == (17 + 288 + 300 + 47, True, esk(m1))
    assert st["n_msgs_none"] >= 1 and st["n_frames"] == 2


# ------------------------------------------------------------------------------------------------ names, constants, sizes
def test_binding_names_constants_and_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RCF_\w+)\s+(-?\d+)", hdr)}
    assert native.HARD_EDACS == defs["RCF_HARD_EDACS"] == 49 and native.HARD_TSBK == 48
    assert native.T_SLICE == defs["RCF_T_SLICE"] == 13 and defs["RCF_T_COUNT"] == 14
    assert native._read_what("edacs", True) == 49 and native._read_what("edacs") == native.READ_FM
    assert native._read_dtype("edacs") == native.EDACS_DTYPE and native.EDACS_DTYPE.itemsize == 32
    assert [native.EDACS_DTYPE.fields[n][1] for n in ("flags", "k", "m1", "m2", "zero")] == [0, 4, 8, 16, 24]
    assert C.sizeof(native.EdacsParams) == 16 and C.sizeof(native.EdacsState) == 40
    assert re.search(r"typedef struct rcf_edacs_params \{\s*int capacity;[^}]*int esk;[^}]*int reserved_\[2\];\s*\} rcf_edacs_params_t;", hdr)
    # sync_both took the place of the slicer's reserved field: same size, same offset
    assert re.search(r"int hit_capacity;[^}]*\n\s*int sync_both;[^}]*\} rcf_slicer_params_t;", hdr)
    assert C.sizeof(native.SlicerParams) == 48 and native.SlicerParams.sync_both.offset == 44 and native.SlicerParams.hit_capacity.offset == 40
    for name in ("rcf_chan_edacs", "rcf_chan_edacs_state", "rcf_chan_read_edacs", "rcf_chan_edacs_ring"):
        assert name in native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr)
    for name in ("chan_edacs", "chan_edacs_state", "chan_read_edacs", "chan_edacs_ring"):
        assert callable(getattr(native.Frontend, name))
    assert callable(control.edacs_messages)
    # the readers' row behind the stream table's eleven: kind 11, records of 8 words, uint32, counted; the table itself and
    # stream_kind, which are the pump's as well, stay as they were, so the pump refuses 49 as a stream it does not know
    exe = os.path.join(HERE, "native", "_build", "edacs_stream_row")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    prog = ('#include <cstdio>\n#include "rcf_streams.h"\nusing namespace rcfx;\nint main() { const int k = read_kind(RCF_HARD_EDACS); '
            'const StreamKind &r = read_row(k); printf("%d %d %u %d %d %d %d %d %d %d\\n", k, (int)kReadKinds, r.item_w, (int)r.u32, (int)r.counted, '
            '(int)r.pumped, read_kind(50), (int)kStreamKinds, stream_kind(RCF_HARD_EDACS), read_kind(RCF_HARD_TSBK)); return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-x", "c++", "-", "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc"), "-o", exe],
                   input=prog.encode(), check=True)
    assert subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode().split() == ["11", "12", "8", "1", "1", "0", "-1", "11", "-1", "10"]
    f = native.edacs_fields(np.array([(0b11_10_01_00_11_01 << 10 | 37 << 4 | 4 | 1, 0, [0] * 8, [0] * 8, [0, 0])], native.EDACS_DTYPE))
    assert (int(f["inverted"][0]), int(f["has_m1"][0]), int(f["has_m2"][0]), int(f["dist"][0])) == (1, 0, 1, 37)
    assert f["status"][0].tolist() == [1, 3, 0, 1, 2, 3]
