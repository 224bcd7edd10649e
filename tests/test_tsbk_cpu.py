"""The P25 trunking stage (rcf_chan_tsbk) without a GPU: the numpy restatement (tests/tsbk_ref.py) against what the
reference's own procTSDU returned for the frames of tests/golden/p25_tsdu.npz (made by tests/golden/make_tsbk_goldens.py,
which runs the reference); the kernel's arithmetic header (radiocapture-rf_amd/csrc/tsbk_core.hpp) compiled for the host
and walked over the same streams as the restatement -- once more under AddressSanitizer and UBSan --: planted frames at
every start mod 16, ragged cuts, the six-step scan against the 49-step walk, all 64 (state, code word) pairs, the 26-bit
widening of k, the accept rule; and the binding's names, constants and struct sizes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import slicer_ref as S
import tsbk_ref as T
from rcf import native, p25

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOFT = np.array([1.0, 3.0, -1.0, -3.0], np.float32)              # a soft symbol in the middle of each dibit's interval
SYNC = dict(sync_word=p25.FRAME_SYNC, sync_bits=48, max_errors=4)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "p25_tsdu.npz"))


def slicer_streams(dibits):
    r = S.run(SOFT[np.asarray(dibits)], S.FSK4, **SYNC)
    return r["words"], r["k"], r["dist"]


# ------------------------------------------------------------------------------------------------ the reference's results
def test_restatement_gives_what_the_reference_returned_for_every_golden_frame(golden):
    g = golden
    assert len(g["lengths"]) >= 300 and set(g["lengths"].tolist()) == {45, 72, 90} and set(g["flips"].tolist()) == {0, 1, 2, 4, 8}
    at = blk = 0
    stopped_early = 0
    for n_bytes, count, nid in zip(g["lengths"], g["counts"], g["nid"]):
        by = g["frames"][at:at + n_bytes]
        at += n_bytes
        fd = 4 * int(n_bytes)
        stream = np.concatenate([by, np.zeros(4 * ((T.DECIDE - fd + 15) // 16), np.uint8)])     # the frame, then nulls up to the decision
        recs, st = T.run(stream, [23, 23 + fd], [0, 0])
        frames = p25.tsdu_frames(recs, reference_rule=True)
        assert len(frames) == 1 and frames[0]["frame_dibits"] == fd and st["n_frames"] == 1
        assert int.from_bytes(frames[0]["nid"], "big") == int(nid) and frames[0]["duid"] == 7
        got = frames[0]["tsbk"]
        assert len(got) == count, (at, len(got), count)
        stopped_early += len(p25.tsdu_frames(recs)[0]["tsbk"]) > count
        for t in got:
            assert t["octets"] == g["octets"][blk].tobytes() and t["crc"] == g["crc"][blk], (at, blk)
            assert (t["octets"][0] >> 7, t["octets"][0] & 63, t["octets"][1]) == (g["lb"][blk], g["opcode"][blk], g["mfid"][blk])
            blk += 1
    assert blk == len(g["crc"]) and at == len(g["frames"])
    assert stopped_early > 50                                      # the goldens exercise procTSDU's early stop
    clean = g["flips"] == 0
    assert int(np.sum(g["counts"][clean])) > 0 and not np.any(g["crc"][:int(np.sum(g["counts"][clean]))])   # clean frames come first


# ------------------------------------------------------------------------------------------------ the header on the host
@pytest.fixture(scope="module")
def check_programs():
    """tsbk_core.hpp compiled for the host, plain and with the sanitizers: stand-alone programs"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(HERE, "native", "tsbk_core_check.cpp")
    exes = []
    for name, extra in (("tsbk_core_check", ["-O2"]), ("tsbk_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(out, name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-variable"] + extra + [src, "-o", exe])
        exes.append(exe)
    return exes


def through_header(exes, tmp_path, words, k, dist, cuts, n_symbols, first_hit=0, word_cap=1 << 20, hit_cap=1 << 20):
    """the stand-alone programs over the streams, a launch after each cut (a symbol count) -> (records, counters, launches)"""
    wp, hp = str(tmp_path / "words.u32"), str(tmp_path / "hits.u32")
    np.asarray(words, "<u4").tofile(wp)
    S.hit_items(k, dist).astype("<u4").tofile(hp)
    launches, args, before = [], [], 0
    for c in list(cuts) + [n_symbols]:
        launches.append((c // 16, int(np.count_nonzero(np.asarray(k) < c))))
        args += [c // 16, launches[-1][1], c, c - before]
        before = c
    outs = []
    for exe in exes:
        p = subprocess.run([exe, "stream", wp, hp, str(first_hit), str(word_cap), str(hit_cap)] + [str(a) for a in args],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert p.returncode == 0, (exe, p.stdout.decode()[-2000:])
        outs.append(p.stdout.decode())
    assert outs[0] == outs[1]
    lines = outs[0].strip().split("\n")
    names = lines[0].split()
    st = {"n_" + names[i]: int(names[i + 1]) for i in range(0, 10, 2)}
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1:]], dtype="<u4").reshape(-1, 8)
    return recs.view(native.TSBK_DTYPE).reshape(-1), st, launches


def planted(seed, starts, kinds=None):
    """random dibits with TSDUs planted at the given starts -> (dibits, the TSBKs sent per frame)"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 4, starts[-1] + 800).astype(np.uint8)
    sent = []
    for n, s in enumerate(starts):
        tsbks = [T.tsbk_octets(rng) for _ in range((kinds or [3, 1, 2])[n % len(kinds or [3, 1, 2])])]
        f = T.frame(0x293, 7, tsbks, rng)
        d[s:s + len(f)] = f
        sent.append(tsbks)
    return d, sent


def test_planted_frames_at_every_start_mod_16_through_the_header(check_programs, tmp_path):
    starts = [100 + 401 * n for n in range(16)]                    # 401 = 1 mod 16: every start mod 16 once
    assert sorted(s % 16 for s in starts) == list(range(16))
    d, sent = planted(7, starts)
    words, k, dist = slicer_streams(d)
    want, want_st = T.run(words, k, dist)
    got, st, _ = through_header(check_programs, tmp_path, words, k, dist, [], len(d))
    assert got.tobytes() == want.tobytes() and st == want_st
    frames = {f["k"]: f for f in p25.tsdu_frames(want)}
    for s, tsbks in zip(starts, sent):                             # every sent TSBK comes back with a good CRC
        f = frames[s + 23]
        assert [t["octets"] for t in f["tsbk"][:len(tsbks)]] == tsbks and not any(t["crc"] or t["n_inexact"] for t in f["tsbk"][:len(tsbks)])
        assert (f["nac"], f["duid"]) == (0x293, 7)
    assert want_st["n_blocks"] >= sum(len(t) for t in sent) and want_st["n_lost"] == 0


def test_back_to_back_frames_and_ragged_cuts_through_the_header(check_programs, tmp_path):
    # three 360-dibit frames back to back, then a 180-, a 288- and a 360-dibit one, not aligned to a word
    starts = [37, 397, 757, 1117, 1297, 1585]
    d, sent = planted(8, starts, kinds=[3, 3, 3, 1, 2, 3])
    words, k, dist = slicer_streams(d)
    want, want_st = T.run(words, k, dist)
    frames = p25.tsdu_frames(want)
    assert [f["frame_dibits"] for f in frames if f["k"] - 23 in starts] == [360, 360, 360, 180, 288, 360]
    rng = np.random.default_rng(9)
    for cuts in ([], sorted(rng.choice(len(d), 60).tolist()), list(range(0, len(d), 7)), [5, 5, 5, 6, 1500, 1500, 1501]):
        got, st, launches = through_header(check_programs, tmp_path, words, k, dist, cuts, len(d))
        assert got.tobytes() == want.tobytes() and st == want_st, cuts[:8]
        again, again_st = T.run(words, k, dist, launches=launches)               # the restatement under the same cuts
        assert again.tobytes() == want.tobytes() and again_st == want_st
    # a ring of 64 words and launches longer than it: lost frames as in the restatement, and decoding goes on afterwards
    cuts = [300, 1700]
    got, st, launches = through_header(check_programs, tmp_path, words, k, dist, cuts, len(d), word_cap=64)
    want_l, want_l_st = T.run(words, k, dist, launches=launches, word_cap=64)
    assert got.tobytes() == want_l.tobytes() and st == want_l_st and st["n_lost"] >= 1 and 0 < st["n_records"] < want_st["n_records"]
    # a hit ring of 16 and a stage attached at hit 2
    loose = S.run(SOFT[d], S.FSK4, sync_word=p25.FRAME_SYNC, sync_bits=48, max_errors=18)
    assert len(loose["k"]) > 40
    got, st, launches = through_header(check_programs, tmp_path, loose["words"], loose["k"], loose["dist"], [900], len(d), first_hit=2, hit_cap=16)
    want_h, want_h_st = T.run(loose["words"], loose["k"], loose["dist"], first_hit=2, launches=launches, hit_cap=16)
    assert got.tobytes() == want_h.tobytes() and st == want_h_st and st["n_lost"] >= 1


def test_designed_dibits_guarantee_their_census_and_header_equals_restatement_on_them(check_programs, tmp_path):
    """the input of the GPU suite's designed carrier (T.designed_dibits) without a device: what it guarantees, and the header
    on the same stream -- header, restatement and kernel stand on one input"""
    d, starts = T.designed_dibits()
    assert len(starts) == 50 and 16000 < len(d) < 20000
    words, k, dist = slicer_streams(d)
    assert (np.asarray(k) - 23).tolist() == starts and not np.any(dist)           # every planted frame, and nothing else
    blocks = []
    want, want_st = T.run(words, k, dist, blocks=blocks)
    T.check_census(T.census(blocks, want_st))
    frames = p25.tsdu_frames(want)
    assert [f["frame_dibits"] for f in frames] == T.DESIGNED_FRAME_DIBITS and want_st["n_blocks"] == len(blocks) == 147
    # what set 2 is made of: a valid TSBK with 1 .. 4 wrong dibits, one of them in the code word asked for (48: dibits 24, 25)
    rng = np.random.default_rng(5)
    for t in range(49):
        octets = T.tsbk_octets(rng)
        block = T.damaged_block(octets, t, 1 + t % 4, rng)
        wrong = {p for p, (a, b) in enumerate(zip(T.encode_block(octets), block)) if a != b}
        assert len(wrong) == 1 + t % 4 and len(wrong & {T.ORDER[2 * t], T.ORDER[2 * t + 1]}) == 1, (t, wrong)
    assert (T.ORDER[96], T.ORDER[97]) == (24, 25)
    # the blocks of sets 2 and 3 as delivered: 54 blocks that are no code words' images, of which the walk repairs some
    damaged = [T.decode_block(b) for b in blocks[90:144]]
    assert any(inexact > 0 and not bad for _, bad, inexact in damaged) and 0 < sum(bad for _, bad, _ in damaged) < 54
    assert [T.decode_block(b)[1:] for b in blocks[144:]] == [(0, 0)] * 3        # the last frame is clean
    for cuts in ([], list(range(0, len(d), 997))):
        got, st, _ = through_header(check_programs, tmp_path, words, k, dist, cuts, len(d))
        assert got.tobytes() == want.tobytes() and st == want_st, cuts[:4]


def test_accept_rule_with_hits_1_to_30_dibits_apart(check_programs, tmp_path):
    rng = np.random.default_rng(10)
    d = rng.integers(0, 4, 30 * 500 + 600).astype(np.uint8)
    words = np.packbits(np.stack([(d >> 1) & 1, d & 1], axis=1).reshape(-1)).view("<u4")
    k, accepted = [], []
    for gap in range(1, 31):                                       # a pair of hits `gap` apart, then one 3 behind the second
        k += [500 * gap, 500 * gap + gap, 500 * gap + gap + 3]
        accepted += [500 * gap] + ([500 * gap + gap] if gap >= 24 else [500 * gap + gap + 3] if gap + 3 >= 24 else [])
    dist = list(rng.integers(0, 5, len(k)))
    want, want_st = T.run(words, k, dist)
    assert sorted(set(want["k"].tolist())) == accepted and want_st["n_frames"] == len(accepted)
    short = want[np.isin(want["k"], [500 * g for g in range(24, 31)])]
    assert sorted(set(short["frame_dibits"].tolist())) == list(range(24, 31))          # a frame ends where the next accepted one starts
    for cuts in ([], list(range(0, len(d), 11))):
        got, st, _ = through_header(check_programs, tmp_path, words, k, dist, cuts, len(d))
        assert got.tobytes() == want.tobytes() and st == want_st


def test_scan_pairs_and_widening(check_programs):
    ladder = []
    for s in range(4):
        for c in range(16):
            same = [4 - bin(T.W[s][d] ^ c).count("1") for d in range(4)]
            # the reference's ladder: the one candidate with 4, else the one with 3, else the first with the best count
            if same.count(4) == 1:
                d = same.index(4)
            elif same.count(3) == 1:
                d = same.index(3)
            else:
                d = next(same.index(j) for j in range(3, -1, -1) if same.count(j) > 0)
            ladder.append("%d %d %d %d" % (s, c, d, 4 in same))
    for exe in check_programs:
        assert subprocess.run([exe, "pairs"], stdout=subprocess.PIPE, timeout=60, check=True).stdout.decode().split("\n")[:-1] == ladder
        assert subprocess.run([exe, "scan", "5", "2000"], stdout=subprocess.PIPE, timeout=60, check=True).stdout.decode().strip() == "ok 2000"
        n = (1 << 26) + 1000
        for true_k in (n - (1 << 26), (1 << 26) - 1, 1 << 26, n - 1):
            item = int(S.hit_items([true_k], [3])[0])
            out = subprocess.run([exe, "widen", "%x" % item, str(n)], stdout=subprocess.PIPE, timeout=60, check=True).stdout.decode()
            assert int(out) == true_k == int(native.widen_hits([item], n)[0][0])


def test_tsdu_frames_groups_records_and_applies_the_reference_rule():
    rng = np.random.default_rng(12)
    d, sent = planted(13, [64, 500], kinds=[3, 2])
    recs, _ = T.run(*slicer_streams(d))
    all_, ref = p25.tsdu_frames(recs), p25.tsdu_frames(recs, reference_rule=True)
    for fa, fr, tsbks in zip([f for f in all_ if f["k"] in (87, 523)], [f for f in ref if f["k"] in (87, 523)], sent):
        assert [t["octets"] for t in fa["tsbk"][:len(tsbks)]] == tsbks
        stop = next((i for i, t in enumerate(fa["tsbk"]) if t["next_bit"]), len(fa["tsbk"]) - 1)
        assert fr["tsbk"] == fa["tsbk"][:stop + 1]
    other = T.frame(0x123, 5, [], rng, total=360)                  # another data unit: a frame record
    recs, st = T.run(*slicer_streams(np.concatenate([np.zeros(40, np.uint8), other, np.zeros(420, np.uint8)])))
    f = [f for f in p25.tsdu_frames(recs) if f["k"] == 63]
    assert len(f) == 1 and f[0]["duid"] == 5 and f[0]["nac"] == 0x123 and f[0]["tsbk"] == [] and st["n_blocks"] == 0


# ------------------------------------------------------------------------------------------------ names, constants, sizes
def test_binding_names_constants_and_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RCF_\w+)\s+(-?\d+)", hdr)}
    assert native.HARD_TSBK == defs["RCF_HARD_TSBK"] == 48
    assert native.T_SLICE == defs["RCF_T_SLICE"] == 13 and defs["RCF_T_COUNT"] == 14
    assert native._read_what("tsbk", True) == 48 and native._read_what("tsbk") == native.READ_FM
    assert native._read_dtype("tsbk") == native.TSBK_DTYPE and native.TSBK_DTYPE.itemsize == 32
    assert [native.TSBK_DTYPE.fields[n][1] for n in ("flags", "k", "octets", "nid", "frame_dibits")] == [0, 4, 8, 20, 28]
    assert C.sizeof(native.TsbkParams) == 16 and C.sizeof(native.TsbkState) == 40
    assert re.search(r"typedef struct rcf_tsbk_params \{\s*int capacity;[^}]*int reserved_\[3\];\s*\} rcf_tsbk_params_t;", hdr)
    for name in ("rcf_chan_tsbk", "rcf_chan_tsbk_state", "rcf_chan_read_tsbk", "rcf_chan_tsbk_ring"):
        assert name in native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr)
    for name in ("chan_tsbk", "chan_tsbk_state", "chan_read_tsbk", "chan_tsbk_ring"):
        assert callable(getattr(native.Frontend, name))
    # the stream table's eleventh row: kind 10, records of 8 words, uint32, counted, and not the pump's to deliver
    # (rcf_pump_start and rcf_pump_subscribe refuse whatever the table does not mark as pumped)
    exe = os.path.join(HERE, "native", "_build", "tsbk_stream_row")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    prog = ('#include <cstdio>\n#include "rcf_streams.h"\nusing namespace rcfx;\nint main() { const int k = stream_kind(RCF_HARD_TSBK); '
            'const StreamKind &r = kStreams[k]; printf("%d %d %u %d %d %d %d\\n", k, (int)kStreamKinds, r.item_w, (int)r.u32, (int)r.counted, '
            '(int)r.pumped, stream_kind(47) + stream_kind(49)); return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-x", "c++", "-", "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc"), "-o", exe],
                   input=prog.encode(), check=True)
    assert subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode().split() == ["10", "11", "8", "1", "1", "0", "-2"]
    pump = open(os.path.join(ROOT, "radiocapture-rf_amd", "csrc", "rcf_pump.cpp")).read()
    assert pump.count("!kStreams[stream_kind(cfg->what)].pumped") == 1 and pump.count("!kStreams[stream_kind(what)].pumped") == 1
    f = native.tsbk_fields(np.array([(0xABC7_0000 | 63 << 10 | 49 << 4 | 8 | 4 | 2, 0, [0] * 12, [0] * 8, 0)], native.TSBK_DTYPE))
    assert {n: int(v[0]) for n, v in f.items()} == dict(b=2, crc_bad=1, next_bit=1, n_inexact=49, dist=63, duid=7, nac=0xABC)
