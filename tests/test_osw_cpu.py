"""The SmartNet OSW stage (rcf_chan_osw) without a GPU: the numpy restatement (tests/osw_ref.py) against what the reference's
own receive_engine published for the streams of tests/golden/smartnet_osw.npz (made by tests/golden/make_osw_goldens.py,
which runs the reference); the kernel's arithmetic header (radiocapture-rf_amd/csrc/osw_core.hpp) compiled for the host and
walked over the same streams as the restatement -- once more under AddressSanitizer and UBSan, as a stand-alone program --:
the golden, designed and lock streams under ragged cuts, frames at every start mod 32, k across the 26-bit wrap, both rings'
losses; the correction as one mask against the reference's sequential loop; and the binding's names, constants and sizes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import osw_ref as O
import slicer_ref as S
from rcf import control, native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "smartnet_osw.npz"))
    streams, events, a, e = [], [], 0, 0
    for nb, ne in zip(g["n_bytes"], g["n_events"]):
        streams.append(g["streams"][a:a + nb])
        events.append({name: g[name][e:e + ne] for name in ("lid", "ind", "cmd", "tg", "status", "packets", "packets_bad", "is_locked")})
        a += nb; e += ne
    assert a == len(g["streams"]) and e == len(g["lid"])
    return streams, events


def padded(bits):
    return np.concatenate([np.asarray(bits, np.uint8), np.zeros(-len(bits) % 32, np.uint8)])


# ------------------------------------------------------------------------------------------------ the reference's results
def test_restatement_and_smartnet_osws_give_what_the_reference_published_for_every_golden_stream(golden):
    streams, events = golden
    assert len(streams) == 60 and sum(len(e["lid"]) for e in events) > 2000
    seen = dict(rejects=0, negative=0, locked=0, bad=0, at_hit=0, at_pos=0)
    for n, (by, ev) in enumerate(zip(streams, events)):
        r = O.slicer(np.unpackbits(by))
        trace = []
        recs, st = O.run(r["words"], r["k"], stop_short=229, trace=trace)
        got = control.smartnet_osws(recs)
        assert len(got) == len(ev["lid"]) == st["n_frames"], n
        assert [g[1] for g in got] == ev["cmd"].tolist() and [g[3] for g in got] == ev["lid"].tolist(), n
        assert [g[2] for g in got] == ["G" if v else "I" for v in ev["ind"]], n
        assert [g[4] for g in got] == ev["tg"].tolist() and [g[5] for g in got] == ev["status"].tolist(), n
        assert [g[7] for g in got] == [bool(v) for v in ev["is_locked"]], n
        # packets and packets_bad as the reference's quality_check reads them: the running n_frames and n_bad
        assert list(range(1, len(got) + 1)) == ev["packets"].tolist() and np.cumsum([g[6] for g in got]).tolist() == ev["packets_bad"].tolist(), n
        assert st["n_bad"] == (int(ev["packets_bad"][-1]) if len(got) else 0)
        c = O.census(trace)
        seen["rejects"] += c["rejects"]; seen["negative"] += min(c["locked"]) < 0; seen["locked"] += max(c["locked"]) == 5
        seen["bad"] += st["n_bad"]; seen["at_hit"] += c["at_h0"]; seen["at_pos"] += c["at_pos"]
    assert min(seen.values()) > 0, seen


# ------------------------------------------------------------------------------------------------ the header on the host
@pytest.fixture(scope="module")
def check_programs():
    """osw_core.hpp compiled for the host, plain and with the sanitizers: stand-alone programs"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(HERE, "native", "osw_core_check.cpp")
    exes = []
    for name, extra in (("osw_core_check", ["-O2"]), ("osw_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
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


def through_header(exes, tmp_path, words, k, cuts, n_symbols, pos0=0, first_hit=0, word_cap=1 << 20, hit_cap=1 << 20, base_words=0,
                   base_hits=0):
    """the stand-alone programs over the streams, a launch after each cut (a symbol count) -> (records, state, launches)"""
    wp, hp = str(tmp_path / "words.u32"), str(tmp_path / "hits.u32")
    np.asarray(words, "<u4").tofile(wp)
    S.hit_items(k, np.zeros(len(k), np.uint8)).astype("<u4").tofile(hp)
    launches, args, before = [], [], 32 * base_words
    for c in list(cuts) + [n_symbols]:
        launches.append((c // 32, base_hits + int(np.count_nonzero(np.asarray(k) < c))))
        args += [c // 32, launches[-1][1], c, c - before]
        before = c
    lines = lines_of(exes, "stream", wp, hp, first_hit, pos0, word_cap, hit_cap, base_words, base_hits, *args)
    names = lines[0].split()
    st = {("n_" if i < 10 else "") + names[i]: int(names[i + 1]) for i in range(0, 14, 2)}
    recs = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1:]], dtype="<u4").reshape(-1, 8)
    return recs.view(native.OSW_DTYPE).reshape(-1), st, launches


def ragged(n, seed):
    rng = np.random.default_rng(seed)
    return [[], sorted(rng.choice(n, 60).tolist()), list(range(0, n, 7)), [5, 5, 5, 6, n // 2, n // 2, n // 2 + 1]]


def test_golden_streams_through_the_header_under_ragged_cuts(golden, check_programs, tmp_path):
    streams, _ = golden
    total = 0
    for n in range(0, len(streams), 7):
        bits = np.unpackbits(streams[n])
        r = O.slicer(bits)
        want, want_st = O.run(r["words"], r["k"])
        assert want_st["n_frames"] > 0                  # (a stream with 5 % bit errors frames little)
        total += want_st["n_frames"]
        for cuts in ragged(len(bits), n):
            got, st, launches = through_header(check_programs, tmp_path, r["words"], r["k"], cuts, len(bits))
            assert got.tobytes() == want.tobytes() and st == want_st, (n, cuts[:8])
            again, again_st = O.run(r["words"], r["k"], launches=launches)          # the restatement under the same cuts
            assert again.tobytes() == want.tobytes() and again_st == want_st
    assert total > 200


def test_designed_bits_every_single_flip_and_adjacent_pair_and_header_equals_restatement(check_programs, tmp_path):
    """the input of the GPU suite's designed carrier without a device: what it guarantees, and the header on the same stream"""
    bits, sent, starts, patterns = O.designed_bits()
    bits = padded(bits)
    assert sorted(p for p in patterns if len(p) == 1) == [(n,) for n in range(76)]
    assert sorted(p for p in patterns if len(p) == 2) == [(n, n + 1) for n in range(75)]
    r = O.slicer(bits)
    assert (r["k"] - 7).tolist() == starts + [starts[-1] + 84]            # the planted sync words and the last one, nothing else
    trace = []
    want, want_st = O.run(r["words"], r["k"], trace=trace)
    f = native.osw_fields(want)
    frames = [t for t in trace if t["kind"] == "frame"][:len(starts)]
    assert [t["s"] for t in frames] == starts and all(t["locked"] == 5 and t["at_pos"] and not t["rel_nz"] for t in frames[8:])
    corrected, uncorrected = set(), set()
    for n, (rec, m, p) in enumerate(zip(want, sent, patterns)):
        bad, fixed, wrong = O.designed_expect(p)
        assert bool(f["bad"][n]) == bad == (len(p) > 0) and f["flipped"][n] == len(fixed) and f["is_locked"][n] == (n >= 5), (n, p)
        data = np.unpackbits(rec["data"])[:38].tolist()
        was = [int(c) for c in "{0:016b}{1:01b}{2:010b}{3:011b}".format(m[0] ^ 0xcc38, m[1], m[2] ^ 0xd5, m[3])]
        assert {i for i in range(38) if data[i] != was[i]} == wrong, (n, p)
        assert np.unpackbits(rec["data"])[38:].sum() == 0 and np.unpackbits(rec["psyn"])[38:].sum() == 0
        if len(p) == 1:
            o = 4 * (p[0] % 19) + p[0] // 19
            if o % 2 == 0 and o // 2 <= 36:                     # a data bit 0 .. 36: corrected, the message as sent
                assert fixed == {o // 2} and not wrong and control.smartnet_osws(want[n:n + 1])[0][1:4] == (m[2], "G" if m[1] else "I", m[0])
                corrected.add(o // 2)
            else:                                               # data bit 37 and every parity bit: counted bad, nothing corrected
                assert not fixed and wrong == ({37} if o == 74 else set())
                uncorrected.add(o)
    assert corrected == set(range(37)) and uncorrected == {74} | set(range(1, 76, 2))
    assert want_st["n_lost"] == 0 and want_st["n_rejects"] == 0 and want_st["n_bad"] >= 151
    for cuts in ragged(len(bits), 3):
        got, st, _ = through_header(check_programs, tmp_path, r["words"], r["k"], cuts, len(bits))
        assert got.tobytes() == want.tobytes() and st == want_st, cuts[:4]


def test_lock_carrier_census_and_header_equals_restatement(check_programs, tmp_path):
    bits = padded(O.lock_bits()[0])
    r = O.slicer(bits)
    want, want_st = O.lock_census(r["words"], r["k"])
    assert want_st["n_rejects"] >= 8 and want["locked"].min() == -4 and want["locked"].max() == 5
    for cuts in ragged(len(bits), 4):
        got, st, _ = through_header(check_programs, tmp_path, r["words"], r["k"], cuts, len(bits))
        assert got.tobytes() == want.tobytes() and st == want_st, cuts[:4]


def planted_stream(seed, starts, n_each=8):
    """random bits with runs of n_each back-to-back frames planted at the given starts -> (bits, {start: message})"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, starts[-1] + 84 * n_each + 640).astype(np.uint8)
    sent = {}
    for s in starts:
        for n in range(n_each):
            m = O.random_osw(rng)
            bits[s + 84 * n:s + 84 * n + 84] = O.frame(*m)
            sent[s + 84 * n] = m
        bits[s + 84 * n_each:s + 84 * n_each + 8] = O.SYNC_LIST
    return padded(bits), sent


def test_frames_at_every_start_mod_32_through_the_header(check_programs, tmp_path):
    starts = [100 + 1185 * n for n in range(32)]                   # 1185 = 1 mod 32: every start mod 32 once
    assert sorted(s % 32 for s in starts) == list(range(32))
    bits, sent = planted_stream(7, starts)
    r = O.slicer(bits)
    want, want_st = O.run(r["words"], r["k"])
    got, st, _ = through_header(check_programs, tmp_path, r["words"], r["k"], list(range(0, len(bits), 501)), len(bits))
    assert got.tobytes() == want.tobytes() and st == want_st
    msgs = {g[0]: g for g in control.smartnet_osws(want)}
    hit = [s for s, m in sent.items() if s in msgs and msgs[s][1:4] == (m[2], "G" if m[1] else "I", m[0])]
    assert len({s % 32 for s in hit}) == 32 and len(hit) > len(sent) // 2 and want_st["n_lost"] == 0


def test_k_across_the_26_bit_wrap(check_programs, tmp_path):
    starts = [40 + 900 * n for n in range(4)]
    bits, sent = planted_stream(11, starts)
    r = O.slicer(bits)
    base_words, base_hits = ((1 << 26) - 1700) // 32, 5
    k = r["k"] + 32 * base_words
    assert k[0] < (1 << 26) < k[-1]
    want, want_st = O.run(r["words"], k, pos0=32 * base_words, first_hit=base_hits, base_words=base_words, base_hits=base_hits)
    plain, plain_st = O.run(r["words"], r["k"])
    assert plain_st == want_st and (want["k"].astype(np.int64) - 32 * base_words).tolist() == plain["k"].tolist() and want_st["n_frames"] > 16
    for cuts in ([], [32 * base_words + c for c in range(3, len(bits), 97)]):
        got, st, _ = through_header(check_programs, tmp_path, r["words"], k, cuts, 32 * base_words + len(bits), pos0=32 * base_words,
                                    first_hit=base_hits, base_words=base_words, base_hits=base_hits)
        assert got.tobytes() == want.tobytes() and st == want_st
    n = (1 << 26) + 1000
    for true_k in (n - (1 << 26), (1 << 26) - 1, 1 << 26, n - 1):
        item = int(S.hit_items([true_k], [0])[0])
        assert [int(v) for v in lines_of(check_programs, "start", "%x" % item, n)] == [true_k - 7]


def test_both_rings_losses_through_the_header(check_programs, tmp_path):
    bits = padded(O.lock_bits()[0])
    r = O.slicer(bits)
    want, want_st = O.run(r["words"], r["k"])
    # a word ring of 16 words and launches longer than it: lost frames as in the restatement, and decoding goes on afterwards
    got, st, launches = through_header(check_programs, tmp_path, r["words"], r["k"], [900, 3000], len(bits), word_cap=16)
    want_l, want_l_st = O.run(r["words"], r["k"], launches=launches, word_cap=16)
    assert got.tobytes() == want_l.tobytes() and st == want_l_st and st["n_lost"] >= 2 and 0 < st["n_records"] < want_st["n_records"]
    # a hit ring of 16 and a stage attached at hit 2, at the bit behind that hit
    pos0 = int(r["k"][1]) + 1
    got, st, launches = through_header(check_programs, tmp_path, r["words"], r["k"], [2500], len(bits), pos0=pos0, first_hit=2, hit_cap=16)
    want_h, want_h_st = O.run(r["words"], r["k"], pos0=pos0, first_hit=2, launches=launches, hit_cap=16)
    assert got.tobytes() == want_h.tobytes() and st == want_h_st and st["n_lost"] >= 4 and st["n_records"] > 0
    # both at once, under many cuts
    cuts = list(range(0, len(bits), 640))
    got, st, launches = through_header(check_programs, tmp_path, r["words"], r["k"], cuts, len(bits), word_cap=16, hit_cap=16)
    want_b, want_b_st = O.run(r["words"], r["k"], launches=launches, word_cap=16, hit_cap=16)
    assert got.tobytes() == want_b.tobytes() and st == want_b_st and st["n_lost"] >= 1


def test_the_correction_as_one_mask_equals_the_references_sequential_loop(check_programs):
    lines = lines_of(check_programs, "masks", 4000)
    assert len(lines) == 38 * 39 // 2 + 4000
    kinds = set()
    for ln in lines:
        p, m = (int(v, 16) for v in ln.split())
        psyn = [(p >> i) & 1 for i in range(38)]
        fixed = O.correct_sequential([0] * 38, psyn)
        assert m == sum(v << i for i, v in enumerate(fixed)), ln
        assert not (m >> 37)                                       # bit 37 is never corrected
        kinds.add(min(bin(m).count("1"), 3))
    assert kinds == {0, 1, 2, 3}
    # and through the packet rules: psyn from the masks as from the lists
    rng = np.random.default_rng(5)
    for _ in range(200):
        b = rng.integers(0, 2, 76)
        data, psyn = O.psyn_of(b)
        D, P = sum(v << i for i, v in enumerate(data)), sum(int(b[O.out_index(2 * i + 1)]) << i for i in range(38))
        assert (P ^ D ^ (D << 1)) & ((1 << 38) - 1) == sum(v << i for i, v in enumerate(psyn))


def test_smartnet_osws_gives_the_fields_the_reference_publishes():
    m = (0x1234 ^ 0x0005, 1, 0x308, 0x555)
    bits = padded(np.concatenate([O.quiet(40), O.frame(*m), O.frame(0xfff7, 0, 0x2f8), O.SYNC_LIST, O.quiet(120, 2)]))
    r = O.slicer(bits)
    recs, st = O.run(r["words"], r["k"])
    assert control.smartnet_osws(recs) == [(40, 0x308, "G", m[0], m[0] & 0xfff0, m[0] & 0xf, False, False),
                                           (124, 0x2f8, "I", 0xfff7, 0xfff0, 7, False, False)]
    assert st == dict(O.STATE0, n_records=2, n_frames=2, locked=1, n_rejects=1)       # (the last sync word has no follower)
    assert native.osw_fields(recs)["rel"].tolist() == [40, 0] and native.osw_fields(recs)["at_cursor"].tolist() == [0, 1]
    assert recs["locked"].tolist() == [0, 1] and np.unpackbits(recs["data"][0])[27:38].tolist() == [int(c) for c in "{0:011b}".format(0x555)]


# ------------------------------------------------------------------------------------------------ names, constants, sizes
def test_binding_names_constants_and_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RCF_\w+)\s+(-?\d+)", hdr)}
    assert native.HARD_OSW == defs["RCF_HARD_OSW"] == 51 and native.HARD_EDACS == 49 and native.HARD_TSBK == 48
    assert native.T_SLICE == defs["RCF_T_SLICE"] == 13 and defs["RCF_T_COUNT"] == 14
    assert native._read_what("osw", True) == 51 and native._read_what("osw") == native.READ_FM
    assert native._read_dtype("osw") == native.OSW_DTYPE and native.OSW_DTYPE.itemsize == 32
    assert [native.OSW_DTYPE.fields[n][1] for n in ("flags", "k", "lid", "cmd", "data", "psyn", "locked")] == [0, 4, 8, 10, 12, 20, 28]
    assert C.sizeof(native.OswParams) == 16 and C.sizeof(native.OswState) == 48
    assert re.search(r"typedef struct rcf_osw_params \{\s*int capacity;[^}]*int reserved_\[3\];\s*\} rcf_osw_params_t;", hdr)
    assert re.search(r"typedef struct rcf_osw_state \{\s*int64_t n_records, n_frames, n_bad, n_rejects, n_lost;[^}]*int32_t locked, is_locked;[^}]*\} rcf_osw_state_t;", hdr)
    for name in ("rcf_chan_osw", "rcf_chan_osw_state", "rcf_chan_read_osw", "rcf_chan_osw_ring"):
        assert name in native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr)
    for name in ("chan_osw", "chan_osw_state", "chan_read_osw", "chan_osw_ring"):
        assert callable(getattr(native.Frontend, name))
    assert callable(control.smartnet_osws)
    # the readers' second row behind the stream table's eleven: kind 12, records of 8 words, uint32, counted; kReadKinds stays
    # where the first row left it (12) and kAllReadKinds ends the rows; the table itself and stream_kind, which are the pump's as
    # well, stay as they were, so the pump refuses 51 as a stream it does not know; 50 and 52 are no streams at all
    exe = os.path.join(HERE, "native", "_build", "osw_stream_row")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    prog = ('#include <cstdio>\n#include "rcf_streams.h"\nusing namespace rcfx;\nint main() { const int k = read_kind(RCF_HARD_OSW); '
            'const StreamKind &r = read_row(k); printf("%d %d %d %u %d %d %d %d %d %d %d %d %d\\n", k, (int)kReadKinds, (int)kAllReadKinds, r.item_w, (int)r.u32, (int)r.counted, '
            '(int)r.pumped, read_kind(50), read_kind(52), (int)kStreamKinds, stream_kind(RCF_HARD_OSW), read_kind(RCF_HARD_EDACS), read_kind(RCF_HARD_TSBK)); return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-x", "c++", "-", "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc"), "-o", exe],
                   input=prog.encode(), check=True)
    assert subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode().split() == ["12", "12", "13", "8", "1", "1", "0", "-1", "-1", "11", "-1", "11", "10"]
    f = native.osw_fields(np.array([(40000 << 16 | 21 << 10 | 9 << 4 | 8 | 4 | 1, 0, 0, 0, [0] * 8, [0] * 8, -3)], native.OSW_DTYPE))
    assert [int(f[n][0]) for n in ("at_cursor", "bad", "is_locked", "individual", "flipped", "syn_bits", "rel")] == [1, 0, 1, 1, 9, 21, 40000]
