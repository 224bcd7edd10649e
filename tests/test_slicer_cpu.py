"""The hard-decision stage (rcf_chan_slicer) without a GPU: the numpy restatement (tests/slicer_ref.py) against the
project's own host slicers, its invariance under cuts, the P25 frame sync planted in a dibit stream, the 26-bit widening of a
hit's k, the kernel's arithmetic header (radiocapture-rf_amd/csrc/slice_core.hpp) compiled for the host and walked over the
same streams -- once more under AddressSanitizer and UBSan --, and the binding's names."""
import os
import re
import subprocess

import numpy as np
import pytest

import slicer_ref as S
from rcf import control, native, p25

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P25_SYNC, P25_BITS = 0x5575F5FF77FF, 48


def soft_stream(seed, n, special=True):
    """soft symbols that spread over all four dibits, with NaN, +-Inf and values exactly on a level mixed in"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-4.5, 4.5, n).astype(np.float32)
    if special:
        at = rng.choice(n, size=min(n, 40), replace=False)
        s[at] = np.resize(np.array([np.nan, np.inf, -np.inf, -2.0, 0.0, 2.0, 4.0, -0.0], np.float32), len(at))
    return s


def dibits_to_soft(d):
    """a soft symbol in the middle of dibit d's interval: 0 -> 1, 1 -> 3, 2 -> -1, 3 -> -3"""
    return np.array([1.0, 3.0, -1.0, -3.0], np.float32)[np.asarray(d)]


def word_dibits(word, bits):
    return [(word >> (bits - 2 - 2 * i)) & 3 for i in range(bits // 2)]


def test_binary_restatement_is_pack_bits():
    s = soft_stream(1, 4001)
    r = S.run(s, S.BINARY)
    by, carry = control.pack_bits(s)
    assert len(r["bytes"]) == len(s) // 32 * 4
    assert np.array_equal(r["bytes"], by[:len(r["bytes"])])
    assert np.array_equal(r["words"].view(np.uint8), r["bytes"])
    assert S.decisions(np.array([np.nan, -0.0, 0.0, -1e-30, np.inf, -np.inf], np.float32), S.BINARY).tolist() == [0, 1, 1, 0, 1, 0]


def test_fsk4_restatement_is_slice_dibits_packed():
    s = soft_stream(2, 4003)
    d = p25.slice_dibits(s)
    assert np.array_equal(S.decisions(s, S.FSK4), d)
    edge = np.array([np.nan, np.inf, -np.inf, -2.0, 0.0, 2.0, 4.0, np.nextafter(np.float32(-2), np.float32(-3))], np.float32)
    assert S.decisions(edge, S.FSK4).tolist() == [1, 1, 3, 2, 0, 1, 1, 3]
    bits = np.stack([(d >> 1) & 1, d & 1], axis=1).reshape(-1)
    r = S.run(s, S.FSK4)
    assert len(r["bytes"]) == len(s) // 16 * 4
    assert np.array_equal(r["bytes"], np.packbits(bits)[:len(r["bytes"])])


@pytest.mark.parametrize("mode,word,bits,err", [(S.BINARY, 0b10101100, 8, 2), (S.FSK4, P25_SYNC, P25_BITS, 16), (S.BINARY, 0xF0F0F0F0F0F0F0F1, 64, 24)])
def test_any_cuts_give_the_same_words_and_hits(mode, word, bits, err):
    s = soft_stream(3, 1500)
    whole = S.run(s, mode, sync_word=word, sync_bits=bits, max_errors=err)
    assert len(whole["k"]) > 3                                   # loose enough to hit on random bits
    rng = np.random.default_rng(4)
    for cuts in ([1], [5, 5, 6, 70], list(range(7, 1500, 13)), sorted(rng.choice(1500, 40).tolist()), [64, 128, 1472]):
        r = S.run(s, mode, sync_word=word, sync_bits=bits, max_errors=err, cuts=cuts)
        assert np.array_equal(r["words"], whole["words"]) and np.array_equal(r["k"], whole["k"]) and np.array_equal(r["dist"], whole["dist"])
    assert np.all(np.diff(whole["k"]) > 0) and whole["k"][0] >= bits // (1 if mode == S.BINARY else 2) - 1


def planted_stream(seed=11):
    """random dibits with the P25 word planted at dibit offsets 0 .. 3 mod 4, with 0, 1, 4 and 5 flipped bits each
    -> (dibits, {last dibit of a planted word: flipped bits})"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 4, 3000).astype(np.uint8)
    sync = np.array(word_dibits(P25_SYNC, P25_BITS), np.uint8)
    ends, at = {}, 100
    for flips in (0, 1, 4, 5):
        for off in range(4):
            start = at + (off - at) % 4
            w = sync.copy()
            for b in rng.choice(P25_BITS, flips, replace=False):
                w[b // 2] ^= 2 >> (b % 2)
            d[start:start + 24] = w
            ends[start + 23] = flips
            at = start + 120
    return d, ends


def test_planted_p25_sync_hits_exactly_where_planted():
    d, ends = planted_stream()
    r = S.run(dibits_to_soft(d), S.FSK4, sync_word=P25_SYNC, sync_bits=P25_BITS, max_errors=4)
    want = {k: f for k, f in ends.items() if f <= 4}
    assert len(want) == 12 and sorted(k % 4 for k in want) == sorted([3, 0, 1, 2] * 3)
    assert dict(zip(r["k"].tolist(), r["dist"].tolist())) == want          # no hit for 5 flips, none in the random payload
    assert len(r["k"]) == len(want)
    # a frame-aligned stream shows the word's bytes as they stand
    k0 = min(k for k, f in want.items() if f == 0 and (k - 23) % 4 == 0)
    assert r["bytes"][(k0 - 23) // 4:(k0 - 23) // 4 + 6].tobytes() == bytes.fromhex("5575f5ff77ff")


def test_hit_k_widens_across_a_wrap():
    assert np.array_equal(S.hit_items([5, (1 << 26) + 5], [0, 3]), np.array([5, (3 << 26) | 5], np.uint32))
    n = (1 << 26) + 1000
    true_k = np.array([n - 1 - (1 << 26) + 1, (1 << 26) - 1, 1 << 26, n - 1], np.int64)      # the oldest a ring of 2^26 could hold .. the newest
    k, dist = native.widen_hits(S.hit_items(true_k, [0, 1, 2, 63]), n)
    assert np.array_equal(k, true_k) and dist.tolist() == [0, 1, 2, 63]
    k, _ = native.widen_hits(S.hit_items([0, 77], [0, 0]), 78)
    assert k.tolist() == [0, 77]
    k, _ = native.widen_hits(S.hit_items([3 * (1 << 26) + 9], [0]), 3 * (1 << 26) + 10)
    assert k.tolist() == [3 * (1 << 26) + 9]


def fnv(words, hits):
    h = 0xcbf29ce484222325
    for b in np.asarray(words, "<u4").tobytes() + np.asarray(hits, "<u4").tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.fixture(scope="module")
def check_programs():
    """slice_core.hpp compiled for the host, plain and with the sanitizers: stand-alone programs"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(HERE, "native", "slice_core_check.cpp")
    exes = []
    for name, extra in (("slice_core_check", ["-O2"]), ("slice_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(out, name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"] + extra + [src, "-o", exe])
        exes.append(exe)
    return exes


CASES = [(1, 0b10101100, 8, 2), (1, 0x555557125555, 48, 12), (1, 0xF0F0F0F0F0F0F0F1, 64, 24), (1, 0, 0, 0),
         (2, P25_SYNC, P25_BITS, 14), (2, 0x2D, 8, 1), (2, 0x0123456789ABCDEF, 64, 22)]


@pytest.mark.parametrize("bps,word,bits,err", CASES)
def test_kernel_header_on_the_host_equals_the_restatement(check_programs, tmp_path, bps, word, bits, err):
    rng = np.random.default_rng(100 + bits + bps)
    for trial, n in enumerate((1, 31, 64, 777, 5000)):
        s = soft_stream(200 + trial, n)
        path = str(tmp_path / ("soft%d.f32" % trial))
        s.tofile(path)
        r = S.run(s, bps, sync_word=word, sync_bits=bits, max_errors=err)
        want = "symbols %d words %d hits %d digest %016x" % (n, len(r["words"]), len(r["k"]), fnv(r["words"], S.hit_items(r["k"], r["dist"])))
        ragged = sorted(rng.choice(n + 1, min(n, 60)).tolist())              # blocks of 0 symbols, blocks that end inside a word
        for cuts in ([], ragged, list(range(0, n, 3))[:400]):
            for exe in check_programs:
                p = subprocess.run([exe, path, str(bps), "%x" % word, str(bits), str(err)] + [str(c) for c in cuts],
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
                assert p.returncode == 0 and p.stdout.decode().strip() == want, (exe, cuts[:8], p.stdout.decode(), want)


def test_planted_stream_through_the_header(check_programs, tmp_path):
    d, ends = planted_stream()
    path = str(tmp_path / "planted.f32")
    dibits_to_soft(d).tofile(path)
    r = S.run(dibits_to_soft(d), S.FSK4, sync_word=P25_SYNC, sync_bits=P25_BITS, max_errors=4)
    want = "symbols %d words %d hits 12 digest %016x" % (len(d), len(r["words"]), fnv(r["words"], S.hit_items(r["k"], r["dist"])))
    for exe in check_programs:
        out = subprocess.run([exe, path, "2", "%x" % P25_SYNC, "48", "4", "100", "117", "1000"], stdout=subprocess.PIPE, timeout=60).stdout.decode().strip()
        assert out == want


def test_binding_names_and_constants():
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RCF_\w+)\s+(-?\d+)", hdr)}
    assert (native.HARD_BITS, native.HARD_SYNC) == (defs["RCF_HARD_BITS"], defs["RCF_HARD_SYNC"]) == (32, 33)
    assert (native.SLICE_BINARY, native.SLICE_FSK4) == (defs["RCF_SLICE_BINARY"], defs["RCF_SLICE_FSK4"]) == (1, 2)
    assert native.T_SLICE == defs["RCF_T_SLICE"] == 13 and defs["RCF_T_COUNT"] == 14
    assert native._read_what("hard", True) == 32 and native._read_what("sync", True) == 33
    assert native._read_what("bits", True) == native.READ_FM                    # still the discriminator
    assert native._read_what("hard") == native._read_what("sync") == native.READ_FM   # the one-argument form answers as it always has
    assert native._read_dtype("hard") == native._read_dtype("sync") == np.uint32
    import ctypes as C
    assert C.sizeof(native.SlicerParams) == 48 and native.SlicerParams.sync_word.offset == 24
    assert C.sizeof(native.SlicerState) == 24
    assert p25.FRAME_SYNC == P25_SYNC and control.SMARTNET_SYNC == 0b10101100
    assert control.EDACS_SYNC == int("010101010101010101010111000100100101010101010101", 2)
    for name in ("rcf_chan_slicer", "rcf_chan_slicer_state", "rcf_chan_read_hard", "rcf_chan_read_sync", "rcf_chan_slicer_rings"):
        assert name in native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr)
