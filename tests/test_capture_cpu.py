"""The carrier-operated capture (rcf_chan_capture) without a GPU: the kernel's per-sample header
(radiocapture-rf_amd/csrc/capture_core.hpp) compiled for the host -- plain, and once more under AddressSanitizer and UBSan, as
a stand-alone program -- and walked, in random pieces, over designed and random streams; keep, the captured samples, every
record field and the state after every piece equal the numpy restatement's (tests/capture_ref.py) bit for bit.  The designed
streams demand every way a window can begin and end, and a census on the restatement's output fails on a missing case.
Then the binding's names, constants and sizes, and the stream table's two new rows."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import capture_ref as R
import squelch_ref
from rcf import native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EDGE = (0, 1, 63, 64, 65)


@pytest.fixture(scope="module")
def check_programs():
    """capture_core.hpp compiled for the host, plain and with the sanitizers: stand-alone programs"""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(HERE, "native", "capture_core_check.cpp")
    exes = []
    for name, extra in (("capture_core_check", ["-O2"]),
                        ("capture_core_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(out, name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-ffp-contract=off"] + extra
                              + [src, "-o", exe])
        exes.append(exe)
    return exes


def random_pieces(rng, n, pre):
    """piece sizes that sum to n: zeros, ones, pieces shorter than pre, and longer ones"""
    sizes, left = [], n
    while left > 0:
        kind = rng.integers(0, 5)
        s = 0 if kind == 0 else 1 if kind == 1 else int(rng.integers(0, max(pre, 2))) if kind == 2 else int(rng.integers(1, 200))
        s = min(s, left)
        sizes.append(s)
        left -= s
    return sizes + [0]


def walk(exes, tmp_path, cases):
    """cases: dicts(x, thr_db, alpha, a, pre, hang, pieces) -> per case the pieces' parsed output (events, kept, state); the
    plain and the sanitized program must print the same"""
    path, cpath = os.path.join(str(tmp_path), "x.cf32"), os.path.join(str(tmp_path), "cases.txt")
    np.concatenate([np.asarray(c["x"], np.complex64) for c in cases]).tofile(path)
    off, lines = 0, []
    for c in cases:
        lines.append(" ".join([str(off), str(len(c["x"])), float(c["thr_db"]).hex(), float(c["alpha"]).hex(), str(c["a"]), str(c["pre"]),
                               str(c["hang"])] + [str(p) for p in c["pieces"]]))
        off += len(c["x"])
    with open(cpath, "w") as f:
        f.write("\n".join(lines) + "\n")
    outs = [subprocess.check_output([exe, path, cpath], text=True) for exe in exes]
    assert outs[0] == outs[1]
    res = []
    for line in outs[0].splitlines():
        f = line.split()
        if f[0] == "CASE":
            res.append([])
            cur = dict(recs=[], kept=[])
        elif f[0] == "R":
            cur["recs"].append((int(f[1]), int(f[2]), int(f[3]), int(f[4]), np.float32(float.fromhex(f[5])), 0))
        elif f[0] == "K":
            cur["kept"].append((int(f[1]), int(f[2]), int(f[3])))
        else:
            cur["state"] = dict(level=float.fromhex(f[1]), n_seen=int(f[2]), n_decided=int(f[3]), n_kept=int(f[4]), n_records=int(f[5]),
                                n_windows=int(f[6]), last_open=int(f[7]), in_window=int(f[8]), unmuted=int(f[9]))
            res[-1].append(cur)
            cur = dict(recs=[], kept=[])
    assert len(res) == len(cases) and all(len(r) == len(c["pieces"]) for r, c in zip(res, cases))
    return res


def same_float(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def hold(case, got):
    """the program's output of one case against the restatement, piece by piece: what each piece added and the state behind it"""
    x, a = np.asarray(case["x"], np.complex64), case["a"]
    cuts = np.cumsum(case["pieces"])
    refs = R.prefixes(x, squelch_ref.threshold(case["thr_db"]), case["alpha"], case["pre"], case["hang"], cuts, a)
    n_rec = n_dec = 0
    bits = x.view(np.uint32).reshape(-1, 2)
    for ref, g in zip(refs, got):
        st = dict(ref["state"])
        assert same_float(g["state"].pop("level"), st.pop("level"))
        assert g["state"] == st
        new = ref["records"][n_rec:]
        assert len(g["recs"]) == len(new)
        assert np.array(g["recs"], R.REC_DTYPE).tobytes() == new.tobytes() if len(new) else True
        kept_idx = np.flatnonzero(ref["keep"][n_dec:]) + n_dec
        assert [k[0] for k in g["kept"]] == [int(a + i) for i in kept_idx]            # keep, sample by sample
        assert [(k[1], k[2]) for k in g["kept"]] == [tuple(int(v) for v in bits[i]) for i in kept_idx]     # unchanged bits
        n_rec, n_dec = len(ref["records"]), ref["state"]["n_decided"]
    assert R.records_ok(refs[-1]["records"], a)
    return refs[-1]


# ------------------------------------------------------------------------------------------------ designed streams
def designed(pre, hang):
    """power sequences with alpha = 1 and threshold 0 dB (thr = 1): the level IS the input, so the open pattern is the design
    (power 4: open, 0: muted).  -> {name: (power array or complex array, alpha)}"""
    W = pre + hang
    n = 3 * W + 400

    def seq(open_idx, n=n):
        p = np.zeros(n, np.complex64)
        p[list(open_idx)] = 2.0
        return p
    g0 = 100
    out = {
        "single": (seq([g0 + W]), 1.0),
        "gap_merge": (seq(list(range(g0, g0 + 5)) + list(range(g0 + 5 + W, g0 + 9 + W))), 1.0),          # gap exactly pre + hang
        "gap_split": (seq(list(range(g0, g0 + 5)) + list(range(g0 + 6 + W, g0 + 9 + W))), 1.0),          # gap pre + hang + 1
        "clipped": (seq([pre // 2, pre // 2 + 1]), 1.0),                       # an opening inside the first pre samples
        "open_at_a": (seq([0]), 1.0),
        "ends_in_window": (seq(range(n - pre - 3, n)), 1.0),
        "ends_in_pre_tail": (seq([n - 1 - pre // 2]), 1.0),
        "never": (seq([]), 1.0),
        "always": (seq(range(n)), 1.0),
    }
    nan = seq(list(range(g0, g0 + 5)) + list(range(g0 + W + 40, n)))
    nan[g0 + W + 20] = np.float32("nan")                                   # the window of the first burst has closed by then
    out["nan"] = (nan, 0.5)
    inf = seq([])
    inf[g0] = np.float32("inf")
    out["inf"] = (inf, 0.5)
    return out


def designed_census(name, r, pre, hang, n):
    """what the restatement's output of a designed stream must show: the case is there"""
    c, st, W = R.census(r, pre, hang), r["state"], pre + hang
    w = c["windows"]
    if name == "single":
        return w == [(100 + hang, 100 + W + hang + 1)] and r["records"][1]["n_open"] == 1 and st["n_kept"] == W + 1
    if name == "gap_merge":
        return len(w) == 1 and w[0][1] is not None and r["records"][1]["n_open"] == 9 and st["n_kept"] == 9 + 2 * W
    if name == "gap_split":
        return len(w) == 2 and c["one_sample_gaps"] == 1 and r["records"][1]["n_open"] == 5 and r["records"][3]["n_open"] == 3
    if name == "clipped":
        return w[0][0] == 0 and w[0][1] == pre // 2 + 2 + hang and (pre == 0 or st["n_kept"] < W + 2)
    if name == "open_at_a":
        return w == [(0, hang + 1)] and st["n_kept"] == hang + 1
    if name == "ends_in_window":
        return len(w) == 1 and w[0][1] is None and st["in_window"] == 1 and st["n_records"] == 1 and st["unmuted"] == 1
    if name == "ends_in_pre_tail":      # the open sample itself is not decided yet (pre > 0); its lead-in may have begun
        return st["last_open"] == n - 1 - pre // 2 and st["n_decided"] == n - pre and (pre < 2 or st["last_open"] >= st["n_decided"])
    if name == "never":
        return w == [] and st["n_kept"] == 0 and st["last_open"] == -1
    if name == "always":
        return w == [(0, None)] and st["n_kept"] == n - pre and st["in_window"] == 1
    if name == "nan":                   # muted for good behind the NaN; the earlier window closed normally (alpha 0.5: the
        # level after the burst of five is 3.875, then 1.9375 -- one more open sample -- and 0.97)
        return w == [(100 - pre, 106 + hang)] and np.isnan(st["level"]) and st["unmuted"] == 0 and r["records"][1]["n_open"] == 6
    if name == "inf":
        return w == [(100 - pre, None)] and np.isinf(st["level"]) and st["unmuted"] == 1 and st["in_window"] == 1
    return False


@pytest.mark.parametrize("pre", EDGE)
def test_designed_windows_equal_the_restatement(check_programs, tmp_path, pre):
    rng = np.random.default_rng(100 + pre)
    cases, names = [], []
    for hang in EDGE:
        for name, (x, alpha) in designed(pre, hang).items():
            for a in (0, 12345):
                cases.append(dict(x=x, thr_db=0.0, alpha=alpha, a=a, pre=pre, hang=hang, pieces=random_pieces(rng, len(x), pre)))
                names.append((name, hang, a))
    got = walk(check_programs, tmp_path, cases)
    seen = set()
    for case, g, (name, hang, a) in zip(cases, got, names):
        last = hold(case, g)
        if a == 0:
            assert designed_census(name, last, pre, hang, len(case["x"])), (name, pre, hang, R.census(last, pre, hang), last["state"])
            seen.add((name, hang))
    assert seen == {(n, h) for h in EDGE for n in ("single", "gap_merge", "gap_split", "clipped", "open_at_a", "ends_in_window",
                                                    "ends_in_pre_tail", "never", "always", "nan", "inf")}


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.1, 0.01])
def test_random_streams_equal_the_restatement(check_programs, tmp_path, alpha):
    rng = np.random.default_rng(int(alpha * 1000))
    thr_db = -30.0
    thr = squelch_ref.threshold(thr_db)
    cases = []
    for k in range(12):
        n = int(rng.integers(300, 1500))
        on, at = [], 0
        while at < n:                                   # keyings of random length and spacing, some closer than pre + hang
            at += int(rng.integers(1, 150))
            ln = int(rng.integers(1, 120))
            on.append((at, min(n, at + ln)))
            at += ln
        x = squelch_ref.keyed_noise(rng, n, on, amp_on=np.sqrt(100 * thr), amp_off=np.sqrt(thr / 100), noise=np.sqrt(thr) * 0.3)
        pre, hang = (int(v) for v in rng.choice([0, 1, 5, 63, 64, 65, 200], 2))
        cases.append(dict(x=x, thr_db=thr_db, alpha=alpha, a=int(rng.integers(0, 1 << 40)) if k % 2 else 0, pre=pre, hang=hang,
                          pieces=random_pieces(rng, n, pre)))
    got = walk(check_programs, tmp_path, cases)
    n_windows = 0
    for case, g in zip(cases, got):
        n_windows += hold(case, g)["state"]["n_windows"]
    assert n_windows >= len(cases)                         # (a window per stream on average: with alpha 0.01 the level is slow)


def test_restatement_is_the_definition_by_brute_force():
    """capture_ref's cumulative-count form against the definition read literally (a double loop), on a small stream"""
    rng = np.random.default_rng(5)
    is_open = rng.random(120) < 0.08
    x = (is_open * 2.0).astype(np.complex64)
    for pre, hang in ((0, 0), (3, 0), (0, 4), (5, 7)):
        r = R.run(x, 1.0, 1.0, pre, hang, a=50)
        want = [any(is_open[i] for i in range(max(j - hang, 0), j + pre + 1)) for j in range(len(x) - pre)]
        assert list(r["keep"]) == want
        assert R.records_ok(r["records"], 50)
        w = R.census(r, pre, hang)["windows"]
        for i in np.flatnonzero(is_open):                   # every open sample lies in exactly one window
            assert sum(1 for lo, hi in w if lo <= 50 + i and (hi is None or 50 + i < hi)) == 1
        for k, (lo, hi) in enumerate(w):                    # and a CLOSE counts its window's open samples
            if hi is not None:
                assert r["records"][2 * k + 1]["n_open"] == is_open[lo - 50:hi - 50].sum()


# ------------------------------------------------------------------------------------------------ names, constants, sizes
def test_binding_names_constants_and_struct_sizes():
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RCF_\w+)\s+(-?\d+)", hdr)}
    # (the two stream numbers are enumerators: the header says why)
    defs.update({m.group(1): int(m.group(2)) for m in re.finditer(r"^\s+(RCF_(?:READ|HARD)_CAPTURE) = (\d+),?\s", hdr, re.M)})
    assert native.READ_CAPTURE == defs["RCF_READ_CAPTURE"] == 24 and native.HARD_CAPTURE == defs["RCF_HARD_CAPTURE"] == 56
    assert native.CAPTURE_OPEN == defs["RCF_CAPTURE_OPEN"] == R.OPEN == 1 and native.CAPTURE_CLOSE == defs["RCF_CAPTURE_CLOSE"] == R.CLOSE == 2
    assert defs["RCF_T_COUNT"] == 14
    assert native._read_what("capture", True) == 24 and native._read_what("capture_rec", True) == 56
    assert native._read_dtype("capture") == np.complex64 and native._read_dtype("capture_rec") == native.CAPTURE_REC_DTYPE
    assert native.CAPTURE_REC_DTYPE == R.REC_DTYPE and native.CAPTURE_REC_DTYPE.itemsize == 32
    assert [native.CAPTURE_REC_DTYPE.fields[n][1] for n in ("kind", "n_open", "sample", "pos", "peak", "reserved_")] == [0, 4, 8, 16, 24, 28]
    assert C.sizeof(native.CaptureParams) == 40 and C.sizeof(native.CaptureState) == 64
    assert [getattr(native.CaptureParams, n).offset for n in ("threshold_db", "alpha", "pre", "hang", "capacity", "rec_capacity")] == [0, 8, 16, 24, 32, 36]
    assert re.search(r"typedef struct rcf_capture_params \{\s*double threshold_db;[^}]*double alpha;[^}]*int64_t pre;[^}]*int64_t hang;[^}]*"
                     r"uint32_t capacity;[^}]*uint32_t rec_capacity;[^}]*\} rcf_capture_params_t;", hdr)
    assert re.search(r"typedef struct rcf_capture_rec \{\s*uint32_t kind;[^}]*uint32_t n_open;[^}]*int64_t sample;[^}]*int64_t pos;[^}]*float peak;[^}]*"
                     r"uint32_t reserved_;[^}]*\} rcf_capture_rec_t;", hdr)
    assert re.search(r"typedef struct rcf_capture_state \{\s*double level;[^}]*int64_t n_seen;[^}]*int64_t n_decided;[^}]*int64_t n_kept;[^}]*"
                     r"int64_t n_records;[^}]*int64_t n_windows;[^}]*int64_t last_open;[^}]*int32_t in_window;[^}]*int32_t unmuted;[^}]*\} rcf_capture_state_t;", hdr)
    assert [n for n, _ in native.CaptureState._fields_] == ["level", "n_seen", "n_decided", "n_kept", "n_records", "n_windows", "last_open",
                                                            "in_window", "unmuted"]
    for name in ("rcf_chan_capture", "rcf_chan_capture_state", "rcf_chan_read_capture", "rcf_chan_read_capture_rec", "rcf_chan_capture_rings"):
        assert name in native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr)
        assert hasattr(native.lib(), name)
    for name in ("chan_capture", "chan_capture_state", "chan_read_capture", "chan_read_capture_rec", "chan_capture_rings"):
        assert callable(getattr(native.Frontend, name))


def test_stream_table_rows_and_bounds():
    """the two rows behind the readers' rows: kinds 14 and 15, cf32 counted and pumped / records of 8 uint32 counted; the
    pinned ends stay, 21, 50 and 52 are still no streams, the table that rcf_pump_start reads knows neither number, and
    read_kind -- which the suite pins over 0 .. 60 -- does not either: the readers find the two rows through row_kind"""
    exe = os.path.join(HERE, "native", "_build", "capture_stream_rows")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    prog = ('#include <cstdio>\n#include "rcf_streams.h"\nusing namespace rcfx;\nint main() { const int k = row_kind(RCF_READ_CAPTURE), q = row_kind(RCF_HARD_CAPTURE); '
            'const StreamKind &r = read_row(k), &s = read_row(q); printf("%d %d %d %d %d %d %d\\n", k, q, (int)kStreamKinds, (int)kReadKinds, (int)kAllReadKinds, '
            '(int)kReadKindsEnd, (int)kReadRowsEnd); printf("%u %d %d %d %u %d %d %d\\n", r.item_w, (int)r.u32, (int)r.counted, (int)r.pumped, s.item_w, (int)s.u32, '
            '(int)s.counted, (int)s.pumped); printf("%d %d %d %d %d %d %d %d %d\\n", row_kind(21), row_kind(50), '
            'row_kind(52), row_kind(-1), stream_kind(24), stream_kind(56), row_kind(RCF_HARD_P25LC), read_kind(24), read_kind(56)); '
            'for (int w = 3; w <= 15; ++w) if (row_kind(w) != -1 || read_kind(w) != -1) printf("bad %d\\n", w); '
            'if (read_kind(21) != -1 || read_kind(50) != -1 || read_kind(52) != -1 || row_kind(34) != -1) printf("bad\\n"); '
            'printf("%lld %lld %lld %lld %lld %lld %lld\\n", (long long)capture_bound(1000), (long long)capture_rec_bound(1000, 0, 0), '
            '(long long)capture_rec_bound(1000, 200, 300), (long long)capture_rec_bound(0, 5, 5), (long long)hard_bound(k, 10, 1), (long long)hard_bound(q, 10, 1), '
            '(long long)slot_items(q, 4096)); return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-x", "c++", "-", "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc"), "-o", exe],
                   input=prog.encode(), check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert out[0].split() == ["14", "15", "11", "12", "13", "14", "16"]
    assert out[1].split() == ["2", "0", "1", "1", "8", "1", "1", "0"]
    assert out[2].split() == ["-1", "-1", "-1", "-1", "-1", "-1", "13", "-1", "-1"]
    assert len(out) == 4 and out[3].split() == ["1000", "1004", "6", "4", "-1", "-1", "1024"]


def test_record_bound_holds_on_the_densest_keying():
    """capture_rec_bound's derivation (rcf_streams.h) on the restatement: two records cost pre + hang + 2 samples -- a keying of
    one open sample every pre + hang + 2 -- and no run of n_k decided samples holds more records than the bound"""
    for pre, hang in ((0, 0), (1, 1), (3, 4), (0, 5)):
        period = pre + hang + 2
        is_open = np.zeros(40 * period + 50, bool)
        is_open[pre::period] = True
        is_open[1] = True                                   # and a window whose lead-in is clipped in front
        r = R.run((is_open * 2.0).astype(np.complex64), 1.0, 1.0, pre, hang)
        ev = np.sort(np.array([q["sample"] for q in r["records"]]))
        for n_k in (1, 2, period, period + 1, 3 * period, 10 * period + 1):
            most = max(int(np.searchsorted(ev, s + n_k) - np.searchsorted(ev, s)) for s in range(len(is_open)))
            assert most <= 2 * (n_k // period) + 4
            if n_k % period == 0 and n_k >= period:
                assert most >= 2 * (n_k // period)          # (the bound is tight up to its constant)
