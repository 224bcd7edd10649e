"""The stream table (radiocapture-rf_amd/csrc/rcf_streams.h) compiled alone with g++ (tests/native/stream_table_check.cpp):
every `what` in 0 .. 40 gives the row written out here or a refusal, and the readers' integer rules -- the count transform,
the pump's steady-state bounds, the lag clamp and the host ring's skip -- agree with the model in tests/delivery_ref.py."""
import json
import os
import subprocess

import pytest

import delivery_ref as DR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# include/rcf.h: what -> (item bytes, uint32 items, counted, delivered by the pump)
STREAMS = {
    0: (8, 0, 0, 1),      # RCF_READ_IQ
    1: (4, 0, 0, 1),      # RCF_READ_FM
    2: (8, 0, 0, 1),      # RCF_READ_AGC
    16: (4, 0, 0, 1),     # RCF_READ_SYM
    17: (4, 0, 1, 1),     # RCF_READ_CLOCK
    18: (4, 0, 1, 1),     # RCF_READ_COSTAS
    19: (4, 0, 1, 1),     # RCF_READ_FSK4
    20: (4, 0, 1, 1),     # RCF_READ_AUDIO
    32: (4, 1, 1, 0),     # RCF_HARD_BITS
    33: (4, 1, 1, 0),     # RCF_HARD_SYNC
}
COUNTERS = [0, 1, 24, 25, 26, 999, 12345]
RESAMPLERS = [(1, 1), (8, 25), (48, 25), (441, 1000)]
N_KS = [0, 1, 37, 500, 1200]


@pytest.fixture(scope="module")
def got():
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "stream_table_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc"),
                           os.path.join(HERE, "native", "stream_table_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    return json.loads(p.stdout.decode())


def test_every_what_gives_its_row_or_a_refusal(got):
    rows = got["rows"]
    assert len(rows) == 41
    for what, r in enumerate(rows):
        if what not in STREAMS:
            assert r is None, (what, r)
            continue
        assert r is not None, what
        assert (r["what"], r["item_bytes"], r["u32"], r["counted"], r["pumped"]) == (what,) + STREAMS[what], r
        assert "%d" in r["refusal"] and r["refusal"].count("%") == 1
    kinds = [r["kind"] for r in rows if r is not None]
    assert sorted(kinds) == list(range(10))                       # ten rows, each found by exactly one `what`
    assert [w for w, r in enumerate(rows) if r and r["counted"]] == [17, 18, 19, 20, 32, 33]
    assert [w for w, r in enumerate(rows) if r and not r["pumped"]] == [32, 33]


def test_the_written_out_values_are_the_ten_streams_of_the_abi():
    names = {"RCF_READ_IQ": 0, "RCF_READ_FM": 1, "RCF_READ_AGC": 2, "RCF_READ_SYM": 16, "RCF_READ_CLOCK": 17,
             "RCF_READ_COSTAS": 18, "RCF_READ_FSK4": 19, "RCF_READ_AUDIO": 20, "RCF_HARD_BITS": 32, "RCF_HARD_SYNC": 33}
    text = open(os.path.join(ROOT, "include", "rcf.h")).read()
    for name, value in names.items():
        line = [ln for ln in text.splitlines() if ln.startswith("#define %s " % name)]
        assert len(line) == 1 and int(line[0].split()[2]) == value, name
    assert set(names.values()) == set(STREAMS)


def test_count_transform_and_bounds_agree_with_the_model(got):
    ce = {(c, i, d): e for c, i, d, e in got["count_end"]}
    assert set(ce) == {(c, i, d) for c in COUNTERS for i, d in RESAMPLERS}
    for (c, i, d), e in ce.items():
        assert e == DR.stream_end(c, i, d), (c, i, d)
    sb = {(n, i, d): b for n, i, d, b in got["steady_bound"]}
    assert set(sb) == {(n, i, d) for n in N_KS for i, d in RESAMPLERS}
    for (n, i, d), b in sb.items():
        assert b == DR.audio_bound(n, i, d), (n, i, d)
        if (i, d) == (1, 1):
            assert b == DR.loop_bound(n), n                       # a loop: one symbol per input, and one more


def test_lag_clamp_and_the_host_ring_skip_agree_with_the_model(got):
    rows = got["lag_clamp"]
    assert len(rows) >= 500
    assert {r[2] for r in rows} == set(COUNTERS)
    for cap, cursor, end, mx, cur, n, room, cur2, n2 in rows:
        want_cur, want_n, _, _ = DR.gather(end, 1, 1, cap, mx, None, (cursor, 0))
        assert (cur, n) == (want_cur, want_n), (cap, cursor, end, mx)
        if mx >= cap:                                             # the pump's plain slot: whatever the ring holds, then the skip
            want_cur, want_n, _, _ = DR.gather(end, 1, 1, cap, None, room, (cursor, 0))
            assert (cur2, n2) == (want_cur, want_n), (cap, cursor, end, room)
