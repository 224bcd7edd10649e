"""The binding's names for the stages' streams (RCF_READ_SYM .. RCF_READ_AUDIO) without a GPU: the constants, the mapping
every reader of rcf.native uses, the item types -- and that "iq" / "fm" / "agc" map as they always did."""
import re

import numpy as np

from rcf import native


def test_read_constants_are_the_headers():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rcf.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define RCF_READ_(\w+)\s+(\d+)", hdr)}
    assert vals == {"IQ": 0, "FM": 1, "AGC": 2, "SYM": 16, "CLOCK": 17, "COSTAS": 18, "FSK4": 19, "AUDIO": 20}
    for name, v in vals.items():
        assert getattr(native, "READ_" + name) == v


def test_stage_names_map_to_their_streams_and_the_old_three_are_unchanged():
    want = {"sym": native.READ_SYM, "clock": native.READ_CLOCK, "costas": native.READ_COSTAS, "fsk4": native.READ_FSK4,
            "audio": native.READ_AUDIO}
    for name, v in want.items():
        assert native._read_what(name, True) == v
        assert native._read_dtype(name) == np.float32
    for stages in (False, True):
        assert native._read_what("iq", stages) == native.READ_IQ == 0
        assert native._read_what("fm", stages) == native.READ_FM == 1
        assert native._read_what("agc", stages) == native.READ_AGC == 2
        for other in ("FM", None, "bits"):                     # anything unknown stays the discriminator
            assert native._read_what(other, stages) == native.READ_FM
    assert native._read_what("iq") == native.READ_IQ and native._read_what("agc") == native.READ_AGC
    for name in list(want) + ["fm"]:                           # the one-argument form answers as it always has
        assert native._read_what(name) == native.READ_FM
    assert native._read_dtype("iq") == native._read_dtype("agc") == np.complex64
    assert native._read_dtype("fm") == np.float32
    assert len(set(want.values()) | {0, 1, 2}) == 8 and min(want.values()) >= 16   # 3 .. 15 are nobody's


# ---------------------------------------------------------------- the counted gather's rule (tests/delivery_ref.py)
def _blocks(per_block):
    return [int(v) for v in np.cumsum(per_block)]


def test_model_unbounded_replay_before_the_ring_wraps_is_the_stream():
    import delivery_ref as R
    per_block = [96, 7, 0, 1, 230, 96]
    counters = _blocks(per_block)
    stream = list(range(1000, 1000 + counters[-1]))
    big = 1 << 20
    idx, items, per, written = R.replay_slot(stream, counters, [big] * len(counters), cap=1 << 12, room=big)
    assert idx == list(range(counters[-1])) and items == stream and written == counters[-1]
    assert [n for _, n in per] == per_block
    # the steady-state bound n_k + 1 holds what a block of n_k inputs makes, and a linear row takes positions pos, pos + 1, ...
    idx2, _, _, written2 = R.replay_slot(stream, counters, [R.loop_bound(n) for n in per_block], cap=1 << 12, room=1 << 12)
    assert idx2 == idx and written2 == written
    cur, n, positions, state = R.gather(50, 1, 1, 1 << 12, None, None, (20, 3))
    assert (cur, n, positions, state) == (20, 30, list(range(3, 33)), (50, 33))


def test_model_small_room_takes_each_blocks_newest_items():
    import delivery_ref as R
    per_block = [96, 97, 160, 70, 96]
    counters = _blocks(per_block)
    stream = list(range(counters[-1]))
    room = 64
    idx, items, per, written = R.replay_slot(stream, counters, [R.loop_bound(n) for n in per_block], cap=1 << 12, room=room)
    assert written == room * len(per_block) and len(idx) == written
    for b, (cur, n) in enumerate(per):
        assert (cur, n) == (counters[b] - room, room)          # exactly the block's newest `room`
    # consecutive slot positions: block b's items sit at written .. written + 63 modulo the ring
    state = (0, 0)
    for b, c in enumerate(counters):
        _, n, positions, state = R.gather(c, 1, 1, 1 << 12, room, room, state)
        assert positions == [(b * room + i) % room for i in range(n)] and state == (c, (b + 1) * room)
    # a bound below the room leaves a rest for the next block instead of skipping it
    cur, n, _, state = R.gather(60, 1, 1, 1 << 12, 40, 64, (0, 0))
    assert (cur, n, state) == (0, 40, (40, 40))
    cur, n, _, state = R.gather(70, 1, 1, 1 << 12, 40, 64, state)
    assert (cur, n, state) == (40, 30, (70, 70))


def test_model_a_reader_more_than_a_ring_behind_gets_the_newest_ring():
    import delivery_ref as R
    cap = 256
    cur, n, positions, state = R.gather(1000, 1, 1, cap, None, None, (10, 0))
    assert (cur, n, state) == (1000 - cap, cap, (1000, cap)) and positions == list(range(cap))
    # a subscription on a wrapped ring: the first gather is bounded by the device ring, then the stream goes on whole
    counters = _blocks([96] * 9)
    stream = list(range(counters[-1]))
    idx, _, per, written = R.replay_slot(stream, counters, [97] * 9, cap=cap, room=4096, first=6)
    assert per[0] == (counters[6] - cap, cap) and idx == list(range(counters[6] - cap, counters[-1]))
    assert written == len(idx) and idx[0] > 0
    # a reader that stood part-way and a ring that still holds it: from the reader on
    idx, _, _, written = R.replay_slot(stream, counters, [97] * 9, cap=4096, room=4096, first=2, cursor0=50)
    assert idx == list(range(50, counters[-1])) and written == counters[-1] - 50


def test_model_count_transform():
    import delivery_ref as R
    for counter in (0, 1, 24, 25, 26, 999, 12345):
        assert R.stream_end(counter, 1, 1) == R.stream_end(counter, 7, 7) == counter       # the branch of its own
        assert R.stream_end(counter, 8, 25) == (counter * 8 + 24) // 25
        assert R.stream_end(counter, 48, 25) == (counter * 48 + 24) // 25
        assert R.stream_end(counter, 441, 1000) == (counter * 441 + 999) // 1000
        # interp == decim and interp != decim agree where the ratio is 1: 2/2 takes the first, (2, 2) spelled through the
        # division the second
        assert R.stream_end(counter, 2, 2) == -((-counter * 2) // 2)
        a = R.gather(counter, 3, 3, 64, 10, 32, (0, 0))
        b = R.gather(counter * 3, 1, 3, 64, 10, 32, (0, 0))
        assert a == b
    # the audio bound holds every block's increase of the stream, wherever the block starts
    for i, d in ((8, 25), (48, 25), (441, 1000), (1, 1)):
        for n_k in (1, 37, 500, 1200):
            for before in range(0, 60, 7):
                assert R.stream_end(before + n_k, i, d) - R.stream_end(before, i, d) <= R.audio_bound(n_k, i, d)
