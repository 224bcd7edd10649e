"""What the pump's slots of the streams behind the slicer (rcf_pump_subscribe_hard) rest on, without a GPU: the per-block
bounds and the slot geometry of radiocapture-rf_amd/csrc/rcf_streams.h compiled alone with g++ (tests/native/hard_bound_check.cpp,
once more under AddressSanitizer and UBSan) against a restatement written out here; tests/delivery_ref.py's whole-slot replay
with those bounds over the record counts the restatements of the stages (tsbk_ref, p25es_ref / nid_ref, edacs_ref, osw_ref,
slicer_ref) give block by block on the suites' own carriers -- the reference streams stay inside the lag guarantee of
include/rcf.h --; and NativeDataPlane.subscribe_records / read_records over a pump written out here."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import delivery_ref as DR
from rcf import native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HARD = {"hard": 32, "sync": 33, "tsbk": 48, "edacs": 49, "osw": 51, "p25lc": 53}
RECORDS = ("tsbk", "edacs", "osw", "p25lc")
N_KS = (0, 1, 37, 500, 1200)
BLOCKS = (500, 37, 1, 1200)                          # channel samples per block, at 25 kS/s


def bound(what, n_k, bps):
    """include/rcf.h at rcf_pump_subscribe_hard: the most a steady-state gather takes after a block of n_k channel outputs.
    A loop makes at most n_k + 1 symbols of them; the slicer's whole words then reach at most n_k + 1 + (32 / bps - 1) symbols
    further than before, and a decoder decides the frames whose threshold lies among those"""
    n_k = max(0, int(n_k))
    if what == "hard":
        return -((-n_k * bps) // 32) + 1
    if what == "sync":
        return n_k + 1
    span = n_k + (16 if what in ("tsbk", "p25lc") else 32)     # symbols the whole words may advance by: dibits, bits
    if what == "tsbk":                             # frames >= 24 dibits apart; one cut d dibits long gives <= d / 24 records, the last 3
        return (span - 1) // 24 + 3
    if what == "p25lc":                              # the same accept rule, one record a frame
        return (span - 1) // 24 + 1
    if what == "edacs":                              # frames >= 288 bits apart
        return (span - 1) // 288 + 1
    if what == "osw":                                # thresholds pos + 84 or h0 + 92, packets >= 84 bits apart: >= 76
        return (span - 1) // 76 + 1
    raise KeyError(what)


def ring_items(what, out_cap):
    """a slot is out_cap x 8 bytes: out_cap items of 4 bytes (half the slot) or out_cap / 4 records of 32"""
    return out_cap if what in ("hard", "sync") else out_cap // 4


def _build(name, flags):
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc")] + flags +
                          [os.path.join(HERE, "native", "hard_bound_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, (name, p.returncode, p.stderr.decode()[-2000:])
    return p.stdout.decode()


@pytest.fixture(scope="module")
def got():
    return json.loads(_build("hard_bound_check", ["-O1"]))


def test_hard_bound_equals_the_restatement(got):
    rows = {(w, bps, n): b for w, bps, n, b in got["bound"]}
    for name, what in HARD.items():
        for bps in (1, 2):
            for n in N_KS:
                assert rows[(what, bps, n)] == bound(name, n, bps) > 0, (name, bps, n, rows[(what, bps, n)])
    # every other stream the readers know is no hard stream; the program walked them all
    others = {w for w, _, _ in rows} - set(HARD.values())
    assert others == {0, 1, 2, 16, 17, 18, 19, 20} and all(rows[(w, bps, n)] == -1 for w in others for bps in (1, 2) for n in N_KS)
    # the figures the header states, at the suites' block of 500 channel samples
    assert [bound(w, 500, 2 if w in ("tsbk", "p25lc") else 1) for w in ("tsbk", "p25lc", "edacs", "osw")] == [24, 22, 2, 7]
    assert bound("hard", 500, 2) == 33 and bound("hard", 500, 1) == 17 and bound("sync", 500, 1) == 501


def test_slot_geometry_and_the_capacity_edge(got):
    rows = {(w, c): (item, r) for w, c, item, r in got["slot"]}
    for name, what in HARD.items():
        for cap in (16, 32, 64, 4096):
            item, r = rows[(what, cap)]
            assert item == (4 if name in ("hard", "sync") else 32) and r == ring_items(name, cap), (name, cap, item, r)
            assert r * item <= cap * 8                             # the ring lies inside its slot
            if name in RECORDS:
                assert r * item == cap * 8                         # ... and a record ring fills it
    for what in (0, 1, 2, 16, 17, 18, 19, 20):                     # the plain and soft streams keep out_cap items
        assert all(rows[(what, cap)][1] == cap for cap in (16, 32, 64, 4096))
    # R < 16 is RCF_ECAP: records need out_ring_samples >= 64, the 4-byte streams 16
    assert [cap for cap in (16, 32, 64, 4096) if ring_items("tsbk", cap) >= 16] == [64, 4096]
    assert [cap for cap in (16, 32, 64, 4096) if ring_items("sync", cap) >= 16] == [16, 32, 64, 4096]
    walked = {(w, c): (n, bad) for w, c, n, bad in got["ring"]}
    assert set(walked) == {(HARD[n], c) for n in HARD for c in (16, 32, 64, 4096) if ring_items(n, c) >= 16}
    assert all(n > 1000 and bad == 0 for n, bad in walked.values()), walked


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(got):
    text = _build("hard_bound_check_asan", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                            "-fno-sanitize-recover=undefined"])
    assert json.loads(text) == got


# ---------------------------------------------------------------- the reference streams inside the lag guarantee
def _soft(dibits):
    return np.array([1.0, 3.0, -1.0, -3.0], np.float32)[np.asarray(dibits)]


def _launches(sl, bps, baud, n_blocks):
    """an ideal loop: after each block of BLOCKS (25 kS/s) the symbols so far, the slicer's whole words and its hits"""
    out, samples = [], 0
    for b in range(n_blocks):
        samples += BLOCKS[b % 4]
        n_sym = min(sl["n_symbols"], int(samples * baud / 25000.0))
        out.append((n_sym * bps // 32, int(np.count_nonzero(sl["k"] < n_sym)), n_sym))
    return out


def _p25(dibits):
    import slicer_ref as S
    from rcf import p25
    return S.run(_soft(dibits), S.FSK4, sync_word=p25.FRAME_SYNC, sync_bits=48, max_errors=p25.FRAME_SYNC_MAX_ERRORS)


def _per_block_counts(what, sl, launches, recs):
    """records decided by the end of each block.  The three decoders whose frames are decided by a hit's k alone: the rule of
    include/rcf.h on the record's k; the OSW stage, whose cursor depends on its lock counter: the restatement run over the
    blocks so far"""
    import osw_ref as O
    if what == "osw":
        return [len(O.run(sl["words"], sl["k"], launches=[l[:2] for l in launches[:b + 1]])[0]) for b in range(len(launches))]
    lead, decide, sym_w = {"tsbk": (23, 384, 16), "p25lc": (23, 888, 16), "edacs": (47, 288, 32)}[what]
    k = recs["k"].astype(np.int64)
    return [int(np.count_nonzero(sym_w * n_words >= k - lead + decide)) for n_words, _, _ in launches]


@pytest.fixture(scope="module")
def reference_counts():
    """-> {name: (stream `what`, bps, stage ring, host ring R, cumulative items after every block)} over the suites' carriers"""
    import codewords_ref as CW
    import edacs_ref as ED
    import nid_ref as N
    import osw_ref as O
    import p25es_ref as E
    import p25lc_ref as LC
    import slicer_ref as S
    import tsbk_ref as T
    from rcf import control
    from test_gpu_edacs import edacs_bits
    from test_gpu_osw import clean_bits
    from test_gpu_tsbk import tsdu_dibits
    out = {}
    both = E.ES | E.ERASURES

    def p25_streams(name, dibits, n_blocks, cap, room):
        sl = _p25(dibits)
        la = _launches(sl, 2, 4800.0, n_blocks)
        tsbk = N.run_tsbk(sl["words"], sl["k"], sl["dist"], nid=1)[0]
        voice = N.run_voice(sl["words"], sl["k"], sl["dist"], nid=1, options=both)[0]
        out[name + " tsbk"] = ("tsbk", 2, cap, room, _per_block_counts("tsbk", sl, la, tsbk))
        out[name + " p25lc"] = ("p25lc", 2, cap, room, _per_block_counts("p25lc", sl, la, voice))
        return sl, la

    n40 = 40
    d = tsdu_dibits()[0]
    sl, la = p25_streams("tsdu", d, int(len(d) * 25000 / 4800 / (sum(BLOCKS) / 4)) + 8, 256, 1024)
    out["tsdu hard"] = ("hard", 2, 4096, 4096, [l[0] for l in la])
    out["tsdu sync"] = ("sync", 2, 256, 4096, [l[1] for l in la])
    d = LC.call_dibits()[0]
    p25_streams("call", d, int(len(d) * 25000 / 4800 / (sum(BLOCKS) / 4)) + 8, 256, 1024)
    # the dense NID stream: a TDU every 72 dibits, through rings of 16 and 16 over 40 blocks and the tail that decides them
    d = CW.dense_nid_dibits()[0][:int(sum(BLOCKS) * 10 * 4800 / 25000)]
    p25_streams("dense", d, n40 + 4, 16, 16)
    bits = edacs_bits()[0]
    sl = S.run(np.where(bits, 1.0, -1.0), S.BINARY, sync_word=control.EDACS_SYNC, sync_bits=48)
    la = _launches(sl, 1, 9600.0, int(len(bits) * 25000 / 9600 / (sum(BLOCKS) / 4)) + 8)
    out["edacs"] = ("edacs", 1, 256, 1024, _per_block_counts("edacs", sl, la, ED.run(sl["words"], sl["k"], sl["dist"])[0]))
    out["edacs hard"] = ("hard", 1, 4096, 4096, [l[0] for l in la])
    bits = clean_bits(36)[0]
    sl = O.slicer(bits)
    la = _launches(sl, 1, 3600.0, int(len(bits) * 25000 / 3600 / (sum(BLOCKS) / 4)) + 8)
    out["osw"] = ("osw", 1, 256, 1024, _per_block_counts("osw", sl, la, None))
    out["osw 16"] = ("osw", 1, 16, 16, out["osw"][4])
    out["osw sync"] = ("sync", 1, 256, 4096, [l[1] for l in la])
    return out


def test_replay_with_these_bounds_delivers_every_reference_record(reference_counts, got):
    """the bounds are the compiled header's (hard_bound through the check program), not this file's restatement"""
    compiled = {(w, bps, n): b for w, bps, n, b in got["bound"]}
    seen = set()
    for name, (what, bps, cap, room, counters) in reference_counts.items():
        total = counters[-1]
        assert total > 0 and counters == sorted(counters), (name, counters)
        bounds = [compiled[(HARD[what], bps, BLOCKS[b % 4])] for b in range(len(counters))]
        idx, items, per, written = DR.replay_slot(list(range(total)), counters, bounds, cap=cap, room=room)
        assert idx == list(range(total)) and written == total, (name, total, written, per)
        # ... and no block ever made more than its bound: nothing waited for the next block, so a reader that lags fewer than
        # R - 2 bound items behind `written` loses nothing
        made = np.diff([0] + counters)
        assert all(int(m) <= bd for m, bd in zip(made[1:], bounds[1:])), (name, made.tolist(), bounds)
        seen.add((what, cap, room))
        print("    %-12s %-6s ring %4d / %4d: %4d items in %d blocks, most per block %d (bound %d at 500)"
              % (name, what, cap, room, total, len(counters), int(made.max()), bound(what, 500, bps)))
    assert {w for w, _, _ in seen} == set(HARD)
    assert ("tsbk", 16, 16) in seen and ("p25lc", 16, 16) in seen and ("osw", 16, 16) in seen
    # the dense stream wraps rings of 16
    assert reference_counts["dense tsbk"][4][-1] > 16 and reference_counts["dense p25lc"][4][-1] > 16


# ---------------------------------------------------------------- the data plane over a pump written out here
class _FakePump:
    """slots as the pump hands them out.  A slot delivers what `queue` holds for ITS (channel, stream) and nothing else: a
    subscription on a channel that does not carry the stage starves, as the ABI says.  known: the member's native channels, if
    given -- any other id is RCF_EINVAL"""

    def __init__(self, known=None):
        self.slots, self.calls, self.free = {}, [], list(range(8))
        self.queue, self.known = {}, known

    def subscribe(self, member, chan_id, what="iq", gain=1.0):
        if self.known is not None and chan_id not in self.known:
            raise native.RcfError(native.RCF_EINVAL, "no such channel %d on member %d" % (chan_id, member))
        if not self.free:
            raise native.RcfError(native.RCF_ECAP, "all subscription slots of the pump are taken")
        e = self.free.pop(0)
        self.slots[e] = (member, chan_id, what)
        self.calls.append(("subscribe", member, chan_id, what))
        return e

    def unsubscribe(self, e):
        del self.slots[e]
        self.free.insert(0, e)
        self.calls.append(("unsubscribe", e))

    def read(self, e, max_items=1 << 16):
        member, chan_id, what = self.slots[e]
        self.calls.append(("read", e, max_items))
        q = self.queue.pop((chan_id, what), None)
        return np.zeros(0, native._read_dtype(what)) if q is None else q[:max_items]


class _Chan:
    def __init__(self, fe, chan_id):
        self.frontend, self.chan_id, self.port = fe, chan_id, 0


def _plane():
    from rcf import dataplane

    class Tb:
        access_lock = threading.RLock()
        channels = {}

    class Cl:
        pump = _FakePump()
    fes = [object(), object()]
    plane = object.__new__(dataplane.NativeDataPlane)              # (the constructor wants native front-ends and pinned rings)
    plane.native, plane.tb = native, Tb()
    plane.member_of = {id(fes[0]): (Cl, 0), id(fes[1]): (Cl, 1)}
    plane.subs, plane.rec_subs, plane.socks, plane.fm_socks, plane._plans = {}, {}, {}, {}, {}
    plane.tb.channels = {"a": _Chan(fes[0], 3), "b": _Chan(fes[1], 4), "idle": _Chan(fes[0], None), "alien": _Chan(object(), 9)}
    return plane, Cl.pump


def test_subscribe_records_is_lazy_follows_a_retune_and_goes_with_the_channel():
    plane, pump = _plane()
    assert plane.subscribe_records("a", "tsbk") == 0 and plane.subscribe_records("a", "tsbk") == 0     # once
    assert plane.subscribe_records("b", "osw") == 1 and plane.subscribe_records("a", "sync") == 2
    assert pump.calls == [("subscribe", 0, 3, "tsbk"), ("subscribe", 1, 4, "osw"), ("subscribe", 0, 3, "sync")]
    recs = np.zeros(3, native.TSBK_DTYPE)
    recs["k"] = [5, 6, 7]
    pump.queue[(3, "tsbk")] = recs
    got = plane.read_records("a", "tsbk")
    assert got.dtype == native.TSBK_DTYPE and got["k"].tolist() == [5, 6, 7]
    assert len(plane.read_records("a", "tsbk")) == 0 and plane.read_records("a", "sync").dtype == np.uint32
    got = plane.read_records("b", "edacs", max_items=7)            # read_records subscribes by itself
    assert got.dtype == native.EDACS_DTYPE and pump.calls[-2:] == [("subscribe", 1, 4, "edacs"), ("read", 3, 7)]
    # a retune gives the object a new native channel: the old slot goes, the stream is subscribed again
    plane.tb.channels["a"].chan_id = 11
    pump.queue[(11, "tsbk")] = recs[:1]
    assert plane.read_records("a", "tsbk")["k"].tolist() == [5]
    assert ("unsubscribe", 0) in pump.calls and pump.slots[0] == (0, 11, "tsbk") and pump.slots[2] == (0, 3, "sync")
    assert plane.subscribe_records("a", "sync") == 2 and pump.slots[2] == (0, 11, "sync")      # (slot 2 freed and taken again)
    # refusals leave nothing behind
    for block_id, what, exc in (("a", "iq", ValueError), ("a", "costas", ValueError), ("nobody", "tsbk", KeyError),
                                ("idle", "tsbk", KeyError), ("alien", "tsbk", RuntimeError)):
        with pytest.raises(exc):
            plane.subscribe_records(block_id, what)
    assert sorted(plane.rec_subs) == [("a", "sync"), ("a", "tsbk"), ("b", "edacs"), ("b", "osw")]
    # _drop releases every record slot of the channel and nobody else's
    plane._drop("a")
    assert sorted(plane.rec_subs) == [("b", "edacs"), ("b", "osw")] and sorted(pump.slots) == [1, 3]
    plane._drop("b")
    assert plane.rec_subs == {} and pump.slots == {} and sorted(pump.free) == list(range(8))


def test_a_stage_on_a_chained_channel_is_named_by_the_caller_and_starves_on_the_blocks_own():
    """rcf.p25.c4fm_demod / cqpsk_demod put loop, slicer and decoder on a chained pre-filter channel and return its id: block
    "a" owns native channel 3, its P25 chain is channel 7.  Subscribed without the name the slot sits on 3 and starves; named,
    it delivers, and the name is remembered.  A retune replaces channel 3 and takes the chain with it: the slot is released
    and the caller told, until it names the new chain.  An own-channel stream (EDACS) follows the retune by itself"""
    plane, pump = _plane()
    pump.known = {3, 4, 7}
    recs = np.zeros(4, native.TSBK_DTYPE)
    recs["k"] = [1, 2, 3, 4]
    pump.queue[(7, "tsbk")] = recs[:2]
    assert len(plane.read_records("a", "tsbk")) == 0 and pump.slots[0] == (0, 3, "tsbk")        # the block's own channel: starved
    assert (7, "tsbk") in pump.queue
    got = plane.read_records("a", "tsbk", chan_id=7)             # named: the subscription moves to the chain's channel
    assert got["k"].tolist() == [1, 2] and pump.slots == {0: (0, 7, "tsbk")}
    pump.queue[(7, "tsbk")] = recs[2:]
    assert plane.read_records("a", "tsbk")["k"].tolist() == [3, 4]                            # remembered
    assert plane.subscribe_records("a", "tsbk") == 0 and plane.subscribe_records("a", "tsbk", chan_id=7) == 0
    assert [c for c in pump.calls if c[0] != "read"] == [("subscribe", 0, 3, "tsbk"), ("unsubscribe", 0), ("subscribe", 0, 7, "tsbk")]
    assert plane.read_records("a", "tsbk").dtype == native.TSBK_DTYPE and pump.calls[-1] == ("read", 0, 256)
    assert plane.read_records("a", "hard", chan_id=7).dtype == np.uint32 and pump.calls[-1] == ("read", 1, 4096)
    plane.subscribe_records("a", "edacs")                        # a stream on the block's own channel beside them
    assert pump.slots[2] == (0, 3, "edacs")
    with pytest.raises(native.RcfError) as e:                    # a name the member does not know
        plane.subscribe_records("b", "p25lc", chan_id=99)
    assert e.value.code == native.RCF_EINVAL and ("b", "p25lc") not in plane.rec_subs
    # the retune: channel 3 becomes 11, the chain on 7 is gone with it
    plane.tb.channels["a"].chan_id = 11
    pump.known = {4, 11}
    with pytest.raises(RuntimeError):
        plane.read_records("a", "tsbk")
    assert ("a", "tsbk") not in plane.rec_subs and 0 not in pump.slots                         # released, not left starving
    assert len(plane.read_records("a", "edacs")) == 0 and (0, 11, "edacs") in pump.slots.values()   # followed by itself
    pump.known = {4, 11, 12}                                     # the caller built the chain again: channel 12
    pump.queue[(12, "tsbk")] = recs[:1]
    assert plane.read_records("a", "tsbk", chan_id=12)["k"].tolist() == [1]
    assert plane.read_records("a", "hard", chan_id=12).dtype == np.uint32 and (0, 12, "hard") in pump.slots.values()
    assert (0, 7, "hard") not in pump.slots.values()
    # no free slot: the pump's RCF_ECAP reaches the caller
    pump.free = []
    with pytest.raises(native.RcfError) as e:
        plane.subscribe_records("b", "osw")
    assert e.value.code == native.RCF_ECAP
    plane._drop("a")
    assert plane.rec_subs == {} and pump.slots == {}


def test_the_binding_names_the_new_entry_point_and_its_item_types():
    assert "rcf_pump_subscribe_hard" in native.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "rcf.h")).read()
    assert "int rcf_pump_subscribe_hard(rcf_pump_t *p, int member, int chan_id, int what, int64_t *cursor);" in hdr
    assert native._HARD_WHAT == HARD
    assert native._read_dtype("hard") == native._read_dtype("sync") == np.uint32
    for name, dt in (("tsbk", native.TSBK_DTYPE), ("edacs", native.EDACS_DTYPE), ("osw", native.OSW_DTYPE), ("p25lc", native.P25LC_DTYPE)):
        assert native._read_dtype(name) == dt and dt.itemsize == 32
