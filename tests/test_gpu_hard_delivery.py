"""Everything behind the slicer through the real-time pump (rcf_pump_subscribe_hard): packed words, sync hits and the records
of the TSBK, EDACS, OSW and P25 voice stages reach the host without a read that synchronises the stream.  The yardstick is
always a twin front-end fed the same samples block by block and read with the single readers (rcf_chan_read_hard / _sync /
_tsbk / _edacs / _osw / _p25lc): equality is of bits.  Where a slot does not carry the whole stream -- host rings of 16 records,
a subscription on a ring that has wrapped -- tests/delivery_ref.py says which items of the twin's stream it must hold.
Front-ends run at 400 kS/s with 25 kS/s channels and blocks of 500 channel samples; the carriers are the sibling suites'
(test_gpu_frames_fuzz._planted: the EDACS and TSDU fixtures, clean OSW frames, the encrypted voice call), the TSDU fixture
once more as pi/4-DQPSK, and codewords_ref's dense NID stream, a frame every 72 dibits."""
import ctypes
import functools
import time

import numpy as np
import pytest

import delivery_ref as R
import slicer_ref as S
from rcf import control, p25, synth

pytestmark = pytest.mark.gpu

FS, CR, D, BLK = 400e3, 12500, 16, 500
F_EDACS, F_TSDU, F_OSW, F_CALL, F_CQPSK = -140e3, -100e3, -60e3, -20e3, 60e3      # the first four: _planted's
HARD = ("hard", "sync", "tsbk", "edacs", "osw", "p25lc")
STREAM_OF = dict(tsbk="tsbk", tsbk_cqpsk="tsbk", edacs="edacs", osw="osw", p25lc="p25lc")
OFF_OF = dict(tsbk=F_TSDU, tsbk_cqpsk=F_CQPSK, edacs=F_EDACS, osw=F_OSW, p25lc=F_CALL)


def _same(got, want, what=""):
    assert got.dtype == want.dtype and len(got) == len(want), (what, got.dtype, want.dtype, len(got), len(want))
    assert got.tobytes() == want.tobytes(), (what, got[:3], want[:3])


@functools.lru_cache(maxsize=None)
def _signal(total):
    """noise, _planted's four carriers and the TSDU fixture as DQPSK at F_CQPSK (made once, never written to)"""
    import gc_ref as G
    from test_gpu_frames_fuzz import _planted
    from test_gpu_tsbk import tsdu_dibits
    x = (0.02 * synth.awgn(np.random.default_rng(9100), total)).astype(np.complex64)
    made = list(_planted(total)) + [G.dqpsk_carrier(tsdu_dibits()[0], 4800, FS, F_CQPSK + 60.0, 0.4, amplitude=0.4)]
    for c in made:
        n = min(len(c), total)
        x[:n] += c[:n]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _dense(total):
    """codewords_ref.dense_nid_dibits as a C4FM carrier at F_TSDU: after 1000 dibits a frame every 72"""
    import codewords_ref as CW
    import fsk4_ref as F
    d = CW.dense_nid_dibits()[0][:int(total * 4800 / FS) + 9]
    x = (0.4 * F.c4fm_carrier(d, 4800, FS, F_TSDU + 150.0, 0.5, 600.0)[:total]).astype(np.complex64)
    x = x + (0.01 * synth.awgn(np.random.default_rng(9101), len(x))).astype(np.complex64)
    x.setflags(write=False)
    return x


def _chain(nat, fe, kind, f, stage=True, rec_cap=0, loose=False, hit_cap=0, direct=False, nid=True):
    """a channel at f with the loop and the slicer of `kind` and, with stage, its decoder -> the id its streams are read on.
    direct: the loop sits on the channel itself, without p25's chained pre-filter"""
    c = fe.chan_open(CR, f)
    if kind in ("tsbk", "p25lc"):
        if direct:
            fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR, 4800))
        else:
            c = p25.c4fm_front_half(fe, c, CR, 4800)
        fe.chan_fsk4(c, **p25.fsk4_params(CR, 4800))
        fe.chan_slicer(c, nat.READ_FSK4, nat.SLICE_FSK4, p25.SLICER_LEVELS, p25.FRAME_SYNC, 48, 13 if loose else 4, hit_capacity=hit_cap)
    elif kind == "tsbk_cqpsk":
        if direct:
            fe.chan_agc(c, 64, 1.0)
        else:
            c = p25.cqpsk_front_half(fe, c, CR)
        fe.chan_costas(c, **p25.costas_params(CR, 4800))
        fe.chan_slicer(c, nat.READ_COSTAS, nat.SLICE_FSK4, p25.SLICER_LEVELS, p25.FRAME_SYNC, 48, 17 if loose else 4, hit_capacity=hit_cap)
    elif kind == "edacs":
        control.edacs_clock(fe, c)
        fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_BINARY, sync_word=control.EDACS_SYNC, sync_bits=48, sync_max_errors=17 if loose else 0,
                       sync_both=1, hit_capacity=hit_cap)
    else:
        control.smartnet_clock(fe, c)
        fe.chan_slicer(c, nat.READ_CLOCK, nat.SLICE_BINARY, sync_word=control.SMARTNET_SYNC, sync_bits=8, hit_capacity=hit_cap)
    if stage:
        _stage(fe, c, kind, rec_cap, nid)
    return c


def _stage(fe, c, kind, rec_cap=0, nid=True):
    if kind in ("tsbk", "tsbk_cqpsk"):
        fe.chan_tsbk(c, rec_cap, nid=nid)
    elif kind == "edacs":
        fe.chan_edacs(c, rec_cap)
    elif kind == "osw":
        fe.chan_osw(c, rec_cap)
    else:
        fe.chan_p25lc_ex(c, rec_cap, es=True, erasures=True, nid=nid)


def _single(fe, c, what, *a):
    """the single reader of stream `what` in the pump's item form: uint32 words, uint32 hit items, or the stage's records"""
    if what == "hard":
        return fe.chan_read_hard(c, *a).view(np.uint32)
    if what == "sync":
        return S.hit_items(*fe.chan_read_sync(c, *a))
    return getattr(fe, "chan_read_" + what)(c, *a)              # soft symbols, IQ, or a decoder's records


def _n_items(fe, c, what):
    if what in ("hard", "sync"):
        return fe.chan_slicer_state(c)["n_words" if what == "hard" else "n_hits"]
    st = getattr(fe, "chan_%s_state" % what)(c)
    return st["n_records"] if "n_records" in st else st["n_symbols"]   # (a loop's soft symbols)


def _wait_blocks(pump, n, timeout_s=30.0):
    t_end = time.monotonic() + timeout_s
    while time.monotonic() < t_end:
        st = pump.stats()
        if st["blocks_done"] >= n or not st["running"]:
            return st
        time.sleep(0.002)
    raise AssertionError("the pump did not get to %d blocks: %r" % (n, pump.stats()))


class _Fed:
    """front-ends under a counter-fed pump (the pattern of tests/test_gpu_stage_delivery.py): member m's whole stream xs[m]
    sits in a pinned ring, `feed(k)` counts k blocks complete on every member; opener(nat, m) -> (front-end, channel ids)
    makes member m, and its twin"""

    def __init__(self, nat, xs, n_blocks, opener, out_ring_samples=1 << 12, max_read=16, subs=(), what="iq", blk=BLK):
        self.nat, self.xs, self.n_blocks, self.opener, self.blk, self.G = nat, xs, n_blocks, opener, blk, len(xs)
        assert all(len(x) >= D * blk * n_blocks for x in xs)
        self.fes, self.ids = zip(*[opener(nat, m) for m in range(self.G)])
        self.rings, self.counters = [], []
        for x in xs:
            r = nat.PinnedArray(D * blk * n_blocks, np.complex64)
            r.array[:] = x[:D * blk * n_blocks]
            self.rings.append(r)
            self.counters.append(np.zeros(1, dtype=np.uint64))
        self.grp = nat.Group(list(self.fes))
        self.pump = nat.Pump(self.grp, self.rings, D * blk, FS, [(m, self.ids[m][k]) for m, k in subs], fmt=nat.FMT_CF32, what=what,
                             out_ring_samples=out_ring_samples, n_blocks=n_blocks, max_read=max_read, written=self.counters,
                             start_delay_s=0.0)

    def feed(self, k, wait=True):
        for c in self.counters:
            c[0] = k
        if wait:
            st = _wait_blocks(self.pump, self.G * k)
            assert st["error"] == 0, st

    def finish(self):
        self.feed(self.n_blocks, wait=False)
        st = self.pump.wait(timeout_s=30.0)
        assert not st["running"] and st["error"] == 0 and st["blocks_done"] == self.G * self.n_blocks, st

    def close(self):
        self.pump.stop()
        self.grp.close()
        for fe in self.fes:
            fe.close()
        for r in self.rings:
            r.free()

    def twin(self, m):
        """member m's twin, fed block by block: yields (block index, front-end, channel ids) after each push"""
        tw, ids_t = self.opener(self.nat, m)
        try:
            for b in range(self.n_blocks):
                tw.push(self.xs[m][D * self.blk * b: D * self.blk * (b + 1)])
                yield b, tw, ids_t
        finally:
            tw.close()

    def twin_streams(self, m, keys):
        """member m's twin over all blocks, for keys (channel index, what): the single reads block by block and the stage's
        item count after every block"""
        parts, counters = {key: [] for key in keys}, {key: [] for key in keys}
        for b, tw, ids_t in self.twin(m):
            for (k, what) in keys:
                parts[(k, what)].append(_single(tw, ids_t[k], what))
                counters[(k, what)].append(_n_items(tw, ids_t[k], what))
        return parts, counters


def _frontend(nat, blk=BLK, out_capacity=1 << 12):
    return nat.Frontend(FS, 0.0, device=0, block_capacity=D * blk, out_capacity=out_capacity)


def _cat(parts, dtype=None):
    return np.concatenate(parts) if len(parts) else np.zeros(0, dtype)


# ------------------------------------------------------------------------------------------------ 1. whole delivery
def test_pump_delivers_all_six_streams_whole(gpu_required):
    """one pump, three members: TSBK behind the C4FM loop and behind the Gardner / Costas loop; EDACS and OSW behind the binary
    slicer; the voice stage with es, erasures and nid -- and every slicer's words and hits beside them"""
    nat = gpu_required
    n_blocks = 40
    x = _signal(D * BLK * n_blocks + 3200)
    xs = [x[1600 * m:] for m in range(3)]                         # (each member a cut of its own: its k differ from the others')
    kinds = [("tsbk", "tsbk_cqpsk"), ("edacs", "osw"), ("p25lc",)]

    def opener(nat_, m):
        fe = _frontend(nat_)
        return fe, [_chain(nat_, fe, kind, OFF_OF[kind]) for kind in kinds[m]]
    keys = [(m, k, what) for m in range(3) for k, kind in enumerate(kinds[m]) for what in (STREAM_OF[kind], "hard", "sync")]
    f = _Fed(nat, xs, n_blocks, opener, max_read=len(keys))
    try:
        slots = {key: f.pump.subscribe(key[0], f.ids[key[0]][key[1]], key[2]) for key in keys}
        assert sorted(slots.values()) == list(range(len(keys)))
        start = {key: f.pump._cursors[e].value for key, e in slots.items()}
        f.finish()
        got = {key: f.pump.read(e) for key, e in slots.items()}
        written = {key: f.pump.written(e) for key, e in slots.items()}
    finally:
        f.close()
    for m in range(3):
        parts, _ = f.twin_streams(m, [(k, what) for m_, k, what in keys if m_ == m])
        for (k, what), v in parts.items():
            w = _cat(v)
            assert start[(m, k, what)] == 0 and written[(m, k, what)] == len(w) > 0, (m, k, what, written[(m, k, what)], len(w))
            _same(got[(m, k, what)], w, (m, k, what))
            assert w.dtype == (np.uint32 if what in ("hard", "sync") else nat._read_dtype(what))
    assert {what for _, _, what in keys} == set(HARD)
    print("    whole delivery: items per slot %s" % {"%d/%d/%s" % key: n for key, n in written.items()})


# ------------------------------------------------------------------------------------------------ 2. smallest rings
def _check_records(recs, what):
    """a cheap look at every record beside the comparison of bytes with the twin's, which is what catches a torn one: k never
    goes back, and word 0's distance field lies within the strict search (<= 4)"""
    k = recs["k"].astype(np.int64)
    assert np.all(np.diff(k) >= 0), (what, k)
    dist = (recs["flags"] >> 10) & 63
    assert np.all(dist <= 4), (what, dist)


def test_pump_host_rings_of_16_records_and_a_reader_that_sleeps(gpu_required):
    """out_ring_samples = 64: 16 records a slot.  Two members with the same dense stream; on each a TSBK and a voice stage with
    record rings of 16, and a TSBK stage with a ring of 64 that is subscribed after 36 blocks -- its first gather finds more
    than the host ring holds and keeps the newest 16 (the kernel's `room`, in items).  Member 0's reader reads after every
    block and gets everything; member 1's reads every sixteenth block and gets the last 16 records written, whole"""
    nat = gpu_required
    n_blocks, late, room = 48, 36, 16
    xs = [_dense(D * BLK * n_blocks)] * 2

    def opener(nat_, m):
        fe = _frontend(nat_)
        return fe, [_chain(nat_, fe, "tsbk", F_TSDU, rec_cap=16), _chain(nat_, fe, "p25lc", F_TSDU, rec_cap=16),
                    _chain(nat_, fe, "tsbk", F_TSDU, rec_cap=64)]
    keys = [(0, "tsbk"), (1, "p25lc"), (2, "tsbk")]
    f = _Fed(nat, xs, n_blocks, opener, out_ring_samples=64, max_read=8)
    reads = {(m, key): [] for m in range(2) for key in keys}
    try:
        pump = f.pump
        slots = {(m, key): pump.subscribe(m, f.ids[m][key[0]], key[1]) for m in range(2) for key in keys[:2]}
        for b in range(n_blocks):
            f.feed(b + 1)
            if b + 1 == late:
                slots.update({(m, keys[2]): pump.subscribe(m, f.ids[m][2], "tsbk") for m in range(2)})
                late_at = {m: pump._cursors[slots[(m, keys[2])]].value for m in range(2)}
            for (m, key), e in slots.items():
                if m == 0 or (b + 1) % 16 == 0:
                    before = pump._cursors[e].value
                    r = pump.read(e)
                    reads[(m, key)].append((b, before, pump._cursors[e].value, r, pump.written(e)))
    finally:
        f.close()
    parts, counters = f.twin_streams(0, keys)
    for key in keys:
        what = key[1]
        s = _cat(parts[key])
        c = counters[key]
        first = late if key == keys[2] else 0
        cap = 64 if key == keys[2] else 16
        assert c[-1] == len(s) > room and (key != keys[2] or c[late] > room), (key, c)     # the rings wrap
        bounds = [24 if what == "tsbk" else 22] * n_blocks      # rcf.h: (500 + 15) / 24 + 3 and + 1
        idx, items, per, w = R.replay_slot(s, c, bounds, cap=cap, room=room, first=first)
        taken = s[np.asarray(idx, dtype=np.int64)]
        if key != keys[2]:
            assert idx == list(range(len(s)))                   # a ring of 16 under at most 4 records a block: everything
        else:
            assert idx[0] == c[late] - room > 0 and idx == list(range(idx[0], len(s)))      # the newest 16, then all
        for m in range(2):
            at0 = 0 if key != keys[2] else late_at[m]
            assert at0 == 0
            got = []
            for b, before, after, r, written in reads[(m, key)]:
                n_at_b = sum(n for _, n in per[:b - first + 1]) if b >= first else 0
                assert written == n_at_b, (m, key, b, written, n_at_b)
                # the pump is idle: the reader gets what lies between its cursor and `written`, of it the last 16
                lo = max(before, written - room)
                assert after == written and after - len(r) == lo, (m, key, b, before, after, len(r), written)
                _same(r, taken[lo:written], (m, key, b))
                _check_records(r, what)
                got.append(r)
            if m == 0:
                _same(_cat(got, s.dtype), taken, (key, "the reader that reads every block"))
            else:
                assert sum(len(r) for r in got) < len(taken), (key, "the sleeping reader lost nothing?")
        assert w == len(taken)
    print("    rings of 16: %s records" % {key: counters[key][-1] for key in keys})


# ------------------------------------------------------------------------------------------------ 3. subscription cases
def test_subscriptions_in_flight_part_way_and_on_a_wrapped_ring(gpu_required):
    nat = gpu_required
    n_blocks = 40
    xs = [_dense(D * BLK * n_blocks)]

    def opener(nat_, m):
        fe = _frontend(nat_)
        return fe, [_chain(nat_, fe, "tsbk", F_TSDU), _chain(nat_, fe, "p25lc", F_TSDU), _chain(nat_, fe, "tsbk", F_TSDU, rec_cap=16, hit_cap=16)]
    f = _Fed(nat, xs, n_blocks, opener, max_read=8)
    try:
        pump, fe, ids = f.pump, f.fes[0], f.ids[0]
        f.feed(18)
        f.feed(24, wait=False)                                  # blocks in flight while the subscription is made
        e_fly = pump.subscribe(0, ids[0], "tsbk")
        e_hits = pump.subscribe(0, ids[0], "sync")
        f.feed(28)
        head = fe.chan_read_p25lc(ids[1], 3)                    # the single reader takes three records; the pump is idle
        e_part = pump.subscribe(0, ids[1], "p25lc")
        f.feed(36)
        e_wrap = pump.subscribe(0, ids[2], "tsbk")              # a record ring of 16 that has wrapped
        e_wrap_hits = pump.subscribe(0, ids[2], "sync")         # ... and a hit ring of 16
        starts = [pump._cursors[e].value for e in (e_fly, e_hits, e_part, e_wrap, e_wrap_hits)]
        f.finish()
        got = {e: pump.read(e) for e in (e_fly, e_hits, e_part, e_wrap, e_wrap_hits)}
        written = {e: pump.written(e) for e in got}
    finally:
        f.close()
    keys = [(0, "tsbk"), (0, "sync"), (1, "p25lc"), (2, "tsbk"), (2, "sync")]
    parts, counters = f.twin_streams(0, keys)
    s = {key: _cat(v) for key, v in parts.items()}
    assert starts == [0] * 5
    # nobody had read the channel and its rings held everything: the whole stream, whichever block carried the first gather
    _same(got[e_fly], s[(0, "tsbk")], "in flight")
    _same(got[e_hits], s[(0, "sync")], "in flight, hits")
    assert written[e_fly] == len(s[(0, "tsbk")]) > 16 and written[e_hits] == len(s[(0, "sync")]) > 16
    assert len(head) == 3 < counters[(1, "p25lc")][27]
    _same(head, s[(1, "p25lc")][:3], "head")
    _same(got[e_part], s[(1, "p25lc")][3:], "from the single reader on")
    assert written[e_part] == len(s[(1, "p25lc")]) - 3 > 0
    for e, key in ((e_wrap, (2, "tsbk")), (e_wrap_hits, (2, "sync"))):
        c = counters[key]
        assert c[35] > 16 + 4, (key, c[35])                      # more than a ring had gone by
        idx, _, per, w = R.replay_slot(s[key], c, [24 if key[1] == "tsbk" else 501] * n_blocks, cap=16, room=1024, first=36)
        assert per[0] == (c[36] - 16, 16) and idx == list(range(c[36] - 16, len(s[key])))
        _same(got[e], s[key][idx[0]:], key)
        assert written[e] == w == len(idx)


def test_stage_attached_later_attached_again_switched_off_and_channel_closed(gpu_required):
    nat = gpu_required
    n_blocks = 40
    xs = [_dense(D * BLK * n_blocks)]
    ops = {8: "attach", 26: "again", 34: "off"}                  # after that many blocks

    def opener(nat_, m):
        fe = _frontend(nat_)
        return fe, [_chain(nat_, fe, "tsbk", F_TSDU, stage=False), _chain(nat_, fe, "tsbk", F_TSDU), _chain(nat_, fe, "p25lc", F_TSDU),
                    _chain(nat_, fe, "tsbk", F_TSDU)]

    def apply(fe, ids, op):
        if op == "attach":
            _stage(fe, ids[0], "tsbk")                           # the stage comes after the subscription
        elif op == "again":
            _stage(fe, ids[1], "tsbk")                           # a new stream at its item 0
            fe.chan_slicer(ids[3], nat.READ_FSK4, nat.SLICE_FSK4, p25.SLICER_LEVELS, p25.FRAME_SYNC, 48, 4)   # the slicer again: the stage is gone
        else:
            fe.chan_p25lc(ids[2], on=False)                      # off: the slot starves
            fe.chan_close(ids[1])                                # closed under its subscription
    keys = [(0, "tsbk"), (1, "tsbk"), (2, "p25lc"), (3, "tsbk"), (3, "hard")]
    f = _Fed(nat, xs, n_blocks, opener, max_read=8)
    try:
        pump = f.pump
        slots = {key: pump.subscribe(0, f.ids[0][key[0]], key[1]) for key in keys}       # (0, "tsbk"): no stage yet, no error
        for at in sorted(ops):
            f.feed(at)
            apply(f.fes[0], f.ids[0], ops[at])
        f.finish()
        got = {key: pump.read(e) for key, e in slots.items()}
        written = {key: pump.written(e) for key, e in slots.items()}
    finally:
        f.close()
    want = {key: [] for key in keys}
    live = set(keys)
    for b, tw, ids_t in f.twin(0):
        for key in sorted(live):
            if key == (0, "tsbk") and b < 8:
                continue
            want[key].append(_single(tw, ids_t[key[0]], key[1]))
        if b + 1 in ops:
            apply(tw, ids_t, ops[b + 1])
            if ops[b + 1] == "again":
                live.discard((3, "tsbk"))
            if ops[b + 1] == "off":
                live -= {(1, "tsbk"), (2, "p25lc")}
    for key in keys:
        w = _cat(want[key], nat._read_dtype(key[1]))
        assert written[key] == len(w) > 0, (key, written[key], len(w))
        _same(got[key], w, key)
    n_before = sum(len(v) for v in want[(1, "tsbk")][:26])
    assert 0 < n_before < len(_cat(want[(1, "tsbk")]))           # records on either side of the new attachment, no gap between
    n_hard = sum(len(v) for v in want[(3, "hard")][:26])
    assert 0 < n_hard < len(_cat(want[(3, "hard")]))             # ... and words of both slicers in one count


def test_slot_passes_from_soft_symbols_to_records_to_words(gpu_required):
    """one slot, three tenants with three item sizes: float32 soft symbols, 32-byte records, uint32 words.  Each new stream
    begins at the cursor its subscription returned and is whole from there; the count goes on"""
    nat = gpu_required
    n_blocks = 40
    xs = [_dense(D * BLK * n_blocks)]

    def opener(nat_, m):
        fe = _frontend(nat_)
        return fe, [_chain(nat_, fe, "tsbk", F_TSDU)]
    f = _Fed(nat, xs, n_blocks, opener, max_read=1, subs=[(0, 0)], what="fsk4")
    try:
        pump, c = f.pump, f.ids[0][0]
        f.feed(4)
        f.feed(5, wait=False)                                   # (no wait: the hand-over meets whatever is in flight)
        a = pump.read(0)
        pump.unsubscribe(0)
        assert pump.subscribe(0, c, "tsbk") == 0
        at_b = pump._cursors[0].value
        assert at_b >= len(a)
        f.feed(30)
        b = pump.read(0)
        assert b.dtype == nat.TSBK_DTYPE and pump.written(0) == at_b + len(b)
        pump.unsubscribe(0)
        assert pump.subscribe(0, c, "hard") == 0
        at_c = pump._cursors[0].value
        assert at_c == at_b + len(b)                            # nothing in flight: the count is exact again
        f.finish()
        w = pump.read(0)
        assert w.dtype == np.uint32 and pump.written(0) == at_c + len(w)
    finally:
        f.close()
    parts, _ = f.twin_streams(0, [(0, "fsk4"), (0, "tsbk"), (0, "hard")])
    soft = _cat(parts[(0, "fsk4")])
    assert len(_cat(parts[(0, "fsk4")][:4])) <= len(a) <= len(soft)
    _same(a, soft[:len(a)], "soft symbols")
    _same(b, _cat(parts[(0, "tsbk")][:30]), "records")          # from the channel's own reader on: item 0
    _same(w, _cat(parts[(0, "hard")]), "words")
    assert len(b) > 8 and len(w) > 100


# ------------------------------------------------------------------------------------------------ 4. scale and mixing
def test_130_slots_of_mixed_stages_on_two_grouped_front_ends(gpu_required):
    """2 x 65 channels, every one with a slot: more counted records than the gather has workgroups, all blocks fed at once so
    that two are in flight.  Loose searches on the P25 and EDACS channels, so that noise frames come beside the planted ones"""
    nat = gpu_required
    t0 = time.monotonic()
    n_blocks = 20
    x = _signal(D * BLK * 40 + 3200)
    xs = [x[1600 * m:] for m in range(2)]
    rot = ("tsbk", "edacs", "osw", "tsbk_cqpsk", "p25lc", "hard", "sync")
    chain_of = dict(hard="tsbk", sync="edacs")

    def what_of(k):
        return STREAM_OF.get(rot[k % 7], rot[k % 7])

    def opener(nat_, m):
        fe = _frontend(nat_)
        ids = []
        for k in range(65):
            kind = chain_of.get(rot[k % 7], rot[k % 7])
            ids.append(_chain(nat_, fe, kind, OFF_OF[kind] + 40.0 * (k // 7), loose=True, hit_cap=4096, direct=True, nid=bool(k % 2)))
        return fe, ids
    f = _Fed(nat, xs, n_blocks, opener, max_read=130)
    try:
        slots = {(m, k): f.pump.subscribe(m, f.ids[m][k], what_of(k)) for m in range(2) for k in range(65)}
        assert sorted(slots.values()) == list(range(130))
        f.finish()
        got = {key: f.pump.read(e) for key, e in slots.items()}
        written = {key: f.pump.written(e) for key, e in slots.items()}
    finally:
        f.close()
    total = {what: 0 for what in HARD}
    for m in range(2):
        parts, _ = f.twin_streams(m, [(k, what_of(k)) for k in range(65)])
        for k in range(65):
            w = _cat(parts[(k, what_of(k))])
            assert written[(m, k)] == len(w), (m, k, what_of(k), written[(m, k)], len(w))
            _same(got[(m, k)], w, (m, k, what_of(k)))
            total[what_of(k)] += len(w)
    assert all(n > 0 for n in total.values()), total
    assert got[(0, 0)].tobytes() != got[(1, 0)].tobytes()
    print("    130 slots, two members, %d blocks: %s items, %.2f s" % (n_blocks, total, time.monotonic() - t0))


def test_read_many_rows_of_mixed_item_sizes_and_a_small_cap_each(gpu_required):
    """rcf_pump_read_many over slots of 8, 4 and 32 bytes an item: row i stays at i x cap_each x 8 bytes and holds cap_each
    items of up to 8 bytes or cap_each / 4 records.  With cap_each = 8 a record row holds two, fewer than are ready"""
    nat = gpu_required
    n_blocks = 40
    xs = [_signal(D * BLK * n_blocks + 3200)]

    def opener(nat_, m):
        fe = _frontend(nat_)
        return fe, [_chain(nat_, fe, "tsbk_cqpsk", F_CQPSK, loose=True, hit_cap=4096), _chain(nat_, fe, "edacs", F_EDACS)]
    keys = [(0, "iq"), (0, "tsbk"), (0, "costas"), (1, "edacs"), (1, "hard"), (0, "sync")]
    f = _Fed(nat, xs, n_blocks, opener, out_ring_samples=1 << 14, max_read=8)      # (the ring holds the 10 000 IQ samples of 20 blocks)
    got = {key: [] for key in keys}
    try:
        pump = f.pump
        slots = [pump.subscribe(0, f.ids[0][k], what) for k, what in keys]
        plan = pump.read_many_plan(slots + [7], cap_each=1023)    # (slot 7 is nobody's: an empty row; 1023: 255 records and 24 bytes over)
        for b in range(n_blocks - 20):
            f.feed(b + 1)
            rows = plan()
            assert len(rows) == 7 and len(rows[6]) == 0
            for key, r in zip(keys, rows):
                assert r.dtype == nat._read_dtype(key[1]) and len(r) <= (255 if key[1] in ("tsbk", "edacs") else 1023)
                got[key].append(r.copy())
        f.finish()
        # the last twenty blocks' items through the ABI itself, two records or eight words at a time
        lib = nat.lib()
        ents = (ctypes.c_int * 6)(*slots)
        curs = (ctypes.c_int64 * 6)(*[pump._cursors[e].value for e in slots])
        counts = (ctypes.c_int64 * 6)()
        out = np.zeros((6, 8), dtype=np.complex64)
        rows = [out[i].view(nat._read_dtype(what)) for i, (_, what) in enumerate(keys)]
        most = {key: 0 for key in keys}
        for _ in range(100000):
            assert lib.rcf_pump_read_many(pump._p, ents, curs, 6, out.ctypes.data_as(ctypes.c_void_p), 8, counts) == nat.RCF_OK
            if not any(counts):
                break
            for i, key in enumerate(keys):
                assert 0 <= counts[i] <= (2 if key[1] in ("tsbk", "edacs") else 8), (key, counts[i])
                most[key] = max(most[key], counts[i])
                got[key].append(rows[i][:counts[i]].copy())
        assert most[(0, "tsbk")] == 2 and most[(1, "hard")] == 8, most
    finally:
        f.close()
    want = {key: [] for key in keys}
    for b, tw, ids_t in f.twin(0):
        for key in keys:
            want[key].append(_single(tw, ids_t[key[0]], key[1]))
    for key in keys:
        w = _cat(want[key])
        assert len(w) > 2, (key, len(w))
        _same(_cat(got[key]), w, key)


# ------------------------------------------------------------------------------------------------ 5. the existing paths
def test_a_pump_without_hard_slots_and_the_batched_reader_give_the_twins_bits(gpu_required):
    """soft symbols and IQ through the pump with no hard subscription beside them, the records through rcf_chan_read_many once
    the pump has finished: what they were before this entry point, the twin's single reads"""
    nat = gpu_required
    n_blocks = 40
    xs = [_signal(D * BLK * n_blocks + 3200)]

    def opener(nat_, m):
        fe = _frontend(nat_)
        return fe, [_chain(nat_, fe, "tsbk", F_TSDU), _chain(nat_, fe, "edacs", F_EDACS)]
    f = _Fed(nat, xs, n_blocks, opener, out_ring_samples=1 << 15, max_read=4, subs=[(0, 0)], what="fsk4")   # (20 000 IQ samples)
    try:
        e_clock = f.pump.subscribe(0, f.ids[0][1], "clock")
        e_iq = f.pump.subscribe(0, f.ids[0][1], "iq")
        f.finish()
        soft, clock, iq = f.pump.read(0), f.pump.read(e_clock), f.pump.read(e_iq)
        tsbk = f.fes[0].chan_read_many([f.ids[0][0], f.ids[0][1]], "tsbk", cap_each=256)
        edacs = f.fes[0].chan_read_many([f.ids[0][1]], "edacs", cap_each=256)[0].copy()
        assert tsbk[1] is None
        tsbk = tsbk[0].copy()
    finally:
        f.close()
    want = dict(fsk4=[], tsbk=[], clock=[], iq=[], edacs=[])
    for b, tw, ids_t in f.twin(0):
        want["fsk4"].append(tw.chan_read_fsk4(ids_t[0]))
        want["tsbk"].append(tw.chan_read_tsbk(ids_t[0]))
        want["clock"].append(tw.chan_read_clock(ids_t[1]))
        want["iq"].append(tw.chan_read_iq(ids_t[1]))
        want["edacs"].append(tw.chan_read_edacs(ids_t[1]))
    for name, g in (("fsk4", soft), ("clock", clock), ("iq", iq), ("tsbk", tsbk), ("edacs", edacs)):
        w = _cat(want[name])
        assert len(w) > 8, (name, len(w))
        _same(g, w, name)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_of_the_old_and_the_new_entry_point(gpu_required):
    nat = gpu_required
    lib = nat.lib()
    six = (nat.HARD_BITS, nat.HARD_SYNC, nat.HARD_TSBK, nat.HARD_EDACS, nat.HARD_OSW, nat.HARD_P25LC)
    blk = D * BLK
    fe = _frontend(nat)
    c = _chain(nat, fe, "tsbk", F_TSDU)
    bare = fe.chan_open(CR, 0.0)                                 # no slicer: no error, the slot would starve
    ring = nat.PinnedArray(2 * blk, np.complex64)
    ring.array[:] = 0
    counter = np.zeros(1, dtype=np.uint64)
    grp = nat.Group([fe])
    cur = ctypes.c_int64(-1)

    def start(**kw):
        return nat.Pump(grp, [ring], blk, FS, (), fmt=nat.FMT_CF32, max_read=2, written=[counter], start_delay_s=0.0, **kw)
    try:
        for what in HARD:                                        # rcf_pump_start goes on refusing all six
            with pytest.raises(nat.RcfError) as e:
                start(what=what)
            assert e.value.code == nat.RCF_EINVAL, what
        pump = start(what="iq", out_ring_samples=64)
        for what in six:                                         # ... and so does rcf_pump_subscribe
            assert lib.rcf_pump_subscribe(pump._p, 0, c, what, 1.0, ctypes.byref(cur)) == nat.RCF_EINVAL, what
        for what in (0, 1, 17, 50, 2, 16, 19, 20, 34, 52, -1):
            assert lib.rcf_pump_subscribe_hard(pump._p, 0, c, what, ctypes.byref(cur)) == nat.RCF_EINVAL, what
        assert lib.rcf_pump_subscribe_hard(pump._p, 1, c, nat.HARD_TSBK, ctypes.byref(cur)) == nat.RCF_EINVAL      # no such member
        assert lib.rcf_pump_subscribe_hard(pump._p, 0, 9999, nat.HARD_TSBK, ctypes.byref(cur)) == nat.RCF_EINVAL   # no such channel
        assert lib.rcf_pump_subscribe_hard(pump._p, 0, nat.SRC_PFB_BIN0 + 1, nat.HARD_BITS, ctypes.byref(cur)) == nat.RCF_EINVAL
        assert lib.rcf_pump_subscribe_hard(None, 0, c, nat.HARD_TSBK, ctypes.byref(cur)) == nat.RCF_EINVAL
        assert cur.value == -1
        e0 = lib.rcf_pump_subscribe_hard(pump._p, 0, bare, nat.HARD_OSW, ctypes.byref(cur))      # 16 records: the smallest ring
        assert e0 == 0 and cur.value == 0
        e1 = lib.rcf_pump_subscribe_hard(pump._p, 0, c, nat.HARD_SYNC, None)                     # (the cursor is optional)
        assert e1 == 1
        assert lib.rcf_pump_subscribe_hard(pump._p, 0, c, nat.HARD_TSBK, ctypes.byref(cur)) == nat.RCF_ECAP         # no free slot
        assert lib.rcf_pump_unsubscribe(pump._p, e1) == nat.RCF_OK
        assert pump.subscribe(0, c, "p25lc") == 1 and pump.written(1) == 0
        pump.stop()
        pump = start(what="iq", out_ring_samples=32)             # 8 records a slot: RCF_ECAP; 32 words or hits: fine
        for what in six[2:]:
            assert lib.rcf_pump_subscribe_hard(pump._p, 0, c, what, ctypes.byref(cur)) == nat.RCF_ECAP, what
        assert lib.rcf_pump_subscribe_hard(pump._p, 0, c, nat.HARD_BITS, ctypes.byref(cur)) == 0
        assert lib.rcf_pump_subscribe_hard(pump._p, 0, c, nat.HARD_SYNC, ctypes.byref(cur)) == 1
        with pytest.raises(nat.RcfError) as e:
            pump.subscribe(0, c, "edacs")
        assert e.value.code == nat.RCF_ECAP
        pump.stop()
        pump = start(what="iq", out_ring_samples=8)              # 8 words: RCF_ECAP for the 4-byte streams too
        assert lib.rcf_pump_subscribe_hard(pump._p, 0, c, nat.HARD_BITS, ctypes.byref(cur)) == nat.RCF_ECAP
        pump.stop()
    finally:
        grp.close()
        fe.close()
        ring.free()
