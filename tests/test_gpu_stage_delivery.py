"""The stages' streams -- symbol filter, the three symbol loops' soft symbols, the voice chain's audio -- through the batched
readers (rcf_chan_read_many / rcf_group_read_many, RCF_READ_SYM .. RCF_READ_AUDIO) and the real-time pump.  How many items
a loop or the voice chain has produced only the device knows; the counted gather (ingest.hip) reads the counter itself.
The yardstick is always a twin front-end fed the same samples and read with the single readers (rcf_chan_read_sym / _clock
/ _costas / _fsk4 / _audio): equality is of bits."""
import ctypes
import time

import numpy as np
import pytest

from rcf import audio as host_audio
from rcf import p25, synth

pytestmark = pytest.mark.gpu

FS, CR, D = 2.4e6, 12500, 96                       # 12.5 kHz channels: decimation 96, 25 kS/s
BLOCKS = (500, 37, 1, 1200)                        # channel samples per block
OFFS = [-62500.0 + 25000.0 * k for k in range(6)]
WHATS = ("sym", "clock", "costas", "fsk4", "audio")
SINGLE = {"sym": "chan_read_sym", "clock": "chan_read_clock", "costas": "chan_read_costas", "fsk4": "chan_read_fsk4",
          "audio": "chan_read_audio", "agc": "chan_read_agc"}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32)


def _same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(_bits(got), _bits(want)), what


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    x = synth.awgn(rng, n).astype(np.complex128)
    for k in (0, 2, 3):
        x += synth.nbfm_carrier(n, FS, OFFS[k], 600.0 + 170 * k, 2500.0, synth.snr_amp(25.0, 12500.0, FS))
    return x.astype(np.complex64)


def _cuts(blocks):
    at = np.concatenate([[0], np.cumsum([D * b for b in blocks])])
    return list(zip(at[:-1], at[1:]))


def _stages(fe, c, audio=True, agc_n=64):
    """every stage on one channel: symbol filter + C4FM loop, AGC + Gardner / Costas, symbol clock, voice chain"""
    fe.chan_fm_filter(c, p25.fm_gain(CR), p25.symbol_taps(CR))
    fe.chan_fsk4(c, **p25.fsk4_params(CR))
    fe.chan_agc(c, agc_n, 1.0)
    fe.chan_costas(c, **p25.costas_params(CR))
    fe.chan_clock_mm(c, 25000 / 3600.0)
    if audio:
        host_audio.open_analog_voice(fe, c, 25000)


def _open(nat, n_chans=6, out_capacity=1 << 12, block=1200, audio=True, agc_n=64):
    fe = nat.Frontend(FS, 0.0, device=0, block_capacity=D * block, out_capacity=out_capacity)
    ids = [fe.chan_open(CR, OFFS[k]) for k in range(n_chans)]
    for c in ids:
        _stages(fe, c, audio, agc_n)
    return fe, ids


def _produced(fe, c, what):
    return {"sym": lambda: fe.chan_produced(c), "clock": lambda: fe.chan_clock_produced(c)[0],
            "costas": lambda: fe.chan_costas_state(c)["n_symbols"], "fsk4": lambda: fe.chan_fsk4_state(c)["n_symbols"],
            "audio": lambda: fe.chan_audio_produced(c)[0]}[what]()


@pytest.mark.parametrize("what", WHATS)
def test_batched_read_equals_single_reads(gpu_required, what):
    nat = gpu_required
    x = _signal(D * sum(BLOCKS), 11)
    fe, ids = _open(nat)
    tw, ids_t = _open(nat)
    bare = fe.chan_open(CR, 200e3)                             # a channel without any stage
    tw.chan_open(CR, 200e3)
    lst = ids + [bare, 9999, ids[2]]                           # ... an unknown id, and one listed twice
    read = fe.chan_read_many_plan(lst, what, cap_each=2048)
    got, want = [[] for _ in ids], [[] for _ in ids]
    for a, b in _cuts(BLOCKS):
        fe.push(x[a:b])
        tw.push(x[a:b])
        counts, out = read()
        assert out.dtype == np.float32
        assert list(counts[6:]) == [nat.RCF_ESTATE, nat.RCF_ENOCHAN, nat.RCF_EINVAL]
        for k in range(6):
            assert counts[k] >= 0
            got[k].append(out[k, :counts[k]].copy())
            want[k].append(getattr(tw, SINGLE[what])(ids_t[k]))
    for k in range(6):
        g = np.concatenate(got[k])
        _same(g, np.concatenate(want[k]), (what, k))
        assert len(g) == _produced(fe, ids[k], what) == _produced(tw, ids_t[k], what) > 100
    fe.close()
    tw.close()


@pytest.mark.parametrize("what", ("costas", "audio"))
def test_small_cap_each_and_single_reads_interleaved(gpu_required, what):
    nat = gpu_required
    x = _signal(D * sum(BLOCKS), 12)
    fe, ids = _open(nat, 3)
    tw, ids_t = _open(nat, 3)
    for a, b in _cuts(BLOCKS):
        fe.push(x[a:b])
        tw.push(x[a:b])
    want = [getattr(tw, SINGLE[what])(c) for c in ids_t]
    got = [[] for _ in ids]
    for it in range(1000):
        rows = fe.chan_read_many(ids, what, cap_each=7)
        assert all(r is not None and len(r) <= 7 for r in rows)
        for k, r in enumerate(rows):
            got[k].append(r.copy())
        one = getattr(fe, SINGLE[what])(ids[1], 5) if it % 2 else np.zeros(0, np.float32)   # the single reader in between
        assert len(one) <= 5
        got[1].append(one)
        if not any(len(r) for r in rows) and not len(one):
            break
    for k in range(3):
        _same(np.concatenate(got[k]), want[k], (what, k))
        assert len(want[k]) > 100
    fe.close()
    tw.close()


@pytest.mark.parametrize("what,cap,block,n_blocks", [("sym", 1 << 12, 1200, 5), ("audio", 1 << 12, 1200, 12),
                                                     ("costas", 1 << 8, 150, 14), ("clock", 1 << 8, 150, 14),
                                                     ("fsk4", 1 << 8, 150, 14)])
def test_a_reader_left_behind_gets_what_the_single_reader_gets(gpu_required, what, cap, block, n_blocks):
    nat = gpu_required
    x = _signal(D * block * (n_blocks + 2), 13)
    kw = dict(n_chans=2, out_capacity=cap, block=block, audio=cap > 256, agc_n=64 if cap > 256 else 16)
    fe, ids = _open(nat, **kw)
    tw, ids_t = _open(nat, **kw)
    at = 0
    for phase, n in enumerate((n_blocks, 1, 1)):               # neglect, then block by block again
        for _ in range(n):
            fe.push(x[at:at + D * block])
            tw.push(x[at:at + D * block])
            at += D * block
        if phase == 0:
            assert _produced(tw, ids_t[0], what) > cap         # more than a ring behind
        rows = fe.chan_read_many(ids, what, cap_each=2 * cap)
        for k in range(2):
            w = getattr(tw, SINGLE[what])(ids_t[k])
            _same(rows[k], w, (what, phase, k))
            assert len(w) <= cap and (phase or len(w) > cap // 2)
    fe.close()
    tw.close()


def test_group_read_many_equals_members_alone(gpu_required):
    nat = gpu_required
    xs = [_signal(D * sum(BLOCKS), 20 + m) for m in range(3)]
    fes, ids = zip(*[_open(nat, 2, audio=False) for _ in range(3)])
    tws, ids_t = zip(*[_open(nat, 2, audio=False) for _ in range(3)])
    grp = nat.Group(list(fes))
    pairs = [(m, c) for m in range(3) for c in ids[m]]
    got, want = [[] for _ in pairs], [[] for _ in pairs]
    for a, b in _cuts(BLOCKS):
        grp.push([xs[m][a:b] for m in range(3)])
        for m in range(3):
            tws[m].push(xs[m][a:b])
        for j, r in enumerate(grp.read_many(pairs, "fsk4", cap_each=1024)):
            got[j].append(r)
        for j, (m, _) in enumerate(pairs):
            want[j].append(tws[m].chan_read_fsk4(ids_t[m][j % 2]))
    for j in range(len(pairs)):
        w = np.concatenate(want[j])
        assert len(w) > 100
        _same(np.concatenate(got[j]), w, j)
    grp.close()
    for fe in fes + tws:
        fe.close()


# ------------------------------------------------------------------------------------------------ the pump
def _wait_blocks(pump, n, timeout_s=30.0):
    t_end = time.monotonic() + timeout_s
    while time.monotonic() < t_end:
        st = pump.stats()
        if st["blocks_done"] >= n or not st["running"]:
            return st
        time.sleep(0.002)
    raise AssertionError("the pump did not get to %d blocks: %r" % (n, pump.stats()))


class _Fed:
    """a group of front-ends under a counter-fed pump: the whole stream sits in pinned rings, `feed(k)` counts k blocks
    complete on every member"""

    def __init__(self, nat, n_members, blk, n_blocks, seed, subs, what, out_ring_samples, max_read=16):
        self.nat, self.blk, self.n_blocks, self.G = nat, blk, n_blocks, n_members
        self.xs = [_signal(D * blk * n_blocks, seed + m) for m in range(n_members)]
        self.fes, self.ids = zip(*[_open(nat, 3, block=blk) for _ in range(n_members)])
        self.rings, self.counters = [], []
        for m in range(n_members):
            r = nat.PinnedArray(len(self.xs[m]), np.complex64)
            r.array[:] = self.xs[m]
            self.rings.append(r)
            self.counters.append(np.zeros(1, dtype=np.uint64))
        self.grp = nat.Group(list(self.fes))
        self.pump = nat.Pump(self.grp, self.rings, D * blk, FS, [(m, self.ids[m][k]) for m, k in subs], fmt=nat.FMT_CF32,
                             what=what, out_ring_samples=out_ring_samples, n_blocks=n_blocks, max_read=max_read,
                             written=self.counters, start_delay_s=0.0)

    def feed(self, k, wait=True):
        for c in self.counters:
            c[0] = k
        if wait:
            st = _wait_blocks(self.pump, self.G * k)
            assert st["error"] == 0, st

    def close(self):
        self.pump.stop()
        self.grp.close()
        for fe in self.fes:
            fe.close()
        for r in self.rings:
            r.free()

    def twin(self, m):
        """member m's twin, fed block by block: yields (block index, front-end, channel ids) after each push"""
        tw, ids_t = _open(self.nat, 3, block=self.blk)
        for b in range(self.n_blocks):
            tw.push(self.xs[m][D * self.blk * b: D * self.blk * (b + 1)])
            yield b, tw, ids_t
        tw.close()


def test_pump_delivers_every_stage_stream_whole(gpu_required):
    nat = gpu_required
    n_blocks = 8
    f = _Fed(nat, 3, 500, n_blocks, 30, [(0, 0), (1, 0), (2, 0)], "costas", 1 << 13)
    pump = f.pump
    slots = {(m, 0, "costas"): m for m in range(3)}
    f.feed(2)
    for m, k, what in ((0, 1, "clock"), (1, 1, "fsk4"), (2, 1, "sym"), (0, 2, "audio"), (1, 2, "agc"), (2, 2, "costas")):
        slots[(m, k, what)] = pump.subscribe(m, f.ids[m][k], what)
    assert len(set(slots.values())) == 9
    start = {key: pump._cursors[e].value for key, e in slots.items()}
    f.feed(n_blocks, wait=False)
    st = pump.wait(timeout_s=30.0)
    assert not st["running"] and st["error"] == 0 and st["blocks_done"] == 3 * n_blocks, st
    got = {key: pump.read(e) for key, e in slots.items()}
    written = {key: pump.written(e) for key, e in slots.items()}
    f.close()
    want = {key: [] for key in slots}
    for m in range(3):
        for b, tw, ids_t in f.twin(m):
            for (m_, k, what) in slots:
                if m_ == m:
                    want[(m_, k, what)].append(getattr(tw, SINGLE[what])(ids_t[k]))
    for key in slots:
        w = np.concatenate(want[key])
        # (every channel's reader stood at its stream's first item when it was subscribed, and the device ring still held it)
        assert start[key] == 0 and written[key] == len(w) > 300, key
        _same(got[key], w, key)


def test_pump_small_host_ring_and_a_reader_that_sleeps(gpu_required):
    nat = gpu_required
    n_blocks = 40
    f = _Fed(nat, 2, 200, n_blocks, 40, [(0, 0), (1, 0), (1, 2)], "costas", 64)   # ~40 symbols per block into rings of 64
    pump = f.pump
    runs = {e: [] for e in range(3)}

    def drain():
        for e in range(3):
            before = pump._cursors[e].value
            r = pump.read(e, 1 << 10)
            runs[e].append((before, pump._cursors[e].value, r))

    for k in range(4, n_blocks + 1, 4):
        f.feed(k, wait=False)
        time.sleep(0.003)
        drain()
    st = pump.wait(timeout_s=30.0)
    assert not st["running"] and st["error"] == 0 and st["blocks_done"] == 2 * n_blocks, st
    drain()
    written = [pump.written(e) for e in range(3)]
    f.close()
    want = {}
    for m in range(2):
        acc = {0: [], 2: []}
        for b, tw, ids_t in f.twin(m):
            for k in acc:
                acc[k].append(tw.chan_read_costas(ids_t[k]))
        want[m] = {k: np.concatenate(v) for k, v in acc.items()}
    for e, (m, k) in enumerate(((0, 0), (1, 0), (1, 2))):
        w = want[m][k]
        assert written[e] == len(w) > 1000
        last = 0
        for before, after, r in runs[e]:
            assert before == last and after - len(r) >= before    # runs neither overlap nor go backwards
            _same(r, w[after - len(r):after], (e, before, after))  # whatever was dropped, what came is the stream there
            last = after
        assert last == len(w) and sum(len(r) for _, _, r in runs[e]) > 0


def test_pump_stage_replaced_and_switched_off_under_a_subscription(gpu_required):
    nat = gpu_required
    n_blocks = 9
    f = _Fed(nat, 2, 500, n_blocks, 50, [(0, 0), (1, 0)], "costas", 1 << 12)
    pump = f.pump
    f.feed(3)
    f.fes[0].chan_costas(f.ids[0][0], **p25.costas_params(CR))           # attached again: a fresh ring, symbol 0
    f.feed(6)
    f.fes[0].chan_costas(f.ids[0][0], None)                              # off: the slot starves, the pump goes on
    f.feed(n_blocks, wait=False)
    st = pump.wait(timeout_s=30.0)
    assert not st["running"] and st["error"] == 0 and st["blocks_done"] == 2 * n_blocks, st
    got = [pump.read(e) for e in range(2)]
    written = [pump.written(e) for e in range(2)]
    f.close()
    want0 = []
    for b, tw, ids_t in f.twin(0):
        if b < 6:
            want0.append(tw.chan_read_costas(ids_t[0]))
        if b == 2:
            tw.chan_costas(ids_t[0], **p25.costas_params(CR))
        if b == 5:
            tw.chan_costas(ids_t[0], None)
    want1 = [tw.chan_read_costas(ids_t[0]) for b, tw, ids_t in f.twin(1)]
    assert len(want0[3]) > 50 and len(want1[8]) > 50
    for e, w in enumerate((np.concatenate(want0), np.concatenate(want1))):
        assert written[e] == len(w)
        _same(got[e], w, e)


def test_pump_slot_passes_from_a_counted_tenant_to_the_next(gpu_required):
    """one slot, three tenants: soft symbols, then -- taken over while gathers of the first may still be in flight -- another
    loop's, then plain IQ.  Each new stream begins at the cursor its subscription returned and is whole from there."""
    nat = gpu_required
    n_blocks = 6
    f = _Fed(nat, 1, 500, n_blocks, 60, [(0, 0)], "costas", 1 << 12, max_read=1)
    pump = f.pump
    f.feed(1)
    f.feed(2, wait=False)                                     # (no wait: the hand-over meets whatever is in flight)
    a = pump.read(0)
    pump.unsubscribe(0)
    assert pump.subscribe(0, f.ids[0][1], "fsk4") == 0
    at_b = pump._cursors[0].value
    assert at_b >= len(a)
    f.feed(4)
    b = pump.read(0)
    assert pump.written(0) == at_b + len(b)
    pump.unsubscribe(0)
    assert pump.subscribe(0, f.ids[0][2], "iq") == 0
    at_c = pump._cursors[0].value
    assert at_c == at_b + len(b)                              # nothing in flight: the count is exact again
    f.feed(n_blocks, wait=False)
    st = pump.wait(timeout_s=30.0)
    assert st["error"] == 0 and st["blocks_done"] == n_blocks, st
    c = pump.read(0)
    assert pump.written(0) == at_c + len(c)
    f.close()
    want = {"costas": [], "fsk4": [], "iq": []}
    for blk, tw, ids_t in f.twin(0):
        want["costas"].append(tw.chan_read_costas(ids_t[0]))
        if blk < 4:
            want["fsk4"].append(tw.chan_read_fsk4(ids_t[1]))
        want["iq"].append(tw.chan_read_iq(ids_t[2]))
    wa = np.concatenate(want["costas"])
    assert len(want["costas"][0]) <= len(a) <= len(wa)        # block 0 was delivered, block 1 perhaps
    _same(a, wa[:len(a)], "costas")
    _same(b, np.concatenate(want["fsk4"]), "fsk4")
    _same(c, np.concatenate(want["iq"]), "iq")


def test_refusals_and_the_new_values_of_what(gpu_required):
    nat = gpu_required
    lib = nat.lib()
    fe, ids = _open(nat, 1)
    cid = (ctypes.c_int * 1)(ids[0])
    cnt = (ctypes.c_int64 * 1)()
    buf = np.zeros(64, dtype=np.complex64)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    for what in list(range(3, 16)) + [21, -1]:
        assert lib.rcf_chan_read_many(fe._h, what, cid, 1, 1.0, ptr, 16, cnt) == nat.RCF_EINVAL, what
    for what in (nat.READ_SYM, nat.READ_CLOCK, nat.READ_COSTAS, nat.READ_FSK4, nat.READ_AUDIO):
        assert lib.rcf_chan_read_many(fe._h, what, cid, 1, 1.0, ptr, 16, cnt) == nat.RCF_OK, what
        assert cnt[0] == 0
    fe.close()
    # the pump: 3 is no stream, a bin of the fused discriminator ring stays RCF_READ_FM
    from oracle import grspec as G
    fs = 5e6
    Dp, taps = G.channel_params(fs, 12500)
    blk = Dp * 100
    fe = nat.Frontend(fs, 0.0, device=0, block_capacity=blk, hist_capacity=1 << 14, out_capacity=1 << 12)
    fe.pfb_open(2 * Dp, Dp, taps)
    c = fe.pfb_tap_open(7, gr_phase=True)
    fe.pfb_fm_enable(1, gr_phase=True)
    ring = nat.PinnedArray(2 * 2 * blk, np.uint8)
    ring.array[:] = 127
    counter = np.zeros(1, dtype=np.uint64)
    grp = nat.Group([fe])
    pump = nat.Pump(grp, [ring], blk, fs, (), fmt=nat.FMT_U8, what="costas", max_read=4, written=[counter], start_delay_s=0.0)
    cur = ctypes.c_int64(0)
    assert lib.rcf_pump_subscribe(pump._p, 0, c, 3, 1.0, ctypes.byref(cur)) == nat.RCF_EINVAL
    for what in (nat.READ_COSTAS, nat.READ_AUDIO, nat.READ_AGC, nat.READ_IQ):
        assert lib.rcf_pump_subscribe(pump._p, 0, nat.SRC_PFB_BIN0 + 5, what, 1.0, ctypes.byref(cur)) == nat.RCF_EINVAL, what
    assert lib.rcf_pump_subscribe(pump._p, 0, nat.SRC_PFB_BIN0 + 5, nat.READ_FM, 1.0, ctypes.byref(cur)) >= 0
    for what in (nat.READ_AGC, nat.READ_SYM, nat.READ_AUDIO):
        assert lib.rcf_pump_subscribe(pump._p, 0, c, what, 1.0, ctypes.byref(cur)) >= 0, what
    pump.stop()
    grp.close()
    fe.close()
    ring.free()
