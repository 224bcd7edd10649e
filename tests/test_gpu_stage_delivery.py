"""The stages' streams -- symbol filter, the three symbol loops' soft symbols, the voice chain's audio -- through the batched
readers (rcf_chan_read_many / rcf_group_read_many, RCF_READ_SYM .. RCF_READ_AUDIO) and the real-time pump.  How many items
a loop or the voice chain has produced only the device knows; the counted gather (ingest.hip) reads the counter itself.
The yardstick is always a twin front-end fed the same samples and read with the single readers (rcf_chan_read_sym / _clock
/ _costas / _fsk4 / _audio): equality is of bits.  Where a slot does not carry the whole stream -- a host ring smaller than a
block's output, a subscription that begins past item 0 -- tests/delivery_ref.py, a restatement of the gather's documented
rule in integers, says which items of the twin's stream it must hold."""
import ctypes
import json
import os
import time

import numpy as np
import pytest

import delivery_ref as R
from rcf import audio as host_audio
from rcf import p25, synth

pytestmark = pytest.mark.gpu

FS, CR, D = 2.4e6, 12500, 96                       # 12.5 kHz channels: decimation 96, 25 kS/s
BLOCKS = (500, 37, 1, 1200)                        # channel samples per block
OFFS = [-62500.0 + 25000.0 * k for k in range(10)]
OFFS_MANY = [-190000.0 + 2900.0 * k for k in range(130)]     # the loops' three-wave shape (test_130_channels_* of each loop)
WHATS = ("sym", "clock", "costas", "fsk4", "audio")
SINGLE = {"sym": "chan_read_sym", "clock": "chan_read_clock", "costas": "chan_read_costas", "fsk4": "chan_read_fsk4",
          "audio": "chan_read_audio", "agc": "chan_read_agc"}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32)


def _same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(_bits(got), _bits(want)), what


def _signal(n, seed, fs=FS, carriers=None):
    rng = np.random.default_rng(seed)
    x = synth.awgn(rng, n).astype(np.complex128)
    for k, f in enumerate([OFFS[0], OFFS[2], OFFS[3]] if carriers is None else carriers):
        x += synth.nbfm_carrier(n, fs, f, 600.0 + 170 * [0, 2, 3, 1, 4, 5][k % 6], 2500.0, synth.snr_amp(25.0, 12500.0, fs))
    return x.astype(np.complex64)


def _cuts(blocks):
    at = np.concatenate([[0], np.cumsum([D * b for b in blocks])])
    return list(zip(at[:-1], at[1:]))


_CHAINS = {}


def _voice(fe, c, rate=25000, **kw):
    """open_analog_voice with the designs (an equiripple low-pass among them) made once per (rate, arguments)"""
    key = (rate,) + tuple(sorted(kw.items()))
    if key not in _CHAINS:
        _CHAINS[key] = host_audio.analog_chain_params(rate, **kw)
    fe.chan_audio_open(c, **_CHAINS[key])
    return _CHAINS[key]["interpolation"], _CHAINS[key]["decimation"]


def _stages(fe, c, audio=True, agc_n=64, cr=CR, loops=("fsk4", "costas", "clock")):
    """every stage on one channel of rate 2 cr: symbol filter + C4FM loop, AGC + Gardner / Costas, symbol clock, voice chain"""
    if "fsk4" in loops:
        fe.chan_fm_filter(c, p25.fm_gain(cr), p25.symbol_taps(cr))
        fe.chan_fsk4(c, **p25.fsk4_params(cr))
    if "costas" in loops:
        fe.chan_agc(c, agc_n, 1.0)
        fe.chan_costas(c, **p25.costas_params(cr))
    if "clock" in loops:
        fe.chan_clock_mm(c, 2 * cr / 3600.0)
    if audio:
        _voice(fe, c, 2 * cr)


def _open(nat, n_chans=6, out_capacity=1 << 12, block=1200, audio=True, agc_n=64, offs=OFFS):
    """audio: True / False, or a function of the channel's index"""
    fe = nat.Frontend(FS, 0.0, device=0, block_capacity=D * block, out_capacity=out_capacity)
    ids = [fe.chan_open(CR, offs[k]) for k in range(n_chans)]
    for k, c in enumerate(ids):
        _stages(fe, c, audio(k) if callable(audio) else audio, agc_n)
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
    """the batched and the single reader take the same path: a third twin, read after every block so that it never lags,
    gives the whole stream, and what the neglected readers get is its last out_capacity items"""
    nat = gpu_required
    x = _signal(D * block * (n_blocks + 2), 13)
    kw = dict(n_chans=2, out_capacity=cap, block=block, audio=cap > 256, agc_n=64 if cap > 256 else 16)
    fe, ids = _open(nat, **kw)
    tw, ids_t = _open(nat, **kw)
    al, ids_a = _open(nat, **kw)
    whole = [[], []]
    at = 0
    for phase, n in enumerate((n_blocks, 1, 1)):               # neglect, then block by block again
        for _ in range(n):
            fe.push(x[at:at + D * block])
            tw.push(x[at:at + D * block])
            al.push(x[at:at + D * block])
            at += D * block
            for k in range(2):
                whole[k].append(getattr(al, SINGLE[what])(ids_a[k]))
        if phase == 0:
            assert _produced(tw, ids_t[0], what) > cap         # more than a ring behind
        rows = fe.chan_read_many(ids, what, cap_each=2 * cap)
        for k in range(2):
            w = getattr(tw, SINGLE[what])(ids_t[k])
            _same(rows[k], w, (what, phase, k))
            assert len(w) <= cap and (phase or len(w) > cap // 2)
            if phase == 0:
                so_far = np.concatenate(whole[k])
                assert len(so_far) == _produced(al, ids_a[k], what) > cap
                _same(rows[k], so_far[-cap:], (what, "batched, the ring's last items", k))
                _same(w, so_far[-cap:], (what, "single, the ring's last items", k))
    fe.close()
    tw.close()
    al.close()


@pytest.mark.parametrize("what", WHATS)
def test_group_read_many_equals_members_alone(gpu_required, what):
    """every stream through rcf_group_read_many, voice chains on; a pair with a member index out of range and a pair listed
    twice sit BETWEEN valid pairs and answer None without moving the rows behind them"""
    nat = gpu_required
    xs = [_signal(D * sum(BLOCKS), 20 + m) for m in range(3)]
    fes, ids = zip(*[_open(nat, 2) for _ in range(3)])
    tws, ids_t = zip(*[_open(nat, 2) for _ in range(3)])
    grp = nat.Group(list(fes))
    # (member, channel index) or a refused pair
    layout = [(0, 0), (0, 1), "member", (1, 0), (1, 1), "twice", (2, 0), (2, 1)]
    pairs = [(7, ids[0][0]) if p == "member" else (1, ids[1][0]) if p == "twice" else (p[0], ids[p[0]][p[1]]) for p in layout]
    got, want = [[] for _ in pairs], [[] for _ in pairs]
    for a, b in _cuts(BLOCKS):
        grp.push([xs[m][a:b] for m in range(3)])
        for m in range(3):
            tws[m].push(xs[m][a:b])
        rows = grp.read_many(pairs, what, cap_each=2048)       # (a block of 1200 gives the symbol filter 1200)
        assert len(rows) == len(pairs)
        for j, p in enumerate(layout):
            if isinstance(p, str):
                assert rows[j] is None, (what, j, p)
                continue
            assert rows[j] is not None and rows[j].dtype == np.float32, (what, j)
            got[j].append(rows[j])
            want[j].append(getattr(tws[p[0]], SINGLE[what])(ids_t[p[0]][p[1]]))
    for j, p in enumerate(layout):
        if isinstance(p, str):
            continue
        w = np.concatenate(want[j])
        assert len(w) > 100
        _same(np.concatenate(got[j]), w, (what, j))
        assert len(w) == _produced(tws[p[0]], ids_t[p[0]][p[1]], what) == _produced(fes[p[0]], ids[p[0]][p[1]], what)
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

    def __init__(self, nat, n_members, blk, n_blocks, seed, subs, what, out_ring_samples, max_read=16, opener=None, pre=0,
                 fs=FS, dec=D, signal=_signal):
        """opener(nat) -> (front-end, channel ids): a member, and its twin (default: three channels with every stage);
        pre: blocks of the n_blocks that go through Group.push BEFORE the pump exists; a block is blk * dec input samples"""
        self.nat, self.blk, self.n_blocks, self.G, self.dec = nat, blk, n_blocks, n_members, dec
        self.opener = opener if opener is not None else (lambda nat_: _open(nat_, 3, block=blk))
        self.xs = [signal(dec * blk * n_blocks, seed + m) for m in range(n_members)]
        self.fes, self.ids = zip(*[self.opener(nat) for _ in range(n_members)])
        self.rings, self.counters = [], []
        for m in range(n_members):
            rest = self.xs[m][dec * blk * pre:]
            r = nat.PinnedArray(len(rest), np.complex64)
            r.array[:] = rest
            self.rings.append(r)
            self.counters.append(np.zeros(1, dtype=np.uint64))
        self.grp = nat.Group(list(self.fes))
        for b in range(pre):
            self.grp.push([x[dec * blk * b: dec * blk * (b + 1)] for x in self.xs])
        self.pump = nat.Pump(self.grp, self.rings, dec * blk, fs, [(m, self.ids[m][k]) for m, k in subs], fmt=nat.FMT_CF32,
                             what=what, out_ring_samples=out_ring_samples, n_blocks=n_blocks - pre, max_read=max_read,
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
        tw, ids_t = self.opener(self.nat)
        for b in range(self.n_blocks):
            tw.push(self.xs[m][self.dec * self.blk * b: self.dec * self.blk * (b + 1)])
            yield b, tw, ids_t
        tw.close()

    def twin_streams(self, m, keys):
        """member m's twin over all blocks, for keys (channel index, what): the whole stream of each, and the stage's
        device counter after every block (the loops' symbol count; the voice chain's samples behind the squelch)"""
        parts, counters = {key: [] for key in keys}, {key: [] for key in keys}
        for b, tw, ids_t in self.twin(m):
            for (k, what) in keys:
                parts[(k, what)].append(getattr(tw, SINGLE[what])(ids_t[k]))
                counters[(k, what)].append(tw.chan_audio_produced(ids_t[k])[1] if what == "audio" else _produced(tw, ids_t[k], what))
        return {key: np.concatenate(v) for key, v in parts.items()}, counters


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


# ------------------------------------------------------------------------------------------------ the batched readers, wider
def _codes(nat):
    return {"chan": nat.RCF_ENOCHAN, "state": nat.RCF_ESTATE, "twice": nat.RCF_EINVAL}


def _read_many_raw(nat, fe, lst, what, cap_each, rows):
    """rcf_chan_read_many itself (cap_each = 0 included, which the binding's reshape cannot express) -> counts"""
    ids = (ctypes.c_int * len(lst))(*lst)
    cnt = (ctypes.c_int64 * len(lst))()
    rc = nat.lib().rcf_chan_read_many(fe._h, nat._read_what(what, True), ids, len(lst), 1.0, rows.ctypes.data_as(ctypes.c_void_p),
                                      cap_each, cnt)
    assert rc == nat.RCF_OK, (what, rc)
    return list(cnt)


def test_130_channels_more_records_than_workgroups(gpu_required):
    """130 counted records in one launch of at most 128 workgroups: with one part per record (cap_each 256) workgroups 0 and
    1 take a second record, with two parts (cap_each 512) every workgroup takes a second or third item.  The audio read
    lists all 130 channels, of which 26 carry a chain: the records are numbered past the refused entries between them."""
    nat = gpu_required
    t0 = time.monotonic()
    x = _signal(D * sum(BLOCKS), 70)
    chained = lambda k: k % 5 == 0
    fe, ids = _open(nat, 130, audio=chained, offs=OFFS_MANY)
    tw, ids_t = _open(nat, 130, audio=chained, offs=OFFS_MANY)
    whats = ("clock", "costas", "fsk4", "audio")
    plans = {(what, cap): fe.chan_read_many_plan(ids, what, cap_each=cap) for what in whats for cap in (256, 512)}
    got = {what: [[] for _ in ids] for what in whats}
    want = {what: [[] for _ in ids] for what in whats}

    def read(what, cap):
        counts, out = plans[(what, cap)]()
        for k in range(130):
            if what == "audio" and not chained(k):
                assert counts[k] == nat.RCF_ESTATE, (what, k, counts[k])
                continue
            assert 0 <= counts[k] <= cap, (what, k, counts[k])
            got[what][k].append(out[k, :counts[k]].copy())
        return int(sum(c for c in counts if c > 0))

    for blk, (a, b) in enumerate(_cuts(BLOCKS)):
        fe.push(x[a:b])
        tw.push(x[a:b])
        cap = 256 if blk % 2 == 0 else 512                     # the first and third block one part, the others two
        for what in whats:
            read(what, cap)
            for k in range(130):
                if what != "audio" or chained(k):
                    want[what][k].append(getattr(tw, SINGLE[what])(ids_t[k]))
    while read("audio", 512):                                  # (1200 channel samples are 384 of audio: a rest may be left)
        pass
    for what in whats:
        for k in range(130):
            if what == "audio" and not chained(k):
                continue
            w = np.concatenate(want[what][k])
            _same(np.concatenate(got[what][k]), w, (what, k))
            assert len(w) == _produced(tw, ids_t[k], what) > 100, (what, k, len(w))
            if what != "audio":                                # a loop's block fits its row: call by call the twin's read
                assert [len(g) for g in got[what][k]] == [len(v) for v in want[what][k]], (what, k)
    assert got["costas"][0][0].tobytes() != got["costas"][129][0].tobytes()
    fe.close()
    tw.close()
    print("    130 channels, four streams, four blocks: %.2f s" % (time.monotonic() - t0))


@pytest.mark.parametrize("what,blocks", [("costas", (1200,) * 17), ("audio", (1200,) * 10 + (40,))])
def test_all_16_parts_of_a_row_carry_data(gpu_required, what, blocks):
    """rows of more than 3840 items: the launch splits a record into 16 parts of 256 lanes and every part has work -- 9
    records x 16 parts = 144 items on 128 workgroups"""
    nat = gpu_required
    x = _signal(D * sum(blocks), 71)
    fe, ids = _open(nat, 9, out_capacity=4096)
    tw, ids_t = _open(nat, 9, out_capacity=4096)
    for a, b in _cuts(blocks):
        fe.push(x[a:b])
        tw.push(x[a:b])
    rows = fe.chan_read_many(ids, what, cap_each=4096)
    for k in range(9):
        w = getattr(tw, SINGLE[what])(ids_t[k])
        assert 3840 < len(w) <= 4096, (what, k, len(w))
        _same(rows[k], w, (what, k))
        assert len(w) == _produced(tw, ids_t[k], what)
    assert all(len(r) == 0 for r in fe.chan_read_many(ids, what, cap_each=4096))
    fe.close()
    tw.close()


@pytest.mark.parametrize("what", WHATS)
def test_refused_entries_between_counted_entries(gpu_required, what):
    """an unknown id, a channel without stages, a channel listed twice and a channel whose Costas stage was switched off, each
    BETWEEN entries that are read: the refused positions carry their codes, every other row -- at its own position -- is
    the twin's single read.  A call with cap_each = 0 reads nothing and moves no cursor."""
    nat = gpu_required
    E = _codes(nat)
    x = _signal(D * sum(BLOCKS), 72)

    def opened():
        fe, ids = _open(nat, 9)
        fe.chan_costas(ids[8], None)                          # `off`: every stage but the Costas loop
        return fe, ids[:8], fe.chan_open(CR, 200e3), ids[8]
    fe, c, bare, off = opened()
    tw, c_t, bare_t, off_t = opened()
    layout = [0, "chan", 1, "state", 2, "twice", 3, "off", 4, 5, 6, 7]
    lst = [9999 if p == "chan" else bare if p == "state" else c[1] if p == "twice" else off if p == "off" else c[p] for p in layout]
    read = fe.chan_read_many_plan(lst, what, cap_each=2048)
    rows0 = np.zeros((len(lst), 8), dtype=np.float32)
    got, want = {}, {}
    for blk, (a, b) in enumerate(_cuts(BLOCKS)):
        fe.push(x[a:b])
        tw.push(x[a:b])
        if blk == 0:                                           # every channel's reader at a place of its own: 3 + k items in
            for j, p in enumerate(layout):                     # (equal counts and cursors would hide a swap of result words)
                if isinstance(p, int):
                    head, head_t = getattr(fe, SINGLE[what])(c[p], 3 + p), getattr(tw, SINGLE[what])(c_t[p], 3 + p)
                    assert len(head) == 3 + p
                    _same(head, head_t, (what, "head", p))
                    got.setdefault(j, []).append(head)
                    want.setdefault(j, []).append(head_t)
        if blk == 1:                                           # nothing asked for: nothing read, and the read below is whole
            counts0 = _read_many_raw(nat, fe, lst, what, 0, rows0)
            for j, p in enumerate(layout):
                refused = E.get(p, E["state"] if (p == "off" and what == "costas") else None)
                assert counts0[j] == (0 if refused is None else refused), (what, j, p, counts0[j])
        counts, out = read()
        for j, p in enumerate(layout):
            if p in E or (p == "off" and what == "costas"):
                assert counts[j] == E.get(p, E["state"]), (what, j, p, counts[j])
                continue
            w = getattr(tw, SINGLE[what])(off_t if p == "off" else c_t[p])
            _same(out[j, :counts[j]], w, (what, blk, j, p))
            got.setdefault(j, []).append(out[j, :counts[j]].copy())
            want.setdefault(j, []).append(w)
    assert sorted(got) == [j for j, p in enumerate(layout) if not (p in E or (p == "off" and what == "costas"))]
    for j in got:
        assert len(np.concatenate(want[j])) > 100, (what, j)
    k_of = {j: p for j, p in enumerate(layout) if isinstance(p, int)}
    for j, k in k_of.items():
        assert len(np.concatenate(got[j])) == _produced(fe, c[k], what) == _produced(tw, c_t[k], what)
    fe.close()
    tw.close()


def test_count_transforms_of_four_resamplers(gpu_required):
    """four voice chains in one launch, each with its own count transform: 8/25, 441/1000, 48/25 (more out than in: the DSD
    feed) and 1/1, which takes the kernel's branch for interp == decim"""
    nat = gpu_required
    x = _signal(D * sum(BLOCKS), 73)
    ratios = {}

    def opened():
        fe = nat.Frontend(FS, 0.0, device=0, block_capacity=D * 1200, out_capacity=1 << 12)
        ids = [fe.chan_open(CR, OFFS[k]) for k in range(4)]
        ratios[0] = _voice(fe, ids[0], 25000, audio_rate=8000)
        ratios[1] = _voice(fe, ids[1], 25000, audio_rate=11025)
        feed = host_audio.dsd_feed_params(25000, 0.4)
        fe.chan_audio_open(ids[2], **feed)
        ratios[2] = (feed["interpolation"], feed["decimation"])
        ratios[3] = _voice(fe, ids[3], 25000, audio_rate=25000)      # design_resampler(25000, 25000) is 1 / 1
        return fe, ids
    fe, ids = opened()
    tw, ids_t = opened()
    assert [ratios[k] for k in range(4)] == [(8, 25), (441, 1000), (48, 25), (1, 1)]
    f7, ids7 = opened()                                         # the same streams again, drained seven at a time
    got, want = [[] for _ in ids], [[] for _ in ids]
    for a, b in _cuts(BLOCKS):
        for h in (fe, tw, f7):
            h.push(x[a:b])
        for k, r in enumerate(fe.chan_read_many(ids, "audio", cap_each=2048)):
            got[k].append(r.copy())
        for k in range(4):
            want[k].append(tw.chan_read_audio(ids_t[k]))
    for k, r in enumerate(fe.chan_read_many(ids, "audio", cap_each=2048)):      # (1200 samples at 48/25 are 2304: a rest)
        got[k].append(r.copy())
    small = [[] for _ in ids]
    for it in range(2000):
        rows = f7.chan_read_many(ids7, "audio", cap_each=7)
        assert all(r is not None and len(r) <= 7 for r in rows)
        for k, r in enumerate(rows):
            small[k].append(r.copy())
        if not any(len(r) for r in rows):
            break
    n_in = sum(BLOCKS)
    for k in range(4):
        w = np.concatenate(want[k])
        i, d = ratios[k]
        n_audio, n_ungated = tw.chan_audio_produced(ids_t[k])
        assert n_audio == R.stream_end(n_ungated, i, d) == len(w) > 100 and n_ungated <= n_in, (k, n_audio, n_ungated)
        _same(np.concatenate(got[k]), w, ("cap 2048", k))
        _same(np.concatenate(small[k]), w, ("cap 7", k))
        assert fe.chan_audio_produced(ids[k])[0] == f7.chan_audio_produced(ids7[k])[0] == len(w)
    assert len(np.concatenate(want[2])) > n_in > len(np.concatenate(want[0]))      # more out than in, fewer out than in
    for h in (fe, tw, f7):
        h.close()


# ---- other kinds of channel: the smallest frame-major bank with a stage-2 channel and a tap, direct channels of three rates
FS_B, NB_B, D_B = 2.0e6, 160, 80                             # 160 bins 12.5 kHz apart, 25 kS/s each
KINDS = ("stage2", "tap", "direct25", "direct12", "direct6")
F_KINDS = {"stage2": 9 * FS_B / NB_B, "tap": 5 * FS_B / NB_B, "direct25": -100e3, "direct12": -50e3, "direct6": -25e3}
# the streams a kind of channel carries here (the tap: symbol filter + C4FM loop + symbol clock)
HAS = {kind: WHATS if kind != "tap" else ("sym", "clock", "fsk4") for kind in KINDS}


def _signal_b(n, seed):
    return _signal(n, seed, fs=FS_B, carriers=[F_KINDS[k] + 150.0 for k in KINDS])


def _open_kinds(nat, block=1200):
    from oracle import grspec as G
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pfb_shapes.json")))
    col = {name: i for i, name in enumerate(g["columns"])}
    assert (NB_B, D_B) == min((r[col["NB"]], r[col["D"]]) for r in g["rows"] if r[col["supported"]] and r[col["frame_major"]])
    d_, proto = G.channel_params(FS_B, CR)
    assert d_ == D_B
    fe = nat.Frontend(FS_B, 0.0, device=0, block_capacity=D_B * block, hist_capacity=1 << 14, out_capacity=1 << 13)
    fe.pfb_open(NB_B, D_B, proto)
    ids = [fe.pfb_chan_open(9, CR, 0.0), fe.pfb_tap_open(5, gr_phase=True), fe.chan_open(25000, F_KINDS["direct25"]),
           fe.chan_open(12500, F_KINDS["direct12"]), fe.chan_open(6250, F_KINDS["direct6"])]
    _stages(fe, ids[0])                                       # (output rates: 25, 25, 50, 25 and 12.5 kS/s)
    _stages(fe, ids[1], audio=False, loops=("fsk4", "clock"))
    _stages(fe, ids[2], cr=25000)
    _stages(fe, ids[3])
    _stages(fe, ids[4], cr=6250)
    return fe, ids


@pytest.mark.parametrize("what", WHATS)
def test_stage2_channel_tap_and_three_direct_rates_in_one_launch(gpu_required, what):
    nat = gpu_required
    x = _signal_b(D_B * sum(BLOCKS), 74)
    fe, ids = _open_kinds(nat)
    tw, ids_t = _open_kinds(nat)
    read = fe.chan_read_many_plan(ids, what, cap_each=4096)
    got, want = [[] for _ in ids], [[] for _ in ids]
    at = np.concatenate([[0], np.cumsum([D_B * b for b in BLOCKS])])
    for a, b in zip(at[:-1], at[1:]):
        fe.push(x[a:b])
        tw.push(x[a:b])
        counts, out = read()
        for k, kind in enumerate(KINDS):
            if what not in HAS[kind]:
                assert counts[k] == nat.RCF_ESTATE, (what, kind, counts[k])
                continue
            w = getattr(tw, SINGLE[what])(ids_t[k])
            _same(out[k, :counts[k]], w, (what, kind))
            got[k].append(out[k, :counts[k]].copy())
            want[k].append(w)
    lens = {}
    for k, kind in enumerate(KINDS):
        if what in HAS[kind]:
            lens[kind] = len(np.concatenate(want[k]))
            assert lens[kind] == _produced(fe, ids[k], what) == _produced(tw, ids_t[k], what) > 100, (what, kind, lens[kind])
    if what == "sym":                                          # three rates rode in the launch
        assert lens["direct25"] > 1.9 * lens["direct12"] > 3.7 * lens["direct6"]
    fe.close()
    tw.close()


# ------------------------------------------------------------------------------------------------ the pump, wider
def _ratio(what, interp=8, decim=25):
    return (interp, decim) if what == "audio" else (1, 1)


def _bounds(what, n_k, n_blocks, interp=8, decim=25):
    """the host's steady-state bound of every block's gather ("The rule of one gather")"""
    return [R.audio_bound(n_k, interp, decim) if what == "audio" else R.loop_bound(n_k)] * n_blocks


def test_pump_host_ring_smaller_than_a_blocks_output(gpu_required):
    """rings of 64 under blocks that make about 96 soft symbols and 160 audio samples: every gather skips, and the slot
    receives what tests/delivery_ref.py says -- each block's newest items at consecutive positions, `written` counting the
    items delivered"""
    nat = gpu_required
    n_blocks, blk, room = 12, 500, 64
    keys = [(0, "costas"), (1, "audio"), (1, "costas"), (0, "audio")]
    f = _Fed(nat, 1, blk, n_blocks, 80, [(0, 0)], "costas", room, opener=lambda nat_: _open(nat_, 2, block=blk))
    reads, written = {key: [] for key in keys}, {key: [] for key in keys}
    try:
        pump = f.pump
        slots = {keys[0]: 0}
        for k, what in keys[1:]:
            slots[(k, what)] = pump.subscribe(0, f.ids[0][k], what)
        assert sorted(slots.values()) == [0, 1, 2, 3]
        for b in range(n_blocks):
            f.feed(b + 1)
            for key, e in slots.items():
                reads[key].append(pump.read(e))
                written[key].append(pump.written(e))
    finally:
        f.close()
    streams, counters = f.twin_streams(0, keys)
    for key in keys:
        i, d = _ratio(key[1])
        idx, _, per, w = R.replay_slot(streams[key], counters[key], _bounds(key[1], blk, n_blocks), cap=1 << 12, room=room,
                                       interp=i, decim=d)
        assert len(idx) < len(streams[key]) and len(idx) > 5 * room, key          # something was skipped, much was delivered
        total = 0
        for b, (cur, n) in enumerate(per):
            total += n
            assert written[key][b] == total, (key, b, written[key][b], total)
            _same(reads[key][b], streams[key][cur:cur + n], (key, b, cur, n))
            assert cur + n == R.stream_end(counters[key][b], i, d)                 # the block's NEWEST items
        assert w == total


@pytest.mark.parametrize("what", ("costas", "audio"))
def test_pump_started_on_a_group_that_has_processed_blocks(gpu_required, what):
    """three blocks go through Group.push before the pump exists: a subscription given to rcf_pump_start begins at the
    stream's end at that moment"""
    nat = gpu_required
    n_blocks, pre, blk = 8, 3, 500
    f = _Fed(nat, 1, blk, n_blocks, 81, [(0, 1)], what, 1 << 13, opener=lambda nat_: _open(nat_, 2, block=blk), pre=pre)
    try:
        f.feed(n_blocks - pre, wait=False)
        st = f.pump.wait(timeout_s=30.0)
        assert not st["running"] and st["error"] == 0 and st["blocks_done"] == n_blocks - pre, st
        got, written = f.pump.read(0), f.pump.written(0)
    finally:
        f.close()
    streams, counters = f.twin_streams(0, [(1, what)])
    s, c = streams[(1, what)], counters[(1, what)]
    i, d = _ratio(what)
    start = R.stream_end(c[pre - 1], i, d)
    idx, _, _, w = R.replay_slot(s, c, _bounds(what, blk, n_blocks), cap=1 << 12, room=1 << 13, interp=i, decim=d, first=pre,
                                 cursor0=start)
    assert 0 < start == idx[0] and idx == list(range(start, len(s))) and len(idx) > 300, (what, start, len(s))
    assert written == w == len(s) - start
    _same(got, s[start:], what)


def test_pump_subscription_on_a_channel_whose_reader_stands_part_way(gpu_required):
    nat = gpu_required
    n_blocks, blk = 8, 500
    f = _Fed(nat, 1, blk, n_blocks, 82, [(0, 0)], "costas", 1 << 12, opener=lambda nat_: _open(nat_, 2, block=blk))
    try:
        pump = f.pump
        f.feed(2)
        head = f.fes[0].chan_read_fsk4(f.ids[0][1], 50)         # the single reader takes 50 symbols; the pump is idle
        e = pump.subscribe(0, f.ids[0][1], "fsk4")
        assert e == 1 and pump._cursors[e].value == 0
        f.feed(n_blocks, wait=False)
        st = pump.wait(timeout_s=30.0)
        assert not st["running"] and st["error"] == 0 and st["blocks_done"] == n_blocks, st
        got, written = pump.read(e), pump.written(e)
        whole, written0 = pump.read(0), pump.written(0)
    finally:
        f.close()
    streams, counters = f.twin_streams(0, [(1, "fsk4"), (0, "costas")])
    s, c = streams[(1, "fsk4")], counters[(1, "fsk4")]
    assert len(head) == 50 < c[1]
    _same(head, s[:50], "head")
    idx, _, _, w = R.replay_slot(s, c, _bounds("fsk4", blk, n_blocks), cap=1 << 12, room=1 << 12, first=2, cursor0=len(head))
    assert 0 < idx[0] == 50 and idx == list(range(50, len(s))) and len(idx) > 300
    assert written == w == len(s) - 50
    _same(got, s[50:], "from the reader on")
    _same(whole, streams[(0, "costas")], "the start subscription beside it")
    assert written0 == len(whole)


def test_pump_subscription_on_a_stream_whose_device_ring_has_wrapped(gpu_required):
    """device rings of 256 and a channel nobody has read: 20 blocks make about 576 soft symbols before the subscription, so
    its first gather -- bounded by the device ring, not by a block's output -- starts at end - 256 and the stream goes on
    from there without a hole.  (Blocks of 150 channel samples: rings of 256 refuse a block of 500 with RCF_ECAP.)"""
    nat = gpu_required
    n_blocks, late, blk, cap = 24, 20, 150, 256
    opener = lambda nat_: _open(nat_, 2, out_capacity=cap, block=blk, audio=False, agc_n=16)
    f = _Fed(nat, 1, blk, n_blocks, 83, [(0, 0)], "costas", 1 << 12, opener=opener)
    try:
        pump = f.pump
        f.feed(late)
        e = pump.subscribe(0, f.ids[0][1], "costas")
        f.feed(n_blocks, wait=False)
        st = pump.wait(timeout_s=30.0)
        assert not st["running"] and st["error"] == 0 and st["blocks_done"] == n_blocks, st
        got, written = pump.read(e), pump.written(e)
        whole, written0 = pump.read(0), pump.written(0)
    finally:
        f.close()
    streams, counters = f.twin_streams(0, [(1, "costas"), (0, "costas")])
    s, c = streams[(1, "costas")], counters[(1, "costas")]
    assert c[late - 1] > cap + 200                             # much more than a ring had gone by
    idx, _, per, w = R.replay_slot(s, c, _bounds("costas", blk, n_blocks), cap=cap, room=1 << 12, first=late, cursor0=0)
    assert per[0] == (c[late] - cap, cap) and 0 < idx[0] == c[late] - cap and idx == list(range(idx[0], len(s)))
    assert written == w == len(idx)
    _same(got, s[idx[0]:], "from end - cap on")
    _same(whole, streams[(0, "costas")], "the start subscription beside it")
    assert written0 == len(whole) > 2 * cap


def test_pump_132_counted_slots_two_blocks_in_flight(gpu_required):
    """more counted records than the gather has workgroups, from two members in one launch: costas, fsk4, clock and audio
    in rotation over 2 x 66 channels (the costas slots given at rcf_pump_start, the others subscribed before the first
    block), everything fed at once"""
    nat = gpu_required
    t0 = time.monotonic()
    n_blocks, blk = 6, 500
    chained = lambda k: k % 4 == 3 and k < 40                   # ten voice chains per member
    opener = lambda nat_: _open(nat_, 66, block=blk, audio=chained, offs=OFFS_MANY)
    rot = ("costas", "fsk4", "clock", "audio")
    what_of = [rot[k % 4] if rot[k % 4] != "audio" or chained(k) else "costas" for k in range(66)]
    at_start = [(m, k) for m in range(2) for k in range(66) if what_of[k] == "costas"]
    f = _Fed(nat, 2, blk, n_blocks, 84, at_start, "costas", 1 << 12, max_read=132, opener=opener)
    try:
        pump = f.pump
        slots = {(m, k): e for e, (m, k) in enumerate(at_start)}
        for m in range(2):
            for k in range(66):
                if what_of[k] != "costas":
                    slots[(m, k)] = pump.subscribe(m, f.ids[m][k], what_of[k])
        assert sorted(slots.values()) == list(range(132))
        f.feed(n_blocks, wait=False)
        st = pump.wait(timeout_s=30.0)
        assert not st["running"] and st["error"] == 0 and st["blocks_done"] == 2 * n_blocks, st
        got = {key: pump.read(e) for key, e in slots.items()}
        written = {key: pump.written(e) for key, e in slots.items()}
    finally:
        f.close()
    for m in range(2):
        streams, _ = f.twin_streams(m, [(k, what_of[k]) for k in range(66)])
        for k in range(66):
            w = streams[(k, what_of[k])]
            assert written[(m, k)] == len(w) > 300, (m, k, what_of[k], written[(m, k)], len(w))
            _same(got[(m, k)], w, (m, k, what_of[k]))
    assert sum(w == "audio" for w in what_of) == 10
    print("    132 counted slots, two members, six blocks: %.2f s" % (time.monotonic() - t0))


def test_pump_stage2_channel_tap_and_slow_direct_channel(gpu_required):
    nat = gpu_required
    n_blocks, blk = 8, 500
    f = _Fed(nat, 1, blk, n_blocks, 85, [(0, 0)], "costas", 1 << 13, opener=lambda nat_: _open_kinds(nat_, block=blk),
             fs=FS_B, dec=D_B, signal=_signal_b)
    keys = [(0, "costas"), (0, "audio"), (1, "fsk4"), (1, "clock"), (4, "fsk4")]   # stage-2 channel, tap, 6.25 kHz channel
    try:
        pump = f.pump
        slots = {keys[0]: 0}
        for k, what in keys[1:]:
            slots[(k, what)] = pump.subscribe(0, f.ids[0][k], what)
        f.feed(n_blocks, wait=False)
        st = pump.wait(timeout_s=30.0)
        assert not st["running"] and st["error"] == 0 and st["blocks_done"] == n_blocks, st
        got = {key: pump.read(e) for key, e in slots.items()}
        written = {key: pump.written(e) for key, e in slots.items()}
    finally:
        f.close()
    streams, _ = f.twin_streams(0, keys)
    for key in keys:
        assert written[key] == len(streams[key]) > 300, (key, written[key], len(streams[key]))
        _same(got[key], streams[key], key)


def _open_dsd(nat, blk):
    fe = nat.Frontend(FS, 0.0, device=0, block_capacity=D * blk, out_capacity=1 << 12)
    c = fe.chan_open(CR, OFFS[0])
    fe.chan_audio_open(c, **host_audio.dsd_feed_params(25000, 0.4))
    return fe, [c]


def test_pump_dsd_feed_more_out_than_in(gpu_required):
    """48/25: a block of 500 channel samples makes 960 audio samples, and the gather's bound ceil(500 * 48 / 25) + 1 holds them"""
    nat = gpu_required
    n_blocks, blk = 8, 500
    f = _Fed(nat, 1, blk, n_blocks, 86, [(0, 0)], "audio", 1 << 13, opener=lambda nat_: _open_dsd(nat_, blk))
    try:
        f.feed(n_blocks, wait=False)
        st = f.pump.wait(timeout_s=30.0)
        assert not st["running"] and st["error"] == 0 and st["blocks_done"] == n_blocks, st
        got, written = f.pump.read(0), f.pump.written(0)
    finally:
        f.close()
    streams, counters = f.twin_streams(0, [(0, "audio")])
    s, c = streams[(0, "audio")], counters[(0, "audio")]
    idx, _, per, w = R.replay_slot(s, c, _bounds("audio", blk, n_blocks, 48, 25), cap=1 << 12, room=1 << 13, interp=48, decim=25)
    assert idx == list(range(len(s))) and [n for _, n in per] == [960] * n_blocks      # no shortfall carried over
    assert written == w == len(s) == n_blocks * 960
    _same(got, s, "dsd feed")
