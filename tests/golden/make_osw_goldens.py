#!/usr/bin/env python3
"""Generate tests/golden/smartnet_osw.npz by RUNNING the reference's own receive_engine.

moto_control_demod.py's receive_engine is plain Python string work inside a thread loop; the module imports with GNU Radio,
redis and the connectors replaced by stand-ins (build container only: needs /root/reference), and the method runs on an
instance that was never constructed: tune_next_control and log are mocks, client_redis.send_event_lazy a recorder that also
notes packets, packets_bad and is_locked at each event, control_msg_sink_msgq a fake that hands over the whole stream as ONE
message, and time.sleep ends the loop after enough idle turns.  For Python 3 `channels` is an EMPTY dict subclass with
has_key -- no event is skipped, events are 1 : 1 with packets -- and the message is a latin-1 str.

Streams come from an encoder of this generator's OWN, the inverse of the packet's rules: clean runs (some with no sync word
inside a packet: every message of those comes back as sent); bit error rates of 0.5, 2
and 5 %; truncated frames; noise gaps of 1 .. 400 bits every 3rd or 7th frame; random prefixes; every stream ends in at least
300 noise bits, a sync word and zeros up to a whole word, so find never returns -1 while the loop runs and no frame is cut
off by the end.  Written, data only: the packed streams, and per event lid, ind, cmd, tg, status, packets, packets_bad,
is_locked.
"""
import os
import re
import sys
import types
from unittest import mock

import numpy as np

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "smartnet_osw.npz")
SYNC = [1, 0, 1, 0, 1, 1, 0, 0]


class _TopBlock:
    def __init__(self, *a, **k): pass


gr = mock.MagicMock()
gr.top_block = _TopBlock
gnuradio = types.ModuleType("gnuradio")
gnuradio.gr = gr
subs = ("filter", "blocks", "zeromq", "analog", "digital")
for name in subs:
    setattr(gnuradio, name, mock.MagicMock())
sys.modules["gnuradio"] = gnuradio
sys.modules["gnuradio.gr"] = gr
for name in subs:
    sys.modules["gnuradio." + name] = getattr(gnuradio, name)
sys.modules["gnuradio.filter.firdes"] = gnuradio.filter.firdes
for name in ("setproctitle", "frontend_connector", "redis_demod_publisher", "redis_channelizer_manager", "client_redis"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF)
import moto_control_demod as module  # noqa: E402


class Channels(dict):
    def has_key(self, key):
        return key in self


class Message:
    def __init__(self, s): self.s = s
    def to_string(self): return self.s


class Queue:
    def __init__(self, data): self.items = [Message(data)]
    def count(self): return len(self.items)
    def delete_head(self): return self.items.pop(0)


def reference_run(byte_stream):
    """the reference over the stream as one message -> (events, the `locked` values its debug line showed, packets taken at
    the hit ('--- no lock ---'), steps)"""
    ref = object.__new__(module.moto_control_demod)
    ref.log = mock.MagicMock()
    ref.tune_next_control = mock.MagicMock()
    ref.keep_running = True
    ref.is_locked = False
    ref.packets = ref.packets_bad = 0
    ref.system_id = 0x1234
    ref.instance_uuid = "golden"
    ref.system = {"id": 0x1234}
    ref.channels = Channels()
    ref.channels_list = [0]
    ref.control_channel_key = 0
    ref.control_channel = 0
    ref.control_msg_sink_msgq = Queue(bytes(byte_stream).decode("latin-1"))
    events = []

    def send(topic, p):
        events.append(dict(p, packets=ref.packets, packets_bad=ref.packets_bad, is_locked=ref.is_locked))
    ref.client_redis = mock.MagicMock()
    ref.client_redis.send_event_lazy = send
    idle = [0, 0]                                       # turns without a step, steps seen

    def sleep(_):                                       # every turn behind the first sleeps: 50 of them without a step end the run
        steps = ref.log.debug.call_count
        idle[0] = idle[0] + 1 if steps == idle[1] else 0
        idle[1] = steps
        if idle[0] >= 50:
            ref.keep_running = False
    with mock.patch.object(module.time, "sleep", sleep):
        ref.receive_engine()
    locked, steps = [], 0
    for c in ref.log.debug.call_args_list:
        m = re.match(r"sync_loops \((-?\d+)\) locked: \((-?\d+)\)", c.args[0])
        if m:
            locked.append(int(m.group(2)))
            steps += 1
    no_lock = sum(1 for c in ref.log.warning.call_args_list if c.args[0] == "--- no lock ---")
    return events, locked, no_lock, steps


def encode(lid, ind, cmd, rest):
    data = [int(c) for c in "{0:016b}{1:01b}{2:010b}{3:011b}".format(lid ^ 0xcc38, ind, cmd ^ 0xd5, rest)]
    out = []
    for i in range(38):
        out += [data[i], data[i] ^ (data[i - 1] if i else 0)]
    b = [0] * 76
    for x in range(19):
        for j in range(4):
            b[x + 19 * j] = out[4 * x + j]
    return b


def syncs_in(bits):
    return sum(bits[i:i + 8] == SYNC for i in range(len(bits) - 7))


def stream(rng, n_frames, ber, gap_every, truncate, prefix, plain):
    """plain: no packet holds the sync word or makes one with the next frame's (a clean run then frames from its first bit)"""
    bits, sent = list(rng.integers(0, 2, prefix)), []
    for n in range(n_frames):
        while True:
            m = (int(rng.integers(0, 1 << 16)), int(rng.integers(0, 2)), int(rng.integers(0, 1 << 10)), int(rng.integers(0, 1 << 11)))
            f = SYNC + encode(*m)
            if not plain or syncs_in(f + SYNC[:7]) == 1:
                break
        if truncate and n % 11 == 5:
            f = f[:int(rng.integers(20, 84))]
        f = [b ^ int(rng.random() < ber) for b in f]
        sent.append(m)
        bits += f
        if gap_every and n % gap_every == gap_every - 1:
            bits += list(rng.integers(0, 2, int(rng.integers(1, 401))))
    bits += list(rng.integers(0, 2, 300 + int(rng.integers(0, 100)))) + SYNC
    bits += [0] * (96 + (-(len(bits) + 96)) % 32)
    return np.packbits(np.array(bits, np.uint8)), sent


def main():
    rng = np.random.default_rng(3600)
    plans = []
    for n in range(60):
        ber = (0.0, 0.005, 0.02, 0.05)[n % 4] if n >= 6 else 0.0
        plans.append(dict(n_frames=60, ber=ber, gap_every=(0, 3, 7)[n % 3] if n >= 3 else 0, truncate=n % 5 == 4,
                          prefix=int(rng.integers(0, 200)) if n % 2 else 0, plain=n < 6 and n % 2 == 0))
    streams, n_bytes, n_events, rows = [], [], [], []
    seen = dict(top=False, low=False, negative=False, at_pos=0, at_hit=0, rejects=0)
    for n, plan in enumerate(plans):
        by, sent = stream(rng, **plan)
        events, locked, no_lock, steps = reference_run(by)
        streams.append(by); n_bytes.append(len(by)); n_events.append(len(events))
        for e in events:
            lid, cmd = int(e["lid"], 16), int(e["cmd"], 16)
            assert e["tg"] == lid & 0xfff0 and e["status"] == lid & 0xf and e["ind"] in "GI"
            rows.append((lid, e["ind"] == "G", cmd, e["tg"], e["status"], e["packets"], e["packets_bad"], e["is_locked"]))
        assert [e["packets"] for e in events] == list(range(1, len(events) + 1))        # events are 1 : 1 with packets
        seen["top"] |= any(e["is_locked"] for e in events)
        went_up = False
        for v in locked:
            went_up |= v >= 5
            seen["low"] |= went_up and v <= 2
        seen["negative"] |= min(locked) < 0
        seen["at_hit"] += no_lock; seen["at_pos"] += len(events) - no_lock; seen["rejects"] += steps - len(events)
        if plan["plain"] and not plan["gap_every"] and not plan["truncate"]:          # a clean run: every message as sent
            got = [(int(e["lid"], 16), int(e["ind"] == "G"), int(e["cmd"], 16)) for e in events]
            assert got[:len(sent)] == [m[:3] for m in sent], n
            assert events[len(sent) - 1]["packets_bad"] == 0
    assert seen["top"] and seen["low"] and seen["negative"] and min(seen["at_pos"], seen["at_hit"], seen["rejects"]) > 0, seen
    rows = np.array(rows, np.int64)
    np.savez_compressed(OUT, streams=np.concatenate(streams), n_bytes=np.array(n_bytes, np.int32), n_events=np.array(n_events, np.int32),
                        lid=rows[:, 0].astype(np.uint16), ind=rows[:, 1].astype(np.uint8), cmd=rows[:, 2].astype(np.uint16),
                        tg=rows[:, 3].astype(np.uint16), status=rows[:, 4].astype(np.uint8), packets=rows[:, 5].astype(np.int32),
                        packets_bad=rows[:, 6].astype(np.int32), is_locked=rows[:, 7].astype(np.uint8))
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(plans), "streams,", len(rows), "events;", seen)


if __name__ == "__main__":
    main()
