"""The SmartNet OSW stage (rcf_chan_osw, include/rcf.h) restated in numpy / plain Python, for the tests: the framing with its
lock counter over the slicer's words and hits, launch by launch; deinterleave, the parity syndrome, its correction, the
fields, the records.  Also the other direction for the tests' signals: an encoder (the inverse of the packet's rules), and
the designed streams with what they must contain."""
import numpy as np

from rcf import native

SYNC, SYNC_BITS, FRAME_BITS, PACKET_BITS = 0b10101100, 8, 84, 76
SYNC_LIST = [1, 0, 1, 0, 1, 1, 0, 0]
REL_UNKNOWN = 65535
STATE0 = dict(n_records=0, n_frames=0, n_bad=0, n_rejects=0, n_lost=0, locked=0, is_locked=0)


# ---- the packet
def deinterleave(b):
    """76 packet bits -> out: out[4 x + j] = b[x + 19 j]"""
    out = [0] * PACKET_BITS
    for x in range(19):
        for j in range(4):
            out[4 * x + j] = int(b[x + 19 * j])
    return out


def psyn_of(b):
    """76 packet bits -> (data[38], psyn[38])"""
    out = deinterleave(b)
    data, parity = out[0::2], out[1::2]
    return data, [parity[i] ^ data[i] ^ (data[i - 1] if i else 0) for i in range(38)]


def correct_sequential(data, psyn):
    """the reference's loop (moto_control_demod.py:313-318), as it is written there"""
    data = list(data)
    for x in range(0, len(psyn) - 1):
        if psyn[x] == psyn[x + 1] == 1:
            data[x] = 1 if data[x] == 0 else 0
    return data


def decode(b):
    """76 packet bits -> dict(data: the 38 corrected bits, psyn, bad, flipped, lid, ind, cmd)"""
    data, psyn = psyn_of(b)
    bad = any(psyn)
    fixed = correct_sequential(data, psyn) if bad else list(data)
    num = lambda bits: int("".join(str(v) for v in bits), 2)
    return dict(data=fixed, psyn=psyn, bad=bad, flipped=sum(a != c for a, c in zip(data, fixed)),
                lid=num(fixed[:16]) ^ 0xcc38, ind=fixed[16], cmd=num(fixed[17:27]) ^ 0xd5)


def record(rel_nz, rel, is_locked, sync_pos, locked, d):
    r = np.zeros((), native.OSW_DTYPE)
    r["flags"] = (0 if rel_nz else 1) | int(d["bad"]) << 1 | int(is_locked) << 2 | d["ind"] << 3 | d["flipped"] << 4 | sum(d["psyn"]) << 10 | rel << 16
    r["k"], r["lid"], r["cmd"], r["locked"] = sync_pos & 0xffffffff, d["lid"], d["cmd"], locked
    r["data"][:5] = np.packbits(np.array(d["data"], np.uint8))
    r["psyn"][:5] = np.packbits(np.array(d["psyn"], np.uint8))
    return r


def bits_of_words(words):
    """the bit stream of the slicer's words (uint32, or their uint8 view as chan_read_hard gives it)"""
    words = np.asarray(words)
    return np.unpackbits(words if words.dtype == np.uint8 else words.astype("<u4").view(np.uint8))


# ---- the framing
def run(words, k, pos0=0, first_hit=0, launches=None, word_cap=None, hit_cap=None, base_words=0, base_hits=0, stop_short=None,
        trace=None):
    """-> (records, dict(n_records, n_frames, n_bad, n_rejects, n_lost, locked, is_locked)).  words, k: the slicer's streams
    from its start (k: the hits' last bits); pos0 / first_hit: the slicer's n_symbols / n_hits when the stage was attached;
    launches: [(n_words, n_hits)] after each block (default: one, at the end); word_cap / hit_cap: the rings' capacities
    (default: nothing is ever overwritten); base_words / base_hits: the index of the first word / hit given; stop_short: a
    step is only taken while that many bits lie behind the cursor (229: the reference's `len(buf) > frame_len*3`, for the
    comparison with its runs only); trace: a list that takes a dict per step (for census)"""
    bits = bits_of_words(words)
    bit = lambda p: bits[p - 32 * base_words]
    h = [None] * base_hits + [int(v) - 7 for v in k]
    launches = [(base_words + len(bits) // 32, len(h))] if launches is None else launches
    i, pos, locked, is_locked = first_hit, pos0, 0, 0
    out = []
    st = dict(STATE0)
    for n_words, n_hits in launches:
        W = 32 * n_words
        resync = False
        if hit_cap and i < n_hits - hit_cap:
            st["n_lost"] += n_hits - hit_cap - i
            i = n_hits - hit_cap
            resync = True
        while True:
            while i < n_hits and h[i] < pos:
                i += 1
            h0 = h[i] if i < n_hits else None
            if resync:
                resync = False
                if h0 is not None:
                    pos = h0
            if stop_short is not None and W - pos < stop_short:
                break
            at_cursor = h0 == pos
            if locked >= 4 or (locked == 3 and at_cursor):                   # case A
                if W < pos + FRAME_BITS:
                    break
                rel_nz, rel, case = not at_cursor, 0 if at_cursor else REL_UNKNOWN, "A"
            else:                                                            # case B
                if h0 is None or W < h0 + 92:
                    break
                j = i
                while j < n_hits and h[j] < h0 + 8:
                    j += 1
                h1 = h[j] if j < n_hits else None
                if locked <= 2 and not (h1 is not None and h1 - h0 == FRAME_BITS):
                    if trace is not None:
                        trace.append(dict(kind="reject", locked=locked, pos=pos, h0=h0))
                    pos = h0 + 8
                    st["n_rejects"] += 1
                    continue
                rel_nz, rel, case = h0 != pos, min(h0 - pos, REL_UNKNOWN), "B"
            before = locked
            now = locked - 1 if rel_nz else min(locked + 1, 5) if locked < 5 else locked
            s = pos if now > 2 else h0
            if word_cap and s // 32 < n_words - word_cap:
                st["n_lost"] += 1
                pos = 32 * (n_words - word_cap)
                resync = True
                continue
            locked, is_locked = now, int(now >= 5)
            st["n_frames"] += 1
            d = decode([bit(s + 8 + n) for n in range(PACKET_BITS)])
            if d["bad"]:
                st["n_bad"] += 1
            elif rel_nz:
                locked += 1
            out.append(record(rel_nz, rel, is_locked, s, locked, d))
            if trace is not None:
                trace.append(dict(kind="frame", case=case, locked=before, after=locked, pos=pos, h0=h0, s=s, rel_nz=rel_nz, bad=d["bad"],
                                  at_pos=now > 2, flipped=d["flipped"]))
            pos = s + FRAME_BITS
    recs = np.array(out, native.OSW_DTYPE) if out else np.zeros(0, native.OSW_DTYPE)
    st.update(n_records=len(recs), locked=locked, is_locked=is_locked)
    return recs, st


# ---- the slicer that searches the 8-bit word exactly
def hits(bits):
    """k (the last bit) of every exact match of 10101100 in the bit stream"""
    bits = np.asarray(bits, np.uint8)
    if len(bits) < 8:
        return np.zeros(0, np.int64)
    m = np.ones(len(bits) - 7, bool)
    for n, v in enumerate(SYNC_LIST):
        m &= bits[n:len(bits) - 7 + n] == v
    return np.nonzero(m)[0].astype(np.int64) + 7


def slicer(bits):
    """-> dict(words, k, dist, n_symbols) of a binary slicer over these decisions: whole words only, every hit"""
    bits = np.asarray(bits, np.uint8)
    k = hits(bits)
    return dict(words=np.packbits(bits[:len(bits) // 32 * 32]).view("<u4").copy(), k=k, dist=np.zeros(len(k), np.uint8), n_symbols=len(bits))


# ---- the other direction
def encode(lid, ind, cmd, rest=0):
    """-> the 76 bits of a packet: data = (lid ^ 0xcc38) 16 bits, ind, (cmd ^ 0xd5) 10 bits, `rest` 11 bits; the parity bits;
    interleaved"""
    data = [int(c) for c in "{0:016b}{1:01b}{2:010b}{3:011b}".format(lid ^ 0xcc38, ind, cmd ^ 0xd5, rest)]
    out = []
    for i in range(38):
        out += [data[i], data[i] ^ (data[i - 1] if i else 0)]
    b = [0] * PACKET_BITS
    for x in range(19):
        for j in range(4):
            b[x + 19 * j] = out[4 * x + j]
    return b


def frame(lid, ind, cmd, rest=0):
    return np.array(SYNC_LIST + encode(lid, ind, cmd, rest), np.uint8)


def random_osw(rng):
    return int(rng.integers(0, 1 << 16)), int(rng.integers(0, 2)), int(rng.integers(0, 1 << 10)), int(rng.integers(0, 1 << 11))


def quiet(n, phase=0):
    """n bits with no sync word in them or across their borders with a frame: 1100 repeated (10101100 needs 1010)"""
    return np.array([(1, 1, 0, 0)[(phase + i) % 4] for i in range(n)], np.uint8)


def out_index(o):
    """where bit o of the deinterleaved packet sits in the packet as sent"""
    return (o >> 2) + 19 * (o & 3)


# ---- designed input: a locked stream whose packets carry every single flip and every adjacent pair
def designed_bits(seed=71, lead=600, tail=420):
    """`lead` quiet bits for the clock to settle, eight clean frames (locked reaches 5), then back-to-back frames: one per
    single flip of the packet's 76 bits, one per adjacent pair (n, n + 1) of them as sent, n = 0 .. 74; a last sync word and
    `tail` quiet bits -> (bits, per frame (lid, ind, cmd, rest) as sent, the frames' starts, per frame the tuple of packet
    bits flipped)"""
    rng = np.random.default_rng(seed)
    patterns = [()] * 8 + [(n,) for n in range(76)] + [(n, n + 1) for n in range(75)]
    parts, sent, starts = [quiet(lead)], [], []
    for n, p in enumerate(patterns):
        while True:
            m = random_osw(rng)
            f = frame(*m)
            for n_bit in p:
                f[8 + n_bit] ^= 1
            if len(hits(np.concatenate([f, SYNC_LIST[:7]]))) == 1:      # no second sync word in or behind the packet
                break
        starts.append(lead + FRAME_BITS * n); sent.append(m); parts.append(f)
    parts += [np.array(SYNC_LIST, np.uint8), quiet(tail, 2)]
    return np.concatenate(parts), sent, starts, patterns


def designed_expect(pattern):
    """what the rules make of a clean packet with these packet bits (as sent) flipped -> (bad, the data positions the
    correction flips, the data positions left wrong afterwards)"""
    pattern = [4 * (n % 19) + n // 19 for n in pattern]            # packet bit n is bit 4 x + j of the deinterleaved packet
    dflip = {o // 2 for o in pattern if o % 2 == 0}
    pflip = {o // 2 for o in pattern if o % 2}
    psyn = [0] * 39
    for i in range(38):
        psyn[i] = (i in pflip) ^ (i in dflip) ^ ((i - 1) in dflip)
    fixed = {x for x in range(37) if psyn[x] and psyn[x + 1]}
    return any(psyn), fixed, dflip ^ fixed


# ---- the lock carrier: every value of the counter, both acceptance paths, rejects, a false sync word inside a packet
def lock_bits(seed=72, lead=600, tail=420):
    """-> (bits, {start: (lid, ind, cmd, rest)} of the frames planted clean, the starts of those whose packet holds a sync
    word).  In order: clean frames up to lock; a quiet gap that two frames taken blindly at the cursor (case A) fall into, 5 ->
    4 -> 3, then the next frame taken at its hit with a clean packet (3 -> 2 -> 3) and lock again; the same with a broken
    packet (3 -> 2); then [4 quiet bits, broken frame, lone sync word] six times -- each accepted behind a jump with a broken
    packet, a reject at the lone word in between -- down to -4; two frames with nothing 84 bits on (rejects); clean frames up to
    lock from below zero; locked, a frame whose packet holds the sync word (nothing happens); unlocked, another (the framing
    rejects its start); clean frames to lock again"""
    rng = np.random.default_rng(seed)
    parts, planted, with_sync = [quiet(lead)], {}, []
    at = [lead]

    def put(bits):
        bits = np.asarray(bits, np.uint8)
        parts.append(bits)
        at[0] += len(bits)

    def osw(broken=False, false_sync=False):
        while True:
            m = random_osw(rng)
            f = frame(*m)
            if false_sync and len(hits(f[1:])) > 0:
                break
            if not false_sync and not any(len(hits(np.concatenate([f[1:], c]))) for c in (SYNC_LIST[:7], quiet(7))):
                break
        if false_sync:
            with_sync.append(at[0])
        if broken:
            f[8 + out_index(1)] ^= 1                                         # one parity bit: counted bad, nothing to correct
        else:
            planted[at[0]] = m
        put(f)

    for _ in range(8):
        osw()
    put(quiet(2 * FRAME_BITS + 20))
    for _ in range(4):
        osw()
    put(quiet(2 * FRAME_BITS + 20))
    osw(broken=True)
    for _ in range(6):
        put(quiet(4)); osw(broken=True); put(SYNC_LIST)
    for _ in range(2):
        put(quiet(40)); osw(); put(quiet(20))
    for _ in range(12):
        osw()
    osw(false_sync=True)
    for _ in range(3):
        osw()
    put(quiet(2 * FRAME_BITS + 20))
    osw(broken=True)
    osw(false_sync=True)
    for _ in range(10):
        osw()
    put(SYNC_LIST); put(quiet(tail, 2))
    return np.concatenate(parts), planted, with_sync


def census(trace):
    """what a run's trace (run(trace=)) met -> dict"""
    frames = [t for t in trace if t["kind"] == "frame"]
    return dict(locked=sorted({t["locked"] for t in trace} | {t["after"] for t in frames}),
                jump_clean=sum(t["rel_nz"] and not t["bad"] for t in frames), jump_bad=sum(t["rel_nz"] and t["bad"] for t in frames),
                three_to_two_at_h0=sum(t["locked"] == 3 and t["rel_nz"] and not t["at_pos"] for t in frames),
                case_a_jump=sum(t["case"] == "A" and t["rel_nz"] for t in frames),
                at_pos=sum(t["at_pos"] for t in frames), at_h0=sum(not t["at_pos"] for t in frames),
                rejects=sum(t["kind"] == "reject" for t in trace))


def lock_census(words, k, shift=0, **kw):
    """the restatement over a slicer's streams of the lock carrier, whose bit 0 is the stream's bit `shift` -> (records,
    state); asserts the carrier's census, so that no test passes on input that missed its target"""
    _, planted, with_sync = lock_bits()
    trace = []
    want, want_st = run(words, k, trace=trace, **kw)
    c = census(trace)
    assert set(range(-2, 6)) <= set(c["locked"]) and min(c["locked"]) <= -4, c
    assert c["jump_clean"] >= 2 and c["jump_bad"] >= 6 and c["three_to_two_at_h0"] >= 2 and c["case_a_jump"] >= 4 and c["rejects"] >= 8, c
    frames = {t["s"] - shift: t for t in trace if t["kind"] == "frame"}
    locked_one, unlocked_one = with_sync
    assert locked_one in frames and frames[locked_one]["locked"] == 5 and not frames[locked_one]["bad"]    # locked: a sync word inside a packet is nothing
    assert any(t["kind"] == "reject" and t["h0"] - shift == unlocked_one for t in trace) and unlocked_one not in frames   # unlocked: it breaks the framing
    got = {(int(rec["k"]) - shift) & 0xffffffff: (int(rec["lid"]), int(rec["cmd"])) for rec in want}
    assert sum(got.get(s) == (m[0], m[2]) for s, m in planted.items()) >= len(planted) - 4
    return want, want_st
