"""The counted gather's rule in plain integers -- a restatement of the comment above `struct CountedRec` (rcf_internal.h)
and of DESIGN.md's "Counted slots": which items of a counted stream one gather takes, where they land, and what a whole
pump slot holds after a run of blocks.  No arrays of samples in the rule itself; nothing here is read off the kernel."""


def stream_end(counter, interp=1, decim=1):
    """items of the stream so far: the counter itself, or ceil(counter * interp / decim) behind a resampler"""
    counter, interp, decim = int(counter), int(interp), int(decim)
    if interp == decim:
        return counter
    return -((-counter * interp) // decim)


def gather(counter, interp, decim, cap, max_n, room, state):
    """one gather of a counted stream.  cap: the device ring's capacity; max_n: the most it may take (None: unbounded);
    room: the destination ring's length (None: a linear row); state: (cursor in the stream, items the destination has
    taken so far).  -> (cur, n, positions, state after): stream items [cur, cur + n) go to `positions`"""
    cursor, pos = state
    end = stream_end(counter, interp, decim)
    cur = max(int(cursor), end - int(cap))              # a reader more than a ring behind lost what was overwritten
    avail = max(0, end - cur)
    if room is not None and avail > room:               # a destination ring keeps the newest `room` items
        cur += avail - room
        avail = room
    n = avail if max_n is None else min(avail, int(max_n))
    positions = [(pos + i) % room if room is not None else pos + i for i in range(n)]
    return cur, n, positions, (cur + n, pos + n)


def loop_bound(n_k):
    """the most a steady-state gather takes from a symbol loop after a block of n_k stage inputs"""
    return int(n_k) + 1


def audio_bound(n_k, interp, decim):
    """... and from the voice chain's resampler"""
    return -((-int(n_k) * int(interp)) // int(decim)) + 1


def replay_slot(stream, counters, bounds, cap, room, interp=1, decim=1, first_bound=None, first=0, cursor0=0, written0=0):
    """a whole pump slot.  stream: the stage's whole stream (the twin's, indexable); counters[b]: the stage's counter after
    block b; bounds[b]: the host's steady-state bound for block b's gather; first: the block that carries the slot's first
    gather (cursor0: where the channel's reader stood), which is bounded by first_bound -- the device ring's capacity --
    instead; every bound is capped by the pump ring `room`.
    -> (the stream indices the slot took, in delivery order; those items; per block, the (first index, count) of its
    gather; written)"""
    state = (int(cursor0), int(written0))
    idx, per_block = [], []
    for b in range(first, len(counters)):
        bound = bounds[b] if b > first else (cap if first_bound is None else first_bound)
        cur, n, _, state = gather(counters[b], interp, decim, cap, min(int(bound), int(room)), room, state)
        idx.extend(range(cur, cur + n))
        per_block.append((cur, n))
    return idx, [stream[i] for i in idx], per_block, state[1]
