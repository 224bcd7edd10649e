"""The hard-decision stage (rcf_chan_slicer, include/rcf.h) restated in plain numpy: decisions, MSB-first packing to bytes
and little-endian words, and the sync hits as (k, dist).  `cuts` walks the soft symbols in pieces and carries the state --
the bits not yet in a word, the last sync_bits - 1 bits -- across them, as the stage does across blocks."""
import numpy as np

BINARY, FSK4 = 1, 2
LEVELS = (-2.0, 0.0, 2.0, 4.0)


def decisions(soft, mode, levels=LEVELS):
    s = np.asarray(soft, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        if mode == BINARY:
            return (s >= 0).astype(np.uint8)                      # a NaN: 0
        l = np.asarray(levels, dtype=np.float32)
        return np.where(s < l[0], 3, np.where(s < l[1], 2, np.where(s < l[2], 0, 1))).astype(np.uint8)   # a NaN: 1


def bits_of(d, mode):
    """the bit stream of decisions d: per symbol the 1 or 2 bits, the higher one first"""
    d = np.asarray(d, dtype=np.uint8)
    if mode == BINARY:
        return d & 1
    return np.stack([(d >> 1) & 1, d & 1], axis=1).reshape(-1)


def hits_of(bits, bps, sync_word, sync_bits, max_errors, first_bit=0):
    """(k, dist) of every window of sync_bits bits that ends with a symbol and is within max_errors of the word; bit i of
    `bits` is bit first_bit + i of the stream (only windows that lie inside `bits` are looked at)"""
    if not sync_bits:
        return np.zeros(0, np.int64), np.zeros(0, np.uint8)
    word = np.array([(int(sync_word) >> (sync_bits - 1 - i)) & 1 for i in range(sync_bits)], dtype=np.uint8)
    n = len(bits)
    ks, ds = [], []
    for end in range(sync_bits, n + 1):                # window = bits[end - sync_bits : end]
        pos = first_bit + end                          # stream bits up to and with the window's last
        if pos % bps:
            continue
        dist = int(np.count_nonzero(bits[end - sync_bits:end] ^ word))
        if dist <= max_errors:
            ks.append(pos // bps - 1)
            ds.append(dist)
    return np.array(ks, np.int64), np.array(ds, np.uint8)


def run(soft, mode, levels=LEVELS, sync_word=0, sync_bits=0, max_errors=0, cuts=None):
    """-> dict(bytes, words, k, dist, n_symbols): the whole WORDS of the packed stream as uint32 and as their uint8 view
    (GNU Radio's byte stream, cut at the last whole word), and the hits.  cuts: ascending indices at which the soft symbols
    are cut into pieces, each walked with the state the piece before left."""
    soft = np.asarray(soft, dtype=np.float32)
    bps = 1 if mode == BINARY else 2
    edges = [0] + [int(c) for c in (cuts or [])] + [len(soft)]
    pend = np.zeros(0, np.uint8)           # bits not yet in a whole word
    keep = np.zeros(0, np.uint8)           # the stream's last sync_bits - 1 bits
    n_bits = 0
    words, ks, ds = [], [], []
    for a, b in zip(edges[:-1], edges[1:]):
        new = bits_of(decisions(soft[a:b], mode, levels), mode)
        both = np.concatenate([keep, new])
        k, d = hits_of(both, bps, sync_word, sync_bits, max_errors, first_bit=n_bits - len(keep))
        ks.append(k); ds.append(d)
        n_bits += len(new)
        keep = both[max(0, len(both) - max(sync_bits - 1, 0)):] if sync_bits else keep
        pend = np.concatenate([pend, new])
        whole = len(pend) // 32 * 32
        if whole:
            words.append(np.packbits(pend[:whole]))
        pend = pend[whole:]
    by = np.concatenate(words) if words else np.zeros(0, np.uint8)
    return dict(bytes=by, words=by.view("<u4").copy(), k=np.concatenate(ks) if ks else np.zeros(0, np.int64),
                dist=np.concatenate(ds) if ds else np.zeros(0, np.uint8), n_symbols=len(soft))


def hit_items(k, dist):
    """the hit ring's uint32 items"""
    return ((np.asarray(dist, np.uint32) << np.uint32(26)) | (np.asarray(k, np.int64) & 0x3ffffff).astype(np.uint32)).astype(np.uint32)
