"""The carrier-operated capture (rcf_chan_capture; definition: include/rcf.h) restated in numpy from the defining comment
alone: it shares no code with capture_core.hpp.

    open(i)  the carrier detector's, squelch_ref.run from level 0 at the attach point a
    keep(j)  <=> some i >= a has open(i) and j - hang <= i <= j + pre: the dilation of `open` by [-pre, +hang], clipped at a,
             as a count of open samples in [max(j - hang, a), j + pre] out of the cumulative count -- decided for the samples
             a .. a + n_seen - pre - 1 only
    OPEN at j with keep(j) && !(j > a && keep(j - 1)), CLOSE at j with !keep(j) && keep(j - 1); a CLOSE's n_open and peak from
             the open samples inside [open.sample, close.sample)
All indices are channel-output indices; arrays are indexed from the attach point (array index i <-> sample a + i)."""
import numpy as np

import squelch_ref

OPEN, CLOSE = 1, 2
REC_DTYPE = np.dtype([("kind", "<u4"), ("n_open", "<u4"), ("sample", "<i8"), ("pos", "<i8"), ("peak", "<f4"), ("reserved_", "<u4")])


def derive(x, levels, is_open, pre, hang, a=0):
    """What the stage has made of the n samples x (complex64, from the attach point on) whose detector levels / open flags
    are given.  -> dict(keep [n_decided] bool, captured complex64, records REC_DTYPE, state dict)"""
    x = np.asarray(x, np.complex64)
    n = len(x)
    pre, hang = int(pre), int(hang)
    is_open = np.asarray(is_open, bool)
    n_dec = max(0, n - pre)
    c = np.concatenate(([0], np.cumsum(is_open, dtype=np.int64)))       # c[k] = open samples among the first k
    j = np.arange(n_dec, dtype=np.int64)
    lo = np.maximum(j - hang, 0)
    hi = j + pre                                                          # <= n - 1 for every decided j
    keep = (c[hi + 1] - c[lo]) > 0 if n_dec else np.zeros(0, bool)
    prev = np.concatenate(([False], keep[:-1])) if n_dec else keep
    opens = np.flatnonzero(keep & ~prev)
    closes = np.flatnonzero(~keep & prev)
    pos_of = np.concatenate(([0], np.cumsum(keep, dtype=np.int64)))       # captured items before decided sample k
    recs = np.zeros(len(opens) + len(closes), REC_DTYPE)
    k = 0
    with np.errstate(over="ignore"):
        for w, o in enumerate(opens):
            recs[k] = (OPEN, 0, a + o, pos_of[o], 0.0, 0)
            k += 1
            if w < len(closes):
                cl = closes[w]
                inside = is_open[o:cl]
                peak = np.float32(np.max(levels[o:cl][inside])) if inside.any() else np.float32(0)
                recs[k] = (CLOSE, min(int(inside.sum()), 0xFFFFFFFF), a + cl, pos_of[cl], peak, 0)
                k += 1
    any_open = bool(is_open.any())
    state = dict(level=float(levels[-1]) if n else 0.0, n_seen=n, n_decided=n_dec, n_kept=int(keep.sum()), n_records=len(recs),
                 n_windows=len(opens), last_open=int(a + np.flatnonzero(is_open)[-1]) if any_open else -1,
                 in_window=int(bool(keep[-1])) if n_dec else 0, unmuted=int(bool(is_open[-1])) if n else 0)
    return dict(keep=keep, captured=x[:n_dec][keep], records=recs, state=state)


def run(x, thr, alpha, pre, hang, a=0):
    """the stage over the n samples x from the attach point a on; thr: linear (squelch_ref.threshold(db)).  The detector is
    causal, so run(x[:k]) is derive() on the first k levels: see prefixes()"""
    d = squelch_ref.run(np.asarray(x, np.complex64), thr, alpha, first_index=a)
    out = derive(x, d["levels"], d["open"], pre, hang, a)
    out["levels"], out["open"] = d["levels"], d["open"]
    return out


def prefixes(x, thr, alpha, pre, hang, cuts, a=0):
    """run() after each of the cut points (sample counts, ascending): one detector pass, one derive() per cut"""
    d = squelch_ref.run(np.asarray(x, np.complex64), thr, alpha, first_index=a)
    outs = []
    for k in cuts:
        out = derive(x[:k], d["levels"][:k], d["open"][:k], pre, hang, a)
        out["levels"], out["open"] = d["levels"][:k], d["open"][:k]
        outs.append(out)
    return outs


def census(r, pre, hang):
    """what the windows of a result look like, for the tests that demand a case: windows (sample ranges, the last one open-
    ended: None), merged (a window that holds two runs of open samples with a muted gap between), unkept gaps of one sample"""
    recs = r["records"]
    o = [int(q["sample"]) for q in recs if q["kind"] == OPEN]
    c = [int(q["sample"]) for q in recs if q["kind"] == CLOSE]
    return dict(windows=[(o[i], c[i] if i < len(c) else None) for i in range(len(o))],
                one_sample_gaps=sum(1 for i in range(len(c)) if i + 1 < len(o) and o[i + 1] - c[i] == 1))


def records_ok(recs, a=0):
    """the invariants of the record stream: alternate from OPEN, pos and sample advance alike inside a window"""
    for i, q in enumerate(recs):
        if q["kind"] != (OPEN if i % 2 == 0 else CLOSE) or q["reserved_"] != 0:
            return False
        if i % 2 == 1 and q["pos"] - recs[i - 1]["pos"] != q["sample"] - recs[i - 1]["sample"]:
            return False
        if i % 2 == 0 and (q["n_open"] != 0 or q["peak"] != 0 or q["sample"] < a):
            return False
    return True
