"""The five frame decoders behind the slicer -- TSBK, EDACS, OSW and the P25 voice stage with its options, the NID option on
both P25 stages -- under one random lifecycle: what tests/test_gpu_fuzz.py's test_random_hard_decision_lifecycles does for two
of them, for all that share attach_frames / frames_state, the planner's launch records, the deferred ring release and the read
rows.  RCF_FUZZ_SEEDS=a:b runs a range of seeds, as there."""
import functools

import numpy as np
import pytest

from rcf import synth
from test_gpu_fuzz import EINVAL, ESTATE, _EDACS_SYNC, _P25_SYNC, _seeds

_SAMPLES = 600000                                # input samples of a run at 400 kS/s: the voice call's LDUs up to the last are decided
_OSW_SYNC = 0b10101100
_LOOP_OF = dict(edacs="clock", osw="clock", fsk4="fsk4", costas="costas")
_SLOT_KINDS = ("edacs", "fsk4", "osw", "fsk4", "costas", "osw", "costas", "edacs")
_SLOT_STAGE = ("edacs", "tsbk", "osw", "voice", "tsbk", "osw", "voice", "edacs")      # the stage a slot is opened with
# how often a call goes to a slot, relatively: a voice unit is decided 888 dibits (74 000 input samples, an eighth of the run)
# behind its sync word, a TSDU 384, and only by a stage that was attached before the sync word came
_SLOT_WEIGHT = (1.0, 0.4, 0.5, 0.02, 1.0, 1.0, 0.4, 1.0)
# The loose searches (13 errors behind the C4FM loop, 17 elsewhere) make noise hit; they also hit the P25 word two or three
# dibits early on a real carrier, and such a hit is accepted and shuts out the true one 24 dibits long, so that a planted
# unit is framed out of place: p25es_ref.run over the call's own dibits finds none of its seven units at 13 errors and all of
# them at 4.  The slot under the planted voice call therefore searches with the 4 errors of rcf.p25.
_STRICT_SLOTS = (3,)
_STREAMS = ("clock", "fsk4", "costas", "hard", "sync", "tsbk", "edacs", "osw", "p25lc")
_STREAM_OF = dict(tsbk="tsbk", edacs="edacs", osw="osw", voice="p25lc")
_COUNTS = ("loop_again_under_stage", "slicer_again", "stage_again", "close", "refusals", "swaps_refused", "swaps_completed")


def _fits(s, kind, stage):
    """include/rcf.h at rcf_chan_tsbk, rcf_chan_edacs, rcf_chan_osw, rcf_chan_p25lc: does a slicer (model) take this stage"""
    if s is None:
        return False
    if kind in ("tsbk", "voice"):
        other = "voice" if kind == "tsbk" else "tsbk"
        return s["mode"] == 2 and s["bits"] == 48 and not s["both"] and stage != other
    if kind == "edacs":
        return s["mode"] == 1 and s["bits"] == 48
    return s["mode"] == 1 and s["bits"] == 8 and s["errors"] == 0 and not s["both"]


def _frames_plan(seed):
    """Everything test_random_frame_decoder_lifecycles draws, and the model of the lifetime rules (include/rcf.h at
    rcf_chan_slicer, rcf_chan_tsbk_ex, rcf_chan_edacs, rcf_chan_osw, rcf_chan_p25lc_ex, rcf_chan_nid_state) that says what each
    call must answer: no device is needed to make it.  -> dict(cap, group, slots, sizes, ops, reads, counts): ops[b] the calls in
    front of block b, each (name, slot, arguments, expected code); reads[b] per stream (reader, cap_each, order seed)"""
    rng = np.random.default_rng(61000 + seed)
    cap = 1 << int(rng.integers(8, 12))
    most = min(400, (cap - 64) // 2)             # channel samples a block: what the smallest ring takes beside the loops' windows
    group = seed % 2 == 1
    slots = [dict(kind=_SLOT_KINDS[i], stage=_SLOT_STAGE[i], fe=i % 2 if group else 0, f=-140e3 + 40e3 * i) for i in range(8)]
    sizes = []
    while sum(sizes) < _SAMPLES:
        sizes.append(int(rng.integers(1, 40)) if rng.random() < 0.15 else int(rng.integers(8 * most, 16 * most + 1)))
    model = {}                                   # slot -> dict(loop, slicer: None / dict(mode, bits, both, errors), stage: None / kind)
    counts = dict({c: 0 for c in _COUNTS}, retune=0, off=0, cross=0)
    ops, reads = [], []

    def slicer_op(i, ops_b, proper=False):
        kind, m = slots[i]["kind"], model[i]
        loop = _LOOP_OF[kind]
        binary = loop == "clock"
        u = 1.0 if proper else rng.random()
        p = dict(source=loop, mode=1 if binary else 2, sync_word=_EDACS_SYNC if binary else _P25_SYNC, sync_bits=48,
                 sync_max_errors=4 if i in _STRICT_SLOTS else 13 if kind == "fsk4" else 17, hit_capacity=int(rng.choice([16, 64, 4096], p=[0.5, 0.25, 0.25])),
                 sync_both=int(rng.random() < (0.7 if kind == "edacs" else 0.1)))
        if proper and not binary:
            p["sync_both"] = 0                   # (a P25 stage does not go behind a slicer that searches both polarities)
        osw = dict(sync_word=_OSW_SYNC, sync_bits=8, sync_max_errors=0, sync_both=0)
        if kind == "osw":
            p.update(osw)
        code = 0
        if u < 0.05:
            p.update(dict(sync_both=1, sync_max_errors=p["sync_bits"] // 2) if rng.random() < 0.5 else dict(hit_capacity=24))
            code = EINVAL
        elif u < 0.10:
            loops = ("clock", "fsk4", "costas")
            p["source"] = loops[(loops.index(loop) + 1 + int(rng.integers(0, 2))) % 3]
            code = ESTATE
        elif u < 0.17:
            p.update(sync_word=0x2D6, sync_bits=10, sync_max_errors=1, sync_both=0)
        elif u < 0.28:                           # the other system's slicer behind this loop
            if kind == "edacs":
                p.update(osw)
            elif kind == "osw":
                p.update(sync_word=_EDACS_SYNC, sync_bits=48, sync_max_errors=17, sync_both=int(rng.random() < 0.5))
            else:
                p.update(mode=1, sync_word=_EDACS_SYNC, sync_max_errors=17)
        if code == 0 and not m["loop"]:
            code = ESTATE
        ops_b.append(("slicer", i, p, code))
        if code:
            counts["refusals"] += 1
            return
        counts["slicer_again"] += m["slicer"] is not None
        m["slicer"] = dict(mode=p["mode"], bits=p["sync_bits"], both=p["sync_both"], errors=p["sync_max_errors"])
        m["stage"] = None

    def stage_op(i, ops_b, proper=False, kind=None):
        m = model[i]
        own = slots[i]["stage"]
        if kind is None:
            u = 0.0 if proper else rng.random()
            if u < 0.70:
                kind = own
            elif u < 0.88:                       # the other P25 stage on a P25 slot (a swap when one is attached), the other binary one else
                kind = dict(tsbk="voice", voice="tsbk", edacs="osw", osw="edacs")[own]
            else:
                kind = ("tsbk", "voice", "edacs", "osw")[int(rng.integers(0, 4))]
        arg = dict(kind=kind, capacity=int(rng.choice([16, 256])), esk=bool(rng.random() < 0.5), nid=bool(rng.random() < 0.5),
                   correct=bool(rng.random() < 0.75), es=bool(rng.random() < 0.6), erasures=bool(rng.random() < 0.5))
        if proper:
            arg["correct"] = arg["correct"] or arg["erasures"]
        fits = _fits(m["slicer"], kind, m["stage"])
        code = 0 if fits else ESTATE
        if kind == "voice" and arg["erasures"] and not arg["correct"]:
            if fits:
                code = EINVAL                    # RCF_P25LC_ERASURES with correct = 0
            else:
                arg["erasures"] = False          # (one reason to refuse at a time: the header does not rank them)
        elif fits and not proper and rng.random() < 0.07:
            arg["capacity"], code = 24, EINVAL
        swap = {kind, m["stage"]} == {"tsbk", "voice"} and m["slicer"] is not None and code == ESTATE
        counts["cross"] += code == ESTATE and m["slicer"] is not None and m["slicer"]["mode"] == 1 and kind in ("voice", "osw", "edacs")
        ops_b.append(("stage", i, arg, code))
        if code:
            counts["refusals"] += 1
            counts["swaps_refused"] += swap
            if swap and rng.random() < 0.9:      # the first off, then the other: it works
                ops_b.append(("stage", i, None, 0))
                m["stage"] = None
                before = counts["refusals"]
                stage_op(i, ops_b, kind=kind)
                counts["swaps_completed"] += counts["refusals"] == before
            return
        counts["stage_again"] += m["stage"] == kind
        m["stage"] = kind

    def loop_op(i, ops_b):
        m = model[i]
        counts["loop_again_under_stage"] += bool(m["loop"] and m["stage"])
        ops_b.append(("loop", i, True, 0))
        m.update(loop=True, slicer=None, stage=None)

    def pick(among):
        """a slot of `among`, by _SLOT_WEIGHT: the slots under the planted P25 carriers live long enough to decide frames"""
        w = np.array([_SLOT_WEIGHT[j] for j in among])
        return among[int(rng.choice(len(among), p=w / w.sum()))]

    def open_op(i, ops_b):
        model[i] = dict(loop=False, slicer=None, stage=None)
        ops_b.append(("open", i, slots[i]["f"], 0))
        loop_op(i, ops_b); slicer_op(i, ops_b, proper=True); stage_op(i, ops_b, proper=True)

    for b, n in enumerate(sizes):
        ops_b = []
        if b == 0:
            for i in range(6):
                open_op(i, ops_b)
        for _ in range(int(rng.poisson(150.0 * n / _SAMPLES))):
            u = rng.random()
            free = [i for i in range(len(slots)) if i not in model]
            if free and (u < 0.12 or not model):
                open_op(free[int(rng.integers(0, len(free)))], ops_b)
                continue
            if not model:
                continue
            live = sorted(model)
            i = pick(live)
            m = model[i]
            again = rng.random() < 0.7           # what went with the old one is attached again behind the new one
            if u < 0.17:
                counts["close"] += 1
                ops_b.append(("close", i, None, 0))
                del model[i]
            elif u < 0.24:
                counts["retune"] += 1
                ops_b.append(("retune", i, slots[i]["f"] + 1250.0 * float(rng.integers(-3, 4)), 0))
            elif u < 0.37:
                loop_op(i, ops_b)
                if again:
                    slicer_op(i, ops_b, proper=True); stage_op(i, ops_b, proper=True)
            elif u < 0.41:
                counts["off"] += 1
                ops_b.append(("loop", i, False, 0))
                m.update(loop=False, slicer=None, stage=None)
            elif u < 0.57:
                slicer_op(i, ops_b)
                if again:
                    stage_op(i, ops_b)
            elif u < 0.61:
                counts["off"] += 1
                ops_b.append(("slicer", i, None, 0))
                m.update(slicer=None, stage=None)
            elif u < 0.87:
                stage_op(i, ops_b)
            elif u < 0.95:                       # the other P25 stage on a slicer that carries one, if there is such a slicer: a swap
                p25 = [j for j in live if model[j]["stage"] in ("tsbk", "voice") and _SLOT_WEIGHT[j] >= 0.1]      # (not under the planted call)
                if p25:
                    i = pick(p25)
                    stage_op(i, ops_b, kind="voice" if model[i]["stage"] == "tsbk" else "tsbk")
                else:
                    stage_op(i, ops_b)
            else:
                counts["off"] += 1
                ops_b.append(("stage", i, None, 0))
                m["stage"] = None
        ops.append(ops_b)
        reads.append({w: (str(rng.choice(["single", "many", "group"] if group else ["single", "many"])), int(rng.choice([3, 17, 64, 1024])),
                          int(rng.integers(0, 1 << 30))) for w in _STREAMS})
    return dict(cap=cap, group=group, slots=slots, sizes=sizes, ops=ops, reads=reads, counts=counts)


@functools.lru_cache(maxsize=None)
def _planted(total):
    """the four fixtures as carriers at their slots' offsets, truncated to the run (made once, never written to): the EDACS
    fixture under slot 0, the TSDU fixture under slot 1, clean OSW frames at 3600 baud under slot 2, the encrypted voice call
    under slot 3"""
    import fsk4_ref as F
    import mm_ref as M
    import p25es_ref as E
    from test_gpu_edacs import edacs_bits
    from test_gpu_osw import clean_bits
    from test_gpu_tsbk import tsdu_dibits
    fs, f = 400e3, [-140e3 + 40e3 * i for i in range(4)]
    made = [0.2 * M.fsk2_carrier(edacs_bits()[0], 9600.0, fs, f[0], 1200.0, np.random.default_rng(5)),
            0.4 * F.c4fm_carrier(tsdu_dibits()[0], 4800, fs, f[1] + 150.0, 0.5, 600.0),
            0.3 * M.fsk2_carrier(clean_bits(36)[0], 3600.0, fs, f[2], 1200.0, np.random.default_rng(6), noise=0.0),
            0.4 * F.c4fm_carrier(E.call_dibits()[0][:int(total * 4800 / fs) + 9], 4800, fs, f[3] + 150.0, 0.5, 600.0)]
    out = []
    for c in made:
        c = c[:total].astype(np.complex64)
        c.setflags(write=False)
        out.append(c)
    return out


def test_the_draws_alone_give_every_kind_of_call():
    """the floors that stand on the draws: over seeds 0 .. 39 the plan holds at least 3 loop re-attaches under a live stage, 8
    slicer re-attaches, 7 stage re-calls, 7 closes, 33 refused calls, 3 swaps of the two P25 stages refused and 3 completed
    per seed (the minima): more than the 2 of each that the GPU test asserts; every seed attaches each of the four stage kinds"""
    low = {c: min(_frames_plan(s)["counts"][c] for s in range(40)) for c in _COUNTS}
    print("draws, minima over seeds 0 .. 39:", low)
    assert all(v >= 3 for v in low.values()), low
    for s in range(40):
        kinds = {op[2]["kind"] for ops_b in _frames_plan(s)["ops"] for op in ops_b if op[0] == "stage" and op[2] is not None and op[3] == 0}
        assert kinds == {"tsbk", "voice", "edacs", "osw"}, (s, kinds)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", _seeds())
def test_random_frame_decoder_lifecycles(gpu_required, seed):
    """All five decoders behind the slicer under a random lifecycle: eight slots of 25 kS/s channels on a 400 kS/s front end
    (odd seeds: on two front ends in a Group) -- clock loop at 9600 baud -> binary slicer with the 48-bit EDACS word
    (sync_both drawn) -> EDACS stage (esk drawn); clock loop at 3600 baud -> binary slicer with the exact 8-bit word -> OSW
    stage; C4FM loop or Gardner / Costas loop -> FSK4 slicer with the P25 word, loose search (13 / 17 errors; 4 under
    the planted voice call: _STRICT_SLOTS) -> the TSBK stage (nid drawn) or
    the voice stage (correct, es, erasures, nid drawn; erasures without correct: RCF_EINVAL) -- over noise and four planted
    fixtures: the EDACS and TSDU fixtures, clean OSW frames, the encrypted voice call.  At random block boundaries channels
    are opened, closed and retuned; loops, slicers and stages are attached again or switched off; the other P25 stage is
    attached while one is (RCF_ESTATE, the slicer's stage survives) and after switching it off (it works); the same stage is
    attached again with other options (afresh: counters 0, the ring as asked); OSW goes to a 48-bit slicer, EDACS to an 8-bit
    one, the voice stage behind a binary slicer (RCF_ESTATE).  Every answer is compared with a model of the rules of
    include/rcf.h (_frames_plan).  After every block rcf_chan_nid_state is called on every live channel -- RCF_ESTATE without a
    P25 stage, four zeros for a stage without the option -- and all nine streams are drained by the single readers,
    chan_read_many or the group's reader with a drawn cap_each.  Rings: out_capacity 2^8 .. 2^11, hit rings of 16 / 64 / 4096
    (the OSW slicer's too: noise hits the 8-bit word once in 256 bits), record rings of 16 / 256; ragged pushes, some of
    under one symbol.  Yardsticks, bit for bit, per life: slicer_ref.run over a slicer life's soft symbols gives its words
    and hits; over those, from the life's first hit, launch by launch with the hit ring's capacity, tsbk_ref.run /
    nid_ref.run_tsbk, p25es_ref.run / nid_ref.run_voice, edacs_ref.run and osw_ref.run (pos0: the slicer's symbol count at
    the attach) give a stage life's records, final counters and NID counters.  A reader a ring or less behind gets
    everything, one further behind the newest ring's worth.  Every draw is made before the device is touched.
    Floors, so that the test cannot pass empty.  From the draws alone (test_the_draws_alone_give_every_kind_of_call holds
    their minima over seeds 0 .. 39): at least 2 per seed of loop re-attaches under a live stage, slicer re-attaches, stage
    re-calls, closes, refused calls, P25 swaps refused and swaps completed.  From the run, measured once on an MI355X over seeds
    0 .. 39 (all 40 pass, about 1 s each), the minimum and maximum per seed: records of TSBK stages 0 .. 33 (seeds 3, 10, 19 and
    25 have none), of voice stages 4 .. 20, of both together 4 .. 43; of those voice records the decoded units (kind != 3) 0 ..
    8 -- they come from the planted call; seed 36 has none: its planted slot is swapped to the TSBK stage 67 000 samples into
    the run, before the HDU is decided, and every other seed has at least 1 --; records of EDACS stages 10 .. 38, of OSW stages
    0 .. 34 (seeds 2, 3, 19, 23, 28 and 29 have none), of both together 16 .. 59; stage lives with n_lost > 0 2 .. 15, with
    nid_decoded > 0 0 .. 5 (seeds 10, 14 and 15 have none), of both together 4 .. 16; slicer words 1387 .. 2349, hits 653 ..
    1957.  The floors are half the minima in whole units: voice records 2, P25 records 2, a decoded voice unit on every seed but
    36, EDACS records 5, EDACS and OSW records 8, one life with n_lost > 0, two lives with n_lost > 0 or nid_decoded > 0; none
    of their own for TSBK records, OSW records and lives with nid_decoded > 0."""
    import edacs_ref as ED
    import nid_ref as N
    import osw_ref as O
    import p25es_ref as E
    import slicer_ref as S
    from rcf import control, p25
    nat = gpu_required
    plan = _frames_plan(seed)
    cap, slots, sizes, counts = plan["cap"], plan["slots"], plan["sizes"], plan["counts"]
    assert min(counts[c] for c in _COUNTS) >= 2, counts
    fs, cr, total = 400e3, 12500, int(np.sum(sizes))
    n_fe = 2 if plan["group"] else 1
    xs = [(0.05 * synth.awgn(np.random.default_rng(62000 + 2 * seed + m), total)).astype(np.complex64) for m in range(n_fe)]
    for i, c in enumerate(_planted(_SAMPLES + 16 * 400)):
        n = min(len(c), total)
        xs[slots[i]["fe"]][:n] += c[:n]
    single = dict(clock="chan_read_clock", fsk4="chan_read_fsk4", costas="chan_read_costas", hard="chan_read_hard", sync="chan_read_sync",
                  tsbk="chan_read_tsbk", edacs="chan_read_edacs", osw="chan_read_osw", p25lc="chan_read_p25lc")
    state_of = dict(tsbk="chan_tsbk_state", edacs="chan_edacs_state", osw="chan_osw_state", voice="chan_p25lc_state")
    ring_of = dict(tsbk="chan_tsbk_ring", edacs="chan_edacs_ring", osw="chan_osw_ring", voice="chan_p25lc_ring")
    no_nid = dict(n_decoded=0, n_fixed=0, n_bits=0, n_bad=0)
    slicer_lives, stage_lives = [], []
    fes = [nat.Frontend(fs, device=0, block_capacity=max(sizes) + 16, out_capacity=cap) for _ in range(n_fe)]
    grp = nat.Group(fes) if plan["group"] else None
    try:
        dev = {}                                 # slot -> dict(fe, m, cid, loop: life / None, slicer: life / None, stage: life / None)

        def call(code, fn, *a, **kw):
            try:
                fn(*a, **kw)
                got = 0
            except nat.RcfError as e:
                got = e.code
            assert got == code, (seed, fn.__name__, a, kw, got, code)

        def has(d, w):
            if w in ("clock", "fsk4", "costas"):
                return d["loop"] is not None and _LOOP_OF[slots[d["slot"]]["kind"]] == w
            return d["slicer"] is not None if w in ("hard", "sync") else d["stage"] is not None and _STREAM_OF[d["stage"]["kind"]] == w

        def gone(fe, cid, stages_only=False):
            for w in ([] if stages_only else ["chan_slicer_state"]) + list(state_of.values()) + ["chan_nid_state"]:
                call(ESTATE, getattr(fe, w), cid)

        def attach(fe, cid, arg, code):
            kind = arg["kind"]
            if kind == "tsbk":
                call(code, fe.chan_tsbk, cid, arg["capacity"], nid=arg["nid"])
            elif kind == "edacs":
                call(code, fe.chan_edacs, cid, arg["capacity"], esk=arg["esk"])
            elif kind == "osw":
                call(code, fe.chan_osw, cid, arg["capacity"])
            else:
                call(code, fe.chan_p25lc_ex, cid, arg["capacity"], correct=arg["correct"], es=arg["es"], erasures=arg["erasures"], nid=arg["nid"])

        def do(op):
            name, i, arg, code = op
            kind = slots[i]["kind"]
            if name == "open":
                fe = fes[slots[i]["fe"]]
                cid = fe.chan_open(cr, arg)
                if kind == "fsk4":
                    fe.chan_fm_filter(cid, p25.fm_gain(cr), p25.symbol_taps(cr, 4800))
                elif kind == "costas":
                    fe.chan_agc(cid, 16, 1.0)
                dev[i] = dict(slot=i, fe=fe, m=slots[i]["fe"], cid=cid, loop=None, slicer=None, stage=None)
                call(ESTATE, fe.chan_nid_state, cid)                                            # a channel with no slicer
                return
            d = dev[i]
            fe, cid = d["fe"], d["cid"]
            if name == "close":
                fe.chan_close(cid)
                del dev[i]
            elif name == "retune":
                fe.chan_set_offset(cid, arg)
            elif name == "loop":
                if kind == "edacs":
                    control.edacs_clock(fe, cid) if arg else fe.chan_clock_mm(cid, None)
                elif kind == "osw":
                    control.smartnet_clock(fe, cid) if arg else fe.chan_clock_mm(cid, None)
                elif kind == "fsk4":
                    fe.chan_fsk4(cid, **p25.fsk4_params(cr, 4800)) if arg else fe.chan_fsk4(cid, None)
                else:
                    fe.chan_costas(cid, **p25.costas_params(cr, 4800)) if arg else fe.chan_costas(cid, None)
                d.update(loop=dict(soft=[], n=0) if arg else None, slicer=None, stage=None)
                gone(fe, cid)                                                                   # slicer and stage went with the old loop
            elif name == "slicer":
                if arg is None:
                    fe.chan_slicer(cid, None)
                    d.update(slicer=None, stage=None)
                    gone(fe, cid)
                    return
                p = dict(arg)
                source = dict(clock=nat.READ_CLOCK, fsk4=nat.READ_FSK4, costas=nat.READ_COSTAS)[p.pop("source")]
                call(code, fe.chan_slicer, cid, source, p.pop("mode"), **p)
                if code == 0:
                    d["slicer"] = dict(p=arg, kind=kind, loop=d["loop"], soft_from=d["loop"]["n"], words=[], hits=[], launches=[], n_symbols=0)
                    d["stage"] = None
                    slicer_lives.append(d["slicer"])
                    assert fe.chan_slicer_state(cid) == dict(n_symbols=0, n_words=0, n_hits=0)
                    gone(fe, cid, stages_only=True)                                             # the stage went with the old slicer
            else:
                if arg is None:
                    fe.chan_tsbk(cid, on=False); fe.chan_edacs(cid, on=False); fe.chan_osw(cid, on=False); fe.chan_p25lc(cid, on=False)
                    d["stage"] = None
                    if d["slicer"] is not None:
                        gone(fe, cid, stages_only=True)
                    return
                attach(fe, cid, arg, code)
                if code == 0:
                    s = d["slicer"]
                    d["stage"] = dict(arg, slicer=s, first_hit=s["launches"][-1][1] if s["launches"] else 0, pos0=s["n_symbols"],
                                      launch_from=len(s["launches"]), recs=[], n=0, state=None, nid_state=None)
                    stage_lives.append(d["stage"])
                    assert not any(getattr(fe, state_of[arg["kind"]])(cid).values()), seed      # afresh
                    assert getattr(fe, ring_of[arg["kind"]])(cid)[1] == arg["capacity"]
                    if arg["kind"] in ("tsbk", "voice"):
                        assert fe.chan_nid_state(cid) == no_nid
                    else:
                        call(ESTATE, fe.chan_nid_state, cid)
                    for other in state_of:                                                      # a slicer carries one stage
                        if other != arg["kind"]:
                            call(ESTATE, getattr(fe, state_of[other]), cid)
                elif d["stage"] is not None:                                                    # the slicer's stage survives a refused call
                    t = d["stage"]
                    assert getattr(fe, state_of[t["kind"]])(cid)["n_records"] == (t["state"] or dict(n_records=0))["n_records"]
                    assert getattr(fe, ring_of[t["kind"]])(cid)[1] == t["capacity"]

        def drain(w, how, cap_each, order_seed):
            """-> {slot: rows of stream w new since the last drain}, by the drawn reader, repeated until nothing comes"""
            live = [dev[i] for i in np.random.default_rng(order_seed).permutation(sorted(dev))]
            got = {d["slot"]: [] for d in live if has(d, w)}
            if how == "single":
                for d in live:
                    reader = getattr(d["fe"], single[w])
                    if not has(d, w):
                        call(ESTATE, reader, d["cid"], cap_each)
                        continue
                    while True:
                        rows = reader(d["cid"], cap_each)
                        rows = np.stack(rows) if w == "sync" else rows.view("<u4") if w == "hard" else rows
                        if rows.shape[-1] == 0:
                            break
                        got[d["slot"]].append(rows)
                return got
            lists = [live] if how == "group" else [[d for d in live if d["m"] == m] for m in range(n_fe)]
            for lst in lists:
                while lst:
                    if how == "group":
                        rows = grp.read_many([(d["m"], d["cid"]) for d in lst], w, cap_each=cap_each)
                    else:
                        rows = lst[0]["fe"].chan_read_many([d["cid"] for d in lst], w, cap_each=cap_each)
                    more = False
                    for d, r in zip(lst, rows):
                        assert (r is not None) == has(d, w), (seed, w, how, d["slot"])
                        if r is not None and len(r):
                            more = True
                            if w == "sync":
                                r = np.stack(nat.widen_hits(r, d["slicer"]["n_symbols"]))
                            got[d["slot"]].append(r.copy())
                    if not more:
                        break
            return got

        at = 0
        for b, n in enumerate(sizes):
            for op in plan["ops"][b]:
                do(op)
            if grp is not None:
                grp.push([x[at:at + n] for x in xs])
            else:
                fes[0].push(xs[0][at:at + n])
            at += n
            for d in dev.values():
                s, t = d["slicer"], d["stage"]
                if s is not None:
                    st = d["fe"].chan_slicer_state(d["cid"])
                    s["before"] = s["launches"][-1] if s["launches"] else (0, 0)
                    s["launches"].append((st["n_words"], st["n_hits"]))
                    s["n_symbols"] = st["n_symbols"]
                if t is not None:
                    t["state"] = getattr(d["fe"], state_of[t["kind"]])(d["cid"])
                    t["launches"] = s["launches"][t["launch_from"]:]           # (a copy: the slicer may outlive the stage)
                if t is not None and t["kind"] in ("tsbk", "voice"):           # the NID's counters, every block on every live channel
                    t["nid_state"] = d["fe"].chan_nid_state(d["cid"])
                    assert t["nid"] or t["nid_state"] == no_nid, (seed, b, t["nid_state"])
                else:
                    call(ESTATE, d["fe"].chan_nid_state, d["cid"])
            for w, (how, cap_each, order_seed) in plan["reads"][b].items():
                for i, rows in drain(w, how, cap_each, order_seed).items():
                    d = dev[i]
                    if w in ("clock", "fsk4", "costas"):
                        d["loop"]["soft"] += rows
                        d["loop"]["n"] += sum(len(r) for r in rows)
                    elif w == "hard":
                        d["slicer"]["words"] += rows
                    elif w == "sync":
                        s = d["slicer"]
                        s["hits"].append((s["before"][1], s["launches"][-1][1], np.concatenate(rows, axis=1) if rows else np.zeros((2, 0), np.int64)))
                    else:
                        t = d["stage"]
                        t["recs"].append((t["n"], t["state"]["n_records"], np.concatenate(rows) if rows else np.zeros(0, nat._read_dtype(w))))
                        t["n"] = t["state"]["n_records"]
            for d in dev.values():               # the slicer has sliced every symbol its loop has delivered
                if d["slicer"] is not None:
                    assert d["slicer"]["n_symbols"] == d["loop"]["n"] - d["slicer"]["soft_from"], (seed, b, d["slot"])
    finally:
        if grp is not None:
            grp.close()
        for fe in fes:
            fe.close()

    def tail(want, before, after, ring, got, what):
        """a reader that was `ring` or less behind gets everything; one further behind the newest `ring`"""
        first = max(before, after - ring)
        assert len(got) == after - first and after <= len(want), (seed, what, before, after, ring, len(got), len(want))
        return first

    n_items = dict(words=0, hits=0)
    for s in slicer_lives:
        p = s["p"]
        soft = np.concatenate(s["loop"]["soft"] + [np.zeros(0, np.float32)])[s["soft_from"]:s["soft_from"] + s["n_symbols"]]
        assert len(soft) == s["n_symbols"]
        ref = S.run(soft, p["mode"], sync_word=p["sync_word"], sync_bits=p["sync_bits"],
                    max_errors=p["sync_bits"] if p["sync_both"] else p["sync_max_errors"])
        keep = np.array([ED.is_hit(int(v), p["sync_max_errors"], p["sync_both"], p["sync_bits"]) for v in ref["dist"]], bool)
        s["ref"] = ref["words"], np.asarray(ref["k"])[keep], np.asarray(ref["dist"])[keep]
        words = np.concatenate(s["words"] + [np.zeros(0, "<u4")])
        n_words, n_hits = s["launches"][-1] if s["launches"] else (0, 0)
        assert n_words == len(ref["words"]) and np.array_equal(words, ref["words"]), (seed, s["kind"], p, n_words, len(ref["words"]))
        assert n_hits == len(s["ref"][1]), (seed, s["kind"], p, n_hits, len(s["ref"][1]))
        for before, after, rows in s["hits"]:
            first = tail(s["ref"][1], before, after, p["hit_capacity"], rows[0], "hits")
            assert np.array_equal(rows[0], s["ref"][1][first:after]) and np.array_equal(rows[1], s["ref"][2][first:after]), (seed, p, before, after)
        n_items["words"] += n_words; n_items["hits"] += n_hits
    n_recs = dict(tsbk=0, voice=0, voice_units=0, edacs=0, osw=0)
    n_lost = n_nid = 0
    for t in stage_lives:
        s = t["slicer"]
        if t["state"] is None:                   # gone before a block came
            continue
        words, k, dist = s["ref"]
        kw = dict(first_hit=t["first_hit"], launches=t["launches"], hit_cap=s["p"]["hit_capacity"])
        want_nst = None
        if t["kind"] == "tsbk":
            want, want_st, want_nst = N.run_tsbk(words, k, dist, nid=int(t["nid"]), **kw)
        elif t["kind"] == "voice":
            options = (E.ES if t["es"] else 0) | (E.ERASURES if t["erasures"] else 0)
            want, want_st, want_nst = N.run_voice(words, k, dist, nid=int(t["nid"]), correct=int(t["correct"]), options=options, **kw)
            n_recs["voice_units"] += int(np.count_nonzero(nat.p25lc_fields(want)["kind"] != 3))
        elif t["kind"] == "edacs":
            want, want_st = ED.run(words, k, dist, sync_both=bool(s["p"]["sync_both"]), esk=t["esk"], **kw)
        else:
            want, want_st = O.run(words, k, pos0=t["pos0"], **kw)
        assert t["state"] == want_st, (seed, t["kind"], s["kind"], s["p"], t["first_hit"], t["state"], want_st)
        assert want_nst is None or t["nid_state"] == want_nst, (seed, t["kind"], t["nid"], t["nid_state"], want_nst)
        for before, after, rows in t["recs"]:
            first = tail(want, before, after, t["capacity"], rows, "records")
            assert rows.tobytes() == want[first:after].tobytes(), (seed, t["kind"], s["kind"], before, after)
        n_recs[t["kind"]] += want_st["n_records"]
        n_lost += want_st["n_lost"] > 0
        n_nid += bool(want_nst and want_nst["n_decoded"] > 0)
    print("frame decoder lifecycles, seed %d: ring %d blocks %d group %d: %s slicer lives %d stage lives %d items %s records %s lives with n_lost %d with nid_decoded %d" % (
        seed, cap, len(sizes), plan["group"], counts, len(slicer_lives), len(stage_lives), n_items, n_recs, n_lost, n_nid))
    assert n_recs["voice"] >= 2 and n_recs["tsbk"] + n_recs["voice"] >= 2 and (n_recs["voice_units"] >= 1 or seed == 36), (seed, n_recs)
    assert n_recs["edacs"] >= 5 and n_recs["edacs"] + n_recs["osw"] >= 8 and n_lost >= 1 and n_lost + n_nid >= 2, (seed, n_recs, n_lost, n_nid)
