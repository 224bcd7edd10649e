"""The P25 control / voice demodulators behind a channel, built on the GPU up to the slicer (p25_control_demod.py:105-183,
logging_receiver.py:231-332).  Both modulations start from the same pre-filter and split right after it:

  C4FM   quadrature_demod_cf(channel_rate / (2 pi 600)) -> fir_filter_fff(1, (1/sps,)*sps) -> op25 fsk4_demod_ff
         -> op25 fsk4_slicer_fb([-2, 0, 2, 4])
  CQPSK  multiply_const_cc(1.0) -> feedforward_agc_cc(1024, 1.0) -> multiply_const_cc(1.0) -> op25 gardner_costas_cc
         -> diff_phasor_cc -> complex_to_arg -> multiply_const_ff(4 / pi) -> op25 fsk4_slicer_fb([-2, 0, 2, 4])

Both chains run on the GPU up to the slicer (c4fm_demod, cqpsk_demod).  The two sequential op25 loops are the stages
rcf_chan_fsk4 (fsk4_demod_ff) and rcf_chan_costas (gardner_costas_cc ... multiply_const_ff), which include/rcf.h defines
from the published algorithms -- op25's source is not in the reference tree, so both stages are unpinned against op25 --,
and a demod reads soft dibits at the symbol rate (chan_read_fsk4, chan_read_costas) and slices them (slice_dibits) -- or,
with hard=True, lets the GPU slice, pack and look for the frame sync (rcf_chan_slicer) and reads packed dibits and the
places frames begin (chan_read_hard, chan_read_sync).  A consumer that runs op25's own loop reads the front half's output
instead (chan_read_sym, chan_read_agc)."""
import math

import numpy as np

from . import native

SYMBOL_RATE = 4800           # p25_control_demod.py:82 (phase 1; logging_receiver.py:286 runs phase 2 at 6000)
SYMBOL_DEVIATION = 600.0     # p25_control_demod.py:116
SLICER_LEVELS = (-2.0, 0.0, 2.0, 4.0)   # op25.fsk4_slicer_fb's argument (p25_control_demod.py:167)
FRAME_SYNC = 0x5575F5FF77FF  # the 48-bit frame sync the consumer looks for (p25_control_demod.py:337)
FRAME_SYNC_BITS = 48
# Hamming distance up to which a window counts as a frame sync.  A default of this project: the reference itself compares
# bytes exactly (buf.find), and op25's own threshold is not in the reference tree.
FRAME_SYNC_MAX_ERRORS = 4


def _one_decoder(tsbk, lc):
    if tsbk and lc:
        raise ValueError("tsbk and lc exclude each other: a slicer carries one frame decoder")


def _hard(fe, cid, source, tsbk=False, lc=False, es=False, erasures=False, nid=False, viterbi=False):
    fe.chan_slicer(cid, source, native.SLICE_FSK4, SLICER_LEVELS, FRAME_SYNC, FRAME_SYNC_BITS, FRAME_SYNC_MAX_ERRORS)
    if tsbk:
        fe.chan_tsbk(cid, nid=nid, viterbi=viterbi)
    if lc:
        fe.chan_p25lc_ex(cid, es=es, erasures=erasures, nid=nid)


# ---- the NID's BCH(63,16,23) word on the host (the stages' option nid=True decodes it on the GPU: rcf.h at rcf_chan_tsbk_ex)
NID_GENERATOR = 0o6331141367235453   # degree 47: the lcm of the minimal polynomials of alpha^1 .. alpha^22 in GF(64), x^6 + x + 1
_NID_WORDS = None


def nid_encode(nac, duid):
    """the 63-bit code word of (nac, duid), the first bit highest: the 16 data bits, then the 47 check bits"""
    data = ((nac & 0xfff) << 4 | (duid & 15)) << 47
    rem = data
    for e in range(62, 46, -1):
        if rem >> e & 1:
            rem ^= NID_GENERATOR << (e - 47)
    return data | rem


def nid_decode(bits):
    """the host form of the stages' NID rule.  bits: the NID's first 63 bits (a sequence of 0 / 1, info bits 48 .. 110 of a
    frame; a 64th is ignored) or the same as an int, the first bit highest -> dict(nac, duid, nid_fix): the code word within
    11 bits if there is one, nid_fix the bits it changes; else nac and duid as received and nid_fix 15.  By search over all
    65536 code words, so complete by construction"""
    global _NID_WORDS
    if _NID_WORDS is None:
        rows = [nid_encode(0, 0)] + [nid_encode((1 << b) >> 4, (1 << b) & 15) for b in range(16)]
        words = np.zeros(1, np.uint64)
        for r in rows[1:]:
            words = np.concatenate([words, words ^ np.uint64(r)])
        _NID_WORDS = words
    if not isinstance(bits, (int, np.integer)):
        v = 0
        for b in list(bits)[:63]:
            v = v << 1 | (int(b) & 1)
        bits = v
    r = int(bits) & ((1 << 63) - 1)
    x = _NID_WORDS ^ np.uint64(r)
    dist = np.unpackbits(x.view(np.uint8)).reshape(-1, 64).sum(axis=1)
    at = int(np.argmin(dist))
    fix = int(dist[at])
    word = int(_NID_WORDS[at]) if fix <= 11 else r
    return dict(nac=word >> 51, duid=word >> 47 & 15, nid_fix=fix if fix <= 11 else 15)


# ---- a TSBK block's rate-1/2 trellis on the host (the TSBK stage's option viterbi=True decodes it on the GPU: rcf.h at
# rcf_chan_tsbk_opt).  TRELLIS[s][d]: the 4-bit code word sent for dibit d in state s
TRELLIS = ((0x2, 0xC, 0x1, 0xF), (0xE, 0x0, 0xD, 0x3), (0x9, 0x7, 0xA, 0x4), (0x5, 0xB, 0x6, 0x8))


def trellis_decode(code_words, viterbi=True):
    """the host form of the TSBK stage's trellis rule.  code_words: a block's 49 deinterleaved code words of 4 bits each ->
    (the 48 decoded dibits, cost, n_inexact).  viterbi=True: the path of least cost that ends in state 0, the
    lexicographically smallest of equals, by the backward costs beta and a forward walk; cost is the number of bits in which
    the 196 differ from the path's, n_inexact the code words that differ.  viterbi=False: the reference's walk -- per code
    word the nearest candidate, the lowest of equals --; n_inexact counts the words with no equal candidate and cost is the
    sum of the distances to the candidates taken"""
    c = [int(v) & 15 for v in code_words]
    if len(c) != 49:
        raise ValueError("a block has 49 code words, not %d" % len(c))
    dist = lambda s, d, t: bin(TRELLIS[s][d] ^ c[t]).count("1")
    states, cost, inexact, s = [], 0, 0, 0
    if not viterbi:
        for t in range(49):
            away = [dist(s, d, t) for d in range(4)]
            d = away.index(min(away))
            cost += away[d]
            inexact += away[d] != 0
            states.append(d)
            s = d
        return states[:48], cost, inexact
    beta = [[0] * 4 for _ in range(50)]
    beta[48] = [dist(r, 0, 48) for r in range(4)]
    for t in range(47, -1, -1):
        beta[t] = [min(dist(r, d, t) + beta[t + 1][d] for d in range(4)) for r in range(4)]
    for t in range(49):
        sums = [dist(s, d, t) + beta[t + 1][d] for d in (range(4) if t < 48 else range(1))]
        d = sums.index(min(sums))
        away = dist(s, d, t)
        cost += away
        inexact += away != 0
        states.append(d)
        s = d
    return states[:48], cost, inexact


def tsdu_frames(records, reference_rule=False):
    """records of the TSBK stage (Frontend.chan_read_tsbk, native.TSBK_DTYPE) grouped into frames, in the stream's order ->
    list of dict(k, dist, nac, duid, frame_dibits, nid: 8 octets as received, nid_fix, nid_decoded, tsbk: list of dict(b, octets: 12 octets, crc: 0 good /
    1 bad as subprocTSBK's, next_bit, n_inexact)).  A frame record (no block) gives a frame with an empty list.
    reference_rule=True stops a frame's list behind a block whose next_bit is 1, as procTSDU does: the list is then its
    r['tsbk'].  A frame is told from the one before by the low 32 bits of k."""
    records = np.asarray(records, dtype=native.TSBK_DTYPE)
    f = dict(native.tsbk_fields(records), **native.nid_fields(records))
    frames, stopped = [], False
    for i in range(len(records)):
        k = int(records["k"][i])
        if not frames or frames[-1]["k"] != k:
            frames.append(dict(k=k, dist=int(f["dist"][i]), nac=int(f["nac"][i]), duid=int(f["duid"][i]),
                               frame_dibits=int(f["frame_dibits"][i]), nid=bytes(records["nid"][i]), nid_fix=int(f["nid_fix"][i]),
                               nid_decoded=int(f["nid_decoded"][i]), tsbk=[]))
            stopped = False
        if f["b"][i] == 3 or stopped:
            continue
        frames[-1]["tsbk"].append(dict(b=int(f["b"][i]), octets=bytes(records["octets"][i]), crc=int(f["crc_bad"][i]),
                                       next_bit=int(f["next_bit"][i]), n_inexact=int(f["n_inexact"][i])))
        stopped = bool(reference_rule and f["next_bit"][i])
    return frames


# the data units by DUID, as p25_general's proc* name them in r['short']
DUID_SHORT = {0x0: "HDU", 0x3: "TnoLC", 0x5: "LDU1", 0x7: "TSDU", 0xA: "LDU2", 0xC: "PDU", 0xF: "TLC"}


def _bits(octets, lo, hi):
    return (int.from_bytes(octets, "big") >> (8 * len(octets) - hi)) & ((1 << (hi - lo)) - 1)


def link_control(octets):
    """the 9 octets of a link control word as p25_general.subprocLC reads them -> dict(lcf, mfid; for lcf 0x0 lcf_long,
    emergency, tgid, source_id; for lcf 0x15 lcf_long)"""
    lc = dict(lcf=_bits(octets, 2, 8), mfid=_bits(octets, 8, 16))
    if lc["lcf"] == 0x0:
        lc.update(lcf_long="Group Voice Channel User", emergency=_bits(octets, 16, 17), tgid=_bits(octets, 32, 48),
                  source_id=_bits(octets, 48, 72))
    elif lc["lcf"] == 0x15:
        lc["lcf_long"] = "Call Termination / Cancellation"
    return lc


def voice_units(records):
    """records of the P25 voice stage (Frontend.chan_read_p25lc, native.P25LC_DTYPE), in the stream's order -> list of dict
    shaped like the results of p25_general's proc*: short ('HDU' / 'LDU1' / 'TLC' / 'LDU2' / 'TnoLC' / 'TSDU' / 'PDU'; None
    for a DUID the reference does not know), nac, duid, k, dist, frame_dibits, decoded (False: a frame record -- the unit has
    no link control, or the frame was too short for it), rs_bad, n_rs, n_fixed, n_bad, nid_fix, nid_decoded; for a decoded LDU1 or TLC `lc`
    (link_control of the 9 octets) and for the LDU1 `lsd` (4 octets); for a decoded HDU mi (9 octets), mfid, algid, kid, tgid;
    for a decoded LDU2 (a stage attached with es=True) its encryption sync mi (9 octets), algid, kid, and `lsd`"""
    records = np.asarray(records, dtype=native.P25LC_DTYPE)
    f = dict(native.p25lc_fields(records), **native.nid_fields(records))
    units = []
    for i in range(len(records)):
        kind, duid = int(f["kind"][i]), int(f["duid"][i])
        u = dict(short=DUID_SHORT.get(duid), nac=int(f["nac"][i]), duid=duid, k=int(records["k"][i]), dist=int(f["dist"][i]),
                 frame_dibits=int(f["frame_dibits"][i]), decoded=kind != 3, rs_bad=int(f["rs_bad"][i]), n_rs=int(f["n_rs"][i]),
                 n_fixed=int(f["n_fixed"][i]), n_bad=int(f["n_bad"][i]), nid_fix=int(f["nid_fix"][i]), nid_decoded=int(f["nid_decoded"][i]))
        pay = bytes(records["payload"][i])
        if kind == 0:
            u.update(mi=pay[:9], mfid=pay[9], algid=pay[10], kid=_bits(pay, 88, 104), tgid=_bits(pay, 104, 120))
        elif kind in (1, 2):
            u["lc"] = link_control(pay[:9])
            if kind == 1:
                u["lsd"] = bytes(records["lsd"][i])
        elif kind == 4:
            u.update(mi=pay[:9], algid=pay[9], kid=_bits(pay, 80, 96), lsd=bytes(records["lsd"][i]))
        units.append(u)
    return units


def prefilter_taps(channel_rate):
    """firdes.low_pass_2(1.0, 2 cr, cr / 2, 500, 30, WIN_BLACKMAN) (p25_control_demod.py:106-107): 69 taps at cr = 12500"""
    rate = 2 * channel_rate
    return native.design_low_pass_2(1.0, rate, channel_rate / 2.0, 500.0, 30.0, native.WIN_BLACKMAN)


def fm_gain(channel_rate):
    """quadrature_demod_cf gain of the C4FM path: 2 cr / (2 pi symbol_deviation) (p25_control_demod.py:120)"""
    return 2 * channel_rate / (2.0 * math.pi * SYMBOL_DEVIATION)


def symbol_taps(channel_rate, symbol_rate=SYMBOL_RATE):
    """(1/sps,)*sps with sps = 2 cr // symbol_rate (p25_control_demod.py:129-131): five taps of 0.2 at cr = 12500"""
    sps = (2 * channel_rate) // symbol_rate
    return [1.0 / sps] * sps


def _prefilter(fe, chan_id, channel_rate):
    # freq_xlating_fir_filter_ccc(1, taps, 0, 2 cr) on the channel's output (p25_control_demod.py:108)
    return fe.chan_open_taps(chan_id, 1, prefilter_taps(channel_rate), 0.0)


def cqpsk_front_half(fe, chan_id, channel_rate, nsamples=1024, reference=1.0):
    """the CQPSK (LSM / simulcast) front half on channel `chan_id` of Frontend `fe` (rate 2 channel_rate): the chained
    pre-filter, then feedforward_agc_cc(1024, 1.0) (p25_control_demod.py:146-149).  Returns the pre-filter channel's
    id: chan_read_agc on it gives what gardner_costas_cc consumes."""
    cid = _prefilter(fe, chan_id, channel_rate)
    fe.chan_agc(cid, nsamples, reference)
    return cid


def costas_params(channel_rate, symbol_rate=SYMBOL_RATE):
    """gardner_costas_cc's arguments as p25_control_demod.py:150-160 and logging_receiver.py:282-296 compute them, at a
    channel of 2 channel_rate samples per second: keyword arguments of Frontend.chan_costas"""
    rate = 2.0 * channel_rate
    gain_mu, alpha = 0.025, 0.04
    return dict(omega=rate / symbol_rate, gain_mu=gain_mu, gain_omega=0.1 * gain_mu * gain_mu, alpha=alpha,
                beta=0.125 * alpha * alpha, max_freq=2.0 * math.pi * 1200.0 / rate, omega_limit=0.005)


def cqpsk_demod(fe, chan_id, channel_rate, symbol_rate=SYMBOL_RATE, hard=False, tsbk=False, lc=False, es=False, erasures=False, nid=False, viterbi=False):
    """the whole CQPSK chain up to the slicer on channel `chan_id` of Frontend `fe`: the front half, then the Gardner /
    Costas stage (p25_control_demod.py:136-183).  Returns the pre-filter channel's id: chan_read_costas on it gives soft
    dibits at symbol_rate (slice_dibits turns them into dibits), chan_costas_state its carrier estimate.  hard=True also
    attaches the slicer behind the loop: chan_read_hard gives packed dibits, chan_read_sync where FRAME_SYNC ends; with
    tsbk=True as well the TSBK stage behind the slicer (chan_read_tsbk, tsdu_frames), or with lc=True the voice-channel
    stage (chan_read_p25lc, voice_units; es / erasures: its options, Frontend.chan_p25lc); the two exclude each other (ValueError).  nid=True: either stage decodes the NID's BCH word first (nid_decode is the host form).
    viterbi=True: the TSBK stage decodes a block's trellis by the least-cost path (trellis_decode is the host form)."""
    _one_decoder(tsbk, lc)
    cid = cqpsk_front_half(fe, chan_id, channel_rate)
    fe.chan_costas(cid, **costas_params(channel_rate, symbol_rate))
    if hard:
        _hard(fe, cid, native.READ_COSTAS, tsbk, lc, es, erasures, nid, viterbi)
    return cid


def slice_dibits(soft, levels=(-2.0, 0.0, 2.0, 4.0)):
    """op25.fsk4_slicer_fb(levels) (p25_control_demod.py:161): < levels[0] -> 3, < levels[1] -> 2, < levels[2] -> 0, else 1"""
    s = np.asarray(soft)
    return np.where(s < levels[0], 3, np.where(s < levels[1], 2, np.where(s < levels[2], 0, 1))).astype(np.uint8)


def c4fm_front_half(fe, chan_id, channel_rate, symbol_rate=SYMBOL_RATE):
    """the C4FM front half on channel `chan_id` of Frontend `fe`: the chained pre-filter, its discriminator and the
    boxcar symbol filter (p25_control_demod.py:118-135).  Returns the pre-filter channel's id: chan_read_sym on it gives
    what fsk4_demod_ff consumes."""
    cid = _prefilter(fe, chan_id, channel_rate)
    fe.chan_fm_filter(cid, fm_gain(channel_rate), symbol_taps(channel_rate, symbol_rate))
    return cid


def fsk4_params(channel_rate, symbol_rate=SYMBOL_RATE):
    """fsk4_demod_ff's arguments (p25_control_demod.py:135, logging_receiver.py:247: the rate 2 channel_rate and the symbol
    rate) and op25's loop constants: keyword arguments of Frontend.chan_fsk4"""
    return dict(sample_rate=2.0 * channel_rate, symbol_rate=float(symbol_rate), k_spread=0.01, k_timing=0.025, k_fine=0.125,
                k_coarse=0.00125, spread_min=1.6, spread_max=2.4)


def c4fm_demod(fe, chan_id, channel_rate, symbol_rate=SYMBOL_RATE, hard=False, tsbk=False, lc=False, es=False, erasures=False, nid=False, viterbi=False):
    """the whole C4FM chain up to the slicer on channel `chan_id` of Frontend `fe`: the front half, then the symbol loop
    (p25_control_demod.py:118-135).  Returns the pre-filter channel's id: chan_read_fsk4 on it gives soft dibits at
    symbol_rate (slice_dibits turns them into dibits), chan_fsk4_state its offset estimate (`coarse`).  hard=True also
    attaches the slicer behind the loop: chan_read_hard gives packed dibits, chan_read_sync where FRAME_SYNC ends; with
    tsbk=True as well the TSBK stage behind the slicer (chan_read_tsbk, tsdu_frames), or with lc=True the voice-channel
    stage (chan_read_p25lc, voice_units; es / erasures: its options, Frontend.chan_p25lc); the two exclude each other (ValueError).  nid=True: either stage decodes the NID's BCH word first (nid_decode is the host form).
    viterbi=True: the TSBK stage decodes a block's trellis by the least-cost path (trellis_decode is the host form)."""
    _one_decoder(tsbk, lc)
    cid = c4fm_front_half(fe, chan_id, channel_rate, symbol_rate)
    fe.chan_fsk4(cid, **fsk4_params(channel_rate, symbol_rate))
    if hard:
        _hard(fe, cid, native.READ_FSK4, tsbk, lc, es, erasures, nid, viterbi)
    return cid


def front_half(fe, chan_id, channel_rate, modulation):
    """the front half a demod of `modulation` ('C4FM' / 'CQPSK') runs, as p25_control_demod.py:118,136 picks it"""
    if modulation == "C4FM":
        return c4fm_front_half(fe, chan_id, channel_rate)
    if modulation == "CQPSK":
        return cqpsk_front_half(fe, chan_id, channel_rate)
    raise ValueError("unknown P25 modulation %r" % (modulation,))
