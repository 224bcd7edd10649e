"""The SmartNet and EDACS control demodulators behind a channel, on the GPU up to the slicer
(moto_control_demod.py:105-132, edacs_control_demod.py:82-112).  Both have one shape:

  quadrature_demod_cf(5) -> clock_recovery_mm_ff(rate / symbol_rate, 1.4395919, 0.5, 0.05, 0.005)
                         -> binary_slicer_fb -> unpacked_to_packed_bb(1, MSB_FIRST)

The discriminator and the Mueller and Mueller clock run per channel on the GPU (rcf_chan_clock_mm): a demod reads soft
symbols at 3600 or 9600 per second (chan_read_clock), slices and packs them (pack_bits) and does the packet framing -- or,
with hard=True, lets the GPU slice, pack and look for the frame sync (rcf_chan_slicer) and reads packed bits and the places
frames begin (chan_read_hard, chan_read_sync).  For EDACS the GPU goes one step further with frames=True: framing, the BCH
decode of the six copies and the election of the two messages (rcf_chan_edacs; chan_read_edacs, edacs_messages).  For
SmartNet likewise with osw=True: the 84-bit framing with its lock counter, deinterleave, the parity syndrome and its
correction (rcf_chan_osw; chan_read_osw, smartnet_osws)."""
import numpy as np

from . import native

QUAD_GAIN = 5.0              # moto_control_demod.py:105, edacs_control_demod.py:84
GAIN_OMEGA = 1.4395919       # moto_control_demod.py:113, edacs_control_demod.py:85 (the four constants below too)
MU = 0.5
GAIN_MU = 0.05
OMEGA_RELATIVE_LIMIT = 0.005
SMARTNET_SYNC, SMARTNET_SYNC_BITS = 0b10101100, 8      # moto_control_demod.py:216
# edacs_control_demod.py:523; the inverted word is searched as well with sync_both=1 (edacs_clock(frames=True))
EDACS_SYNC, EDACS_SYNC_BITS = 0b010101010101010101010111000100100101010101010101, 48


def smartnet_clock(fe, cid, channel_rate=25000, symbol_rate=3600.0, hard=False, osw=False):
    """clock_recovery_mm_ff(channel_rate / symbol_rate, ...) behind quadrature_demod_cf(5) on channel `cid` of Frontend
    `fe` (moto_control_demod.py:103-113: channel_rate = 2 x 12500, symbol_rate = 3600.0 at :50).  hard=True also attaches
    the slicer behind the clock: binary, exact matches of the 8-bit frame sync.  With osw=True as well the OSW stage sits
    behind it: chan_read_osw gives a record per frame, smartnet_osws the fields the reference publishes."""
    fe.chan_clock_mm(cid, channel_rate / symbol_rate, GAIN_OMEGA, MU, GAIN_MU, OMEGA_RELATIVE_LIMIT, QUAD_GAIN)
    if hard:
        fe.chan_slicer(cid, native.READ_CLOCK, native.SLICE_BINARY, sync_word=SMARTNET_SYNC, sync_bits=SMARTNET_SYNC_BITS)
        if osw:
            fe.chan_osw(cid)


def smartnet_osws(records):
    """records of the OSW stage (Frontend.chan_read_osw, native.OSW_DTYPE) -> list of (k, cmd, ind, lid, tg, status, bad,
    is_locked) in the stream's order: k the low 32 bits of the packet's sync position; cmd, ind ('G' / 'I'), lid, tg =
    lid & 0xfff0 and status = lid & 0xf as receive_engine publishes them (moto_control_demod.py:325-339); bad: the packet
    counted into packets_bad; is_locked as the frame left it"""
    records = np.asarray(records, dtype=native.OSW_DTYPE)
    f = native.osw_fields(records)
    return [(int(r["k"]), int(r["cmd"]), "G" if ind else "I", int(r["lid"]), int(r["lid"]) & 0xfff0, int(r["lid"]) & 0xf,
             bool(bad), bool(lk)) for r, ind, bad, lk in zip(records, f["individual"], f["bad"], f["is_locked"])]


def edacs_clock(fe, cid, receive_rate=25000, symbol_rate=9600.0, hard=False, frames=False, esk=False):
    """the same behind an EDACS control channel (edacs_control_demod.py:76,85: receive_rate = 2 x 12500, symbol_rate
    the system's, 9600 or 4800).  hard=True also attaches the slicer behind the clock: binary, exact matches of the
    48-bit frame sync.  With frames=True as well the slicer searches both polarities (get_next_frame accepts either) and the
    EDACS stage sits behind it: chan_read_edacs gives a record per frame, edacs_messages the reference's strings; esk: the
    system's extended-addressing flag."""
    fe.chan_clock_mm(cid, receive_rate / symbol_rate, GAIN_OMEGA, MU, GAIN_MU, OMEGA_RELATIVE_LIMIT, QUAD_GAIN)
    if hard:
        fe.chan_slicer(cid, native.READ_CLOCK, native.SLICE_BINARY, sync_word=EDACS_SYNC, sync_bits=EDACS_SYNC_BITS,
                       sync_both=1 if frames else 0)
        if frames:
            fe.chan_edacs(cid, esk=esk)


def edacs_messages(records):
    """records of the EDACS stage (Frontend.chan_read_edacs, native.EDACS_DTYPE) -> list of (k, inverted, m1, m2) in the
    stream's order: k the low 32 bits of the sync word's last bit, m the 40-character bit string packet_framer returns for
    the message, or -1 where the election gave none"""
    records = np.asarray(records, dtype=native.EDACS_DTYPE)
    f = native.edacs_fields(records)
    out = []
    for i in range(len(records)):
        ms = []
        for name, has in (("m1", f["has_m1"][i]), ("m2", f["has_m2"][i])):
            ms.append("".join("{0:08b}".format(int(o)) for o in records[name][i][:5]) if has else -1)
        out.append((int(records["k"][i]), bool(f["inverted"][i]), ms[0], ms[1]))
    return out


def pack_bits(soft, carry=None):
    """binary_slicer_fb -> unpacked_to_packed_bb(1, GR_MSB_FIRST) (moto_control_demod.py:114-115,
    edacs_control_demod.py:86-90) over the soft symbols of one read: bit = soft >= 0, eight bits per byte, first bit in
    the byte's top place.  `carry` holds the 0 .. 7 bits the call before left over (a uint8 array of 0 / 1); returns
    (bytes as a uint8 array, the new carry)."""
    bits = (np.asarray(soft, dtype=np.float32) >= 0).astype(np.uint8)
    if carry is not None and len(carry):
        bits = np.concatenate([np.asarray(carry, dtype=np.uint8), bits])
    whole = len(bits) // 8 * 8
    return np.packbits(bits[:whole]), bits[whole:].copy()
