"""ctypes binding of librcf.so (include/rcf.h).  Thin: numpy arrays in/out, no arithmetic here.

There is no CPU fallback: if librcf.so is missing the import of any compute entry point raises
RuntimeError, and rcf_open() fails without a HIP device.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RCF_LIBRCF: another build of the same library (the AddressSanitizer build of the host layer, tools/asan_gpu.sh)
_SO = os.environ.get("RCF_LIBRCF") or os.path.join(_HERE, "librcf.so")
_lib = None

RCF_OK, RCF_EINVAL, RCF_ENOMEM, RCF_EHIP, RCF_ENOCHAN = 0, -1, -2, -3, -4
RCF_ECAP, RCF_ESTATE, RCF_EAGAIN, RCF_ERANGE = -5, -6, -7, -8
WIN_HAMMING, WIN_BLACKMAN, WIN_KAISER, WIN_BLACKMAN_HARRIS = 0, 2, 4, 5
FIR_LOW_PASS, FIR_HIGH_PASS = 0, 1
SRC_PFB_BIN0 = 0x40000000

# every symbol include/rcf.h declares (tests check the library exports all of them)
SYMBOLS = [
    "rcf_version", "rcf_last_error", "rcf_device_count", "rcf_device_pci_bus_id", "rcf_design_low_pass_2", "rcf_design_window",
    "rcf_channel_params", "rcf_channel_params_ex", "rcf_set_decim_rule", "rcf_open", "rcf_open_ex", "rcf_close", "rcf_sync", "rcf_stream", "rcf_device",
    "rcf_push_iq", "rcf_ingest_ptr", "rcf_commit", "rcf_samples_in", "rcf_chan_open", "rcf_chan_open_taps",
    "rcf_chan_set_offset", "rcf_chan_close", "rcf_chan_info", "rcf_chan_produced", "rcf_chan_start", "rcf_chan_read_many", "rcf_chan_read_iq",
    "rcf_chan_read_fm", "rcf_chan_rings", "rcf_source_shift", "rcf_pfb_open", "rcf_pfb_close",
    "rcf_pfb_produced", "rcf_pfb_read_bin", "rcf_pfb_rings", "rcf_pfb_fm_enable", "rcf_pfb_read_fm", "rcf_pfb_fm_ring", "rcf_pfb_fm_lost", "rcf_pfb_chan_open", "rcf_scan_start",
    "rcf_scan_result", "rcf_scan_frames_done", "rcf_scan_result_device", "rcf_find_peaks",
    "rcf_peak_frequency", "rcf_scan_find_peaks", "rcf_timing_enable", "rcf_timing_read",
    "rcf_ingest_write", "rcf_push_raw", "rcf_chan_fm_filter", "rcf_chan_read_sym", "rcf_chan_fm_level",
    "rcf_chan_agc", "rcf_chan_read_agc", "rcf_chan_agc_ring",
    "rcf_chan_clock_mm", "rcf_chan_clock_produced", "rcf_chan_read_clock", "rcf_chan_clock_ring", "rcf_design_mmse_interpolator",
    "rcf_chan_costas", "rcf_chan_costas_state", "rcf_chan_read_costas", "rcf_chan_costas_ring",
    "rcf_chan_fsk4", "rcf_chan_fsk4_state", "rcf_chan_read_fsk4", "rcf_chan_fsk4_ring",
    "rcf_chan_slicer", "rcf_chan_slicer_state", "rcf_chan_read_hard", "rcf_chan_read_sync", "rcf_chan_slicer_rings",
    "rcf_chan_tsbk", "rcf_chan_tsbk_state", "rcf_chan_read_tsbk", "rcf_chan_tsbk_ring",
    "rcf_chan_edacs", "rcf_chan_edacs_state", "rcf_chan_read_edacs", "rcf_chan_edacs_ring",
    "rcf_chan_osw", "rcf_chan_osw_state", "rcf_chan_read_osw", "rcf_chan_osw_ring",
    "rcf_chan_tsbk_ex", "rcf_chan_p25lc_ex", "rcf_chan_nid_state",
    "rcf_chan_tsbk_opt", "rcf_chan_trellis_state",
    "rcf_chan_p25lc", "rcf_chan_p25lc_opt", "rcf_chan_p25lc_state", "rcf_chan_read_p25lc", "rcf_chan_p25lc_ring",
    "rcf_design_firdes", "rcf_design_optfir_low_pass", "rcf_design_fm_deemph", "rcf_design_resampler", "rcf_chan_audio_open",
    "rcf_chan_audio_close", "rcf_chan_audio_produced", "rcf_chan_read_audio",
    "rcf_host_alloc", "rcf_host_free", "rcf_comm_unique_id", "rcf_comm_init", "rcf_comm_destroy", "rcf_comm_size",
    "rcf_allgather_peaks", "rcf_allreduce_max", "rcf_pfb_tap_open", "rcf_chan_set_fm_only", "rcf_pfb_shape_supported", "rcf_pfb_shape_family",
    "rcf_pfb_tap_leakage", "rcf_set_rotator", "rcf_timing_stride", "rcf_set_stage2_lag",
    "rcf_group_open", "rcf_group_close", "rcf_group_size", "rcf_group_push", "rcf_group_commit", "rcf_group_read_many",
    "rcf_chan_squelch", "rcf_chan_squelch_state", "rcf_pfb_squelch", "rcf_pfb_squelch_read", "rcf_pfb_squelch_segment",
    "rcf_chan_capture", "rcf_chan_capture_state", "rcf_chan_read_capture", "rcf_chan_read_capture_rec", "rcf_chan_capture_rings",
    "rcf_group_sync", "rcf_pump_start", "rcf_pump_stats", "rcf_pump_written", "rcf_pump_read", "rcf_pump_read_many", "rcf_pump_subscribe", "rcf_pump_unsubscribe", "rcf_pump_stop",
    "rcf_pump_subscribe_hard",
]
FMT_CF32, FMT_U8, FMT_S8, FMT_S16 = 0, 1, 2, 3
READ_IQ, READ_FM, READ_AGC = 0, 1, 2
# the streams of a channel's stages (RCF_READ_SYM .. RCF_READ_AUDIO): float32 rows of the batched readers and the pump
READ_SYM, READ_CLOCK, READ_COSTAS, READ_FSK4, READ_AUDIO = 16, 17, 18, 19, 20
_STAGE_WHAT = {"sym": READ_SYM, "clock": READ_CLOCK, "costas": READ_COSTAS, "fsk4": READ_FSK4, "audio": READ_AUDIO}
# the slicer's two streams (RCF_HARD_BITS, RCF_HARD_SYNC): uint32 rows of the batched readers; the pump delivers them, and the
# records below, through Pump.subscribe (rcf_pump_subscribe_hard), never as the `what` it is started with
HARD_BITS, HARD_SYNC = 32, 33
# the stream of the TSBK stage behind a slicer (RCF_HARD_TSBK): records of 8 uint32, batched the same way
HARD_TSBK = 48
# ... and of the EDACS stage (RCF_HARD_EDACS): records of 8 uint32 too, one per frame
HARD_EDACS = 49
# ... and of the SmartNet OSW stage (RCF_HARD_OSW): records of 8 uint32 as well, one per frame
HARD_OSW = 51
# ... and of the P25 voice stage (RCF_HARD_P25LC): records of 8 uint32, one per frame
HARD_P25LC = 53
P25LC_ES, P25LC_ERASURES = 1, 2   # rcf_chan_p25lc_opt's options (RCF_P25LC_*)
# the two streams of the capture stage (rcf_chan_capture): RCF_READ_CAPTURE, cf32 samples, and RCF_HARD_CAPTURE, records of
# CAPTURE_REC_DTYPE; the pump delivers the first through rcf_pump_subscribe and the second through rcf_pump_subscribe_hard
READ_CAPTURE, HARD_CAPTURE = 24, 56
CAPTURE_OPEN, CAPTURE_CLOSE = 1, 2
_CAPTURE_WHAT = {"capture": READ_CAPTURE, "capture_rec": HARD_CAPTURE}
_HARD_WHAT = {"hard": HARD_BITS, "sync": HARD_SYNC, "tsbk": HARD_TSBK, "edacs": HARD_EDACS, "osw": HARD_OSW, "p25lc": HARD_P25LC}
# a record of RCF_HARD_TSBK (rcf.h at rcf_chan_tsbk): word 0 (see tsbk_fields), the low 32 bits of k, the 12 decoded octets,
# the NID's 8 octets, frame_dibits
TSBK_DTYPE = np.dtype([("flags", "<u4"), ("k", "<u4"), ("octets", "u1", (12,)), ("nid", "u1", (8,)), ("frame_dibits", "<u4")])
# a record of RCF_HARD_EDACS (rcf.h at rcf_chan_edacs): word 0 (see edacs_fields), the low 32 bits of k, the five octets of
# m1 and of m2, each in a field of eight
EDACS_DTYPE = np.dtype([("flags", "<u4"), ("k", "<u4"), ("m1", "u1", (8,)), ("m2", "u1", (8,)), ("zero", "<u4", (2,))])
# a record of RCF_HARD_OSW (rcf.h at rcf_chan_osw): word 0 (see osw_fields), the low 32 bits of the packet's sync position,
# lid and cmd, the 38 corrected data bits and the 38 syndrome bits as octets (five each, in a field of eight), locked
OSW_DTYPE = np.dtype([("flags", "<u4"), ("k", "<u4"), ("lid", "<u2"), ("cmd", "<u2"), ("data", "u1", (8,)), ("psyn", "u1", (8,)),
                      ("locked", "<i4")])
# a record of RCF_HARD_P25LC (rcf.h at rcf_chan_p25lc): word 0 (see p25lc_fields), the low 32 bits of k, the payload's octets
# (15 of an HDU, 9 of an LDU1 or a TLC, 12 of an LDU2, zero padded), the LDU's four LSD octets, frame_dibits and the inner words' counts
P25LC_DTYPE = np.dtype([("flags", "<u4"), ("k", "<u4"), ("payload", "u1", (16,)), ("lsd", "u1", (4,)), ("tail", "<u4")])
SLICE_BINARY, SLICE_FSK4 = 1, 2
T_FIR, T_PFB, T_FIR_DERIVED, T_DISC, T_SCAN_FFT, T_SCAN_MOVSUM, T_HISTORY, T_FIR_MFMA, T_AUDIO, T_TAPS, T_CLOCK, T_COSTAS, T_FSK4, T_SLICE = range(14)


class AudioParams(C.Structure):
    """rcf_audio_params_t (include/rcf.h)"""
    _fields_ = [("squelch_db", C.c_double), ("squelch_alpha", C.c_double), ("quad_gain", C.c_float),
                ("reserved_", C.c_int), ("deemph_b", C.c_double * 2), ("deemph_a", C.c_double * 2),
                ("lpf_taps", C.POINTER(C.c_float)), ("n_lpf", C.c_int), ("n_hpf", C.c_int),
                ("hpf_taps", C.POINTER(C.c_float)), ("rs_taps", C.POINTER(C.c_float)), ("n_rs", C.c_int),
                ("interpolation", C.c_int), ("decimation", C.c_int), ("reserved2_", C.c_int)]


class ClockMmParams(C.Structure):
    """rcf_clock_mm_params_t (include/rcf.h)"""
    _fields_ = [("gain", C.c_float), ("omega", C.c_float), ("gain_omega", C.c_float), ("mu", C.c_float),
                ("gain_mu", C.c_float), ("omega_relative_limit", C.c_float), ("reserved_", C.c_int),
                ("interp_taps", C.POINTER(C.c_float))]


class CostasParams(C.Structure):
    """rcf_costas_params_t (include/rcf.h)"""
    _fields_ = [("omega", C.c_float), ("gain_mu", C.c_float), ("gain_omega", C.c_float), ("alpha", C.c_float),
                ("beta", C.c_float), ("max_freq", C.c_float), ("omega_limit", C.c_float), ("reserved_", C.c_int),
                ("interp_taps", C.POINTER(C.c_float))]


class CostasState(C.Structure):
    """rcf_costas_state_t (include/rcf.h)"""
    _fields_ = [("n_symbols", C.c_int64), ("n_slips", C.c_int64), ("mu", C.c_float), ("omega", C.c_float),
                ("freq", C.c_float), ("phase", C.c_float)]


def _bank_arg(interp_taps):
    """a caller's [129, 8] interpolator bank as the contiguous float32 array a params struct points into (keep it while
    the struct is in use), or None"""
    if interp_taps is None:
        return None
    taps = np.ascontiguousarray(interp_taps, dtype=np.float32)
    if taps.shape != (129, 8):
        raise ValueError("interp_taps must be a [129, 8] array")
    return taps


def _state_dict(st):
    """a ctypes state struct as a dict of its fields"""
    return {k: getattr(st, k) for k, _ in st._fields_}


def costas_params_struct(omega, gain_mu, gain_omega, alpha, beta, max_freq, omega_limit, interp_taps=None):
    """-> (CostasParams, the array its interp_taps points into or None: keep it while the struct is in use)"""
    p = CostasParams()
    p.omega, p.gain_mu, p.gain_omega, p.alpha = float(omega), float(gain_mu), float(gain_omega), float(alpha)
    p.beta, p.max_freq, p.omega_limit = float(beta), float(max_freq), float(omega_limit)
    taps = _bank_arg(interp_taps)
    if taps is not None:
        p.interp_taps = taps.ctypes.data_as(C.POINTER(C.c_float))
    return p, taps


class Fsk4Params(C.Structure):
    """rcf_fsk4_params_t (include/rcf.h)"""
    _fields_ = [("sample_rate", C.c_double), ("symbol_rate", C.c_double), ("k_spread", C.c_double), ("k_timing", C.c_double),
                ("k_fine", C.c_double), ("k_coarse", C.c_double), ("spread_min", C.c_double), ("spread_max", C.c_double),
                ("interp_taps", C.POINTER(C.c_float)), ("reserved_", C.c_int)]


class Fsk4State(C.Structure):
    """rcf_fsk4_state_t (include/rcf.h)"""
    _fields_ = [("n_symbols", C.c_int64), ("n_slips", C.c_int64), ("clock", C.c_double), ("spread", C.c_double),
                ("fine", C.c_double), ("coarse", C.c_double)]


def fsk4_params_struct(sample_rate, symbol_rate, k_spread, k_timing, k_fine, k_coarse, spread_min, spread_max, interp_taps=None):
    """-> (Fsk4Params, the array its interp_taps points into or None: keep it while the struct is in use)"""
    p = Fsk4Params()
    p.sample_rate, p.symbol_rate, p.k_spread, p.k_timing = float(sample_rate), float(symbol_rate), float(k_spread), float(k_timing)
    p.k_fine, p.k_coarse, p.spread_min, p.spread_max = float(k_fine), float(k_coarse), float(spread_min), float(spread_max)
    taps = _bank_arg(interp_taps)
    if taps is not None:
        p.interp_taps = taps.ctypes.data_as(C.POINTER(C.c_float))
    return p, taps


class SquelchParams(C.Structure):
    """rcf_squelch_params_t (include/rcf.h)"""
    _fields_ = [("threshold_db", C.c_double), ("alpha", C.c_double)]


class SquelchState(C.Structure):
    """rcf_squelch_state_t (include/rcf.h)"""
    _fields_ = [("level", C.c_double), ("n_seen", C.c_int64), ("n_open", C.c_int64), ("first_open", C.c_int64),
                ("last_open", C.c_int64), ("unmuted", C.c_int32), ("reserved_", C.c_int32)]


class CaptureParams(C.Structure):
    """rcf_capture_params_t (include/rcf.h)"""
    _fields_ = [("threshold_db", C.c_double), ("alpha", C.c_double), ("pre", C.c_int64), ("hang", C.c_int64),
                ("capacity", C.c_uint32), ("rec_capacity", C.c_uint32)]


class CaptureState(C.Structure):
    """rcf_capture_state_t (include/rcf.h)"""
    _fields_ = [("level", C.c_double), ("n_seen", C.c_int64), ("n_decided", C.c_int64), ("n_kept", C.c_int64),
                ("n_records", C.c_int64), ("n_windows", C.c_int64), ("last_open", C.c_int64), ("in_window", C.c_int32),
                ("unmuted", C.c_int32)]


class SlicerParams(C.Structure):
    """rcf_slicer_params_t (include/rcf.h)"""
    _fields_ = [("source", C.c_int), ("mode", C.c_int), ("levels", C.c_float * 4), ("sync_word", C.c_uint64),
                ("sync_bits", C.c_int), ("sync_max_errors", C.c_int), ("hit_capacity", C.c_int), ("sync_both", C.c_int)]


class SlicerState(C.Structure):
    """rcf_slicer_state_t (include/rcf.h)"""
    _fields_ = [("n_symbols", C.c_int64), ("n_words", C.c_int64), ("n_hits", C.c_int64)]


class TsbkParams(C.Structure):
    """rcf_tsbk_params_t (include/rcf.h)"""
    _fields_ = [("capacity", C.c_int), ("reserved_", C.c_int * 3)]


class TsbkState(C.Structure):
    """rcf_tsbk_state_t (include/rcf.h)"""
    _fields_ = [("n_records", C.c_int64), ("n_frames", C.c_int64), ("n_blocks", C.c_int64), ("n_crc_bad", C.c_int64),
                ("n_lost", C.c_int64)]


class NidState(C.Structure):
    """rcf_nid_state_t (include/rcf.h)"""
    _fields_ = [("n_decoded", C.c_int64), ("n_fixed", C.c_int64), ("n_bits", C.c_int64), ("n_bad", C.c_int64)]


class TrellisState(C.Structure):
    """rcf_trellis_state_t (include/rcf.h)"""
    _fields_ = [("n_decoded", C.c_int64), ("n_clean", C.c_int64), ("n_bits", C.c_int64), ("n_words", C.c_int64)]


def trellis_fields(records):
    """what RCF_TRELLIS_VITERBI adds to word 7 of TSBK records (TSBK_DTYPE) -> dict of arrays: cost (the bits in which the
    block's 196 differ from the decoded path's, 0 .. 196) and viterbi (the block went through that decoder); both are 0 in a
    frame record and for a stage attached without the option"""
    t = np.asarray(records["frame_dibits"], dtype=np.uint32)
    return dict(cost=((t >> 21) & 255).astype(np.uint8), viterbi=((t >> 29) & 1).astype(np.uint8))


def tsbk_fields(records):
    """word 0 of TSBK records taken apart -> dict of arrays: b (3: a frame record), crc_bad, next_bit, n_inexact, dist, duid, nac"""
    f = np.asarray(records["flags"], dtype=np.uint32)
    return dict(b=(f & 3).astype(np.uint8), crc_bad=((f >> 2) & 1).astype(np.uint8), next_bit=((f >> 3) & 1).astype(np.uint8),
                n_inexact=((f >> 4) & 63).astype(np.uint8), dist=((f >> 10) & 63).astype(np.uint8),
                duid=((f >> 16) & 15).astype(np.uint8), nac=(f >> 20).astype(np.uint16))


def nid_fields(records):
    """what RCF_NID_BCH adds to TSBK records (TSBK_DTYPE) or P25 voice records (P25LC_DTYPE) -> dict of arrays: nid_fix (bits
    the NID's BCH decoder changed, 15: no code word within its bound), nid_decoded (the NID went through that decoder; both
    are 0 for a stage attached without the option) and frame_dibits (word 7's low 16 bits: in a TSBK record the option's
    bits stand above them)"""
    if "frame_dibits" in records.dtype.names:
        t = np.asarray(records["frame_dibits"], dtype=np.uint32)
        fix, decoded = (t >> 16) & 15, (t >> 20) & 1
    else:
        t = np.asarray(records["tail"], dtype=np.uint32)
        fix, decoded = t >> 28, (np.asarray(records["flags"], dtype=np.uint32) >> 9) & 1
    return dict(nid_fix=fix.astype(np.uint8), nid_decoded=decoded.astype(np.uint8), frame_dibits=(t & 0xffff).astype(np.uint16))


class EdacsParams(C.Structure):
    """rcf_edacs_params_t (include/rcf.h)"""
    _fields_ = [("capacity", C.c_int), ("esk", C.c_int), ("reserved_", C.c_int * 2)]


class EdacsState(C.Structure):
    """rcf_edacs_state_t (include/rcf.h)"""
    _fields_ = [("n_records", C.c_int64), ("n_frames", C.c_int64), ("n_msgs", C.c_int64), ("n_msgs_none", C.c_int64),
                ("n_lost", C.c_int64)]


def edacs_fields(records):
    """word 0 of EDACS records taken apart -> dict of arrays: inverted, has_m1, has_m2, dist, status ([n, 6]: per copy 0 clean
    or stands, 1 one position, 2 two positions, 3 failed)"""
    f = np.asarray(records["flags"], dtype=np.uint32)
    return dict(inverted=(f & 1).astype(np.uint8), has_m1=((f >> 1) & 1).astype(np.uint8), has_m2=((f >> 2) & 1).astype(np.uint8),
                dist=((f >> 4) & 63).astype(np.uint8),
                status=np.stack([((f >> (10 + 2 * c)) & 3).astype(np.uint8) for c in range(6)], axis=-1))


class OswParams(C.Structure):
    """rcf_osw_params_t (include/rcf.h)"""
    _fields_ = [("capacity", C.c_int), ("reserved_", C.c_int * 3)]


class OswState(C.Structure):
    """rcf_osw_state_t (include/rcf.h)"""
    _fields_ = [("n_records", C.c_int64), ("n_frames", C.c_int64), ("n_bad", C.c_int64), ("n_rejects", C.c_int64),
                ("n_lost", C.c_int64), ("locked", C.c_int32), ("is_locked", C.c_int32)]


def osw_fields(records):
    """word 0 of OSW records taken apart -> dict of arrays: at_cursor (the sync word stood at the cursor), bad (syndrome
    nonzero), is_locked, individual, flipped (data bits corrected), syn_bits (set syndrome bits), rel (bits between the cursor
    and the sync word; 65535: that many or more, or not determined)"""
    f = np.asarray(records["flags"], dtype=np.uint32)
    return dict(at_cursor=(f & 1).astype(np.uint8), bad=((f >> 1) & 1).astype(np.uint8), is_locked=((f >> 2) & 1).astype(np.uint8),
                individual=((f >> 3) & 1).astype(np.uint8), flipped=((f >> 4) & 63).astype(np.uint8),
                syn_bits=((f >> 10) & 63).astype(np.uint8), rel=(f >> 16).astype(np.uint16))


class P25lcParams(C.Structure):
    """rcf_p25lc_params_t (include/rcf.h)"""
    _fields_ = [("capacity", C.c_int), ("correct", C.c_int), ("reserved_", C.c_int * 2)]


class P25lcState(C.Structure):
    """rcf_p25lc_state_t (include/rcf.h)"""
    _fields_ = [("n_records", C.c_int64), ("n_frames", C.c_int64), ("n_decoded", C.c_int64), ("n_rs_bad", C.c_int64),
                ("n_lost", C.c_int64)]


def p25lc_fields(records):
    """words 0 and 7 of P25 voice records taken apart -> dict of arrays: kind (0 HDU, 1 LDU1, 2 TLC, 3: a frame record, 4 LDU2:
    its third bit is word 0 bit 3), rs_bad, n_rs (five bits, the fifth is word 0 bit 8), dist, duid, nac, frame_dibits, n_fixed,
    n_bad (inner words corrected / given up).  What RCF_NID_BCH adds: nid_fields"""
    f = np.asarray(records["flags"], dtype=np.uint32)
    t = np.asarray(records["tail"], dtype=np.uint32)
    return dict(kind=((f & 3) | ((f >> 1) & 4)).astype(np.uint8), rs_bad=((f >> 2) & 1).astype(np.uint8),
                n_rs=(((f >> 4) & 15) | ((f >> 4) & 16)).astype(np.uint8),
                dist=((f >> 10) & 63).astype(np.uint8), duid=((f >> 16) & 15).astype(np.uint8), nac=(f >> 20).astype(np.uint16),
                frame_dibits=(t & 0xffff).astype(np.uint16), n_fixed=((t >> 16) & 63).astype(np.uint8),
                n_bad=((t >> 22) & 63).astype(np.uint8))


# a record of RCF_HARD_CAPTURE (rcf_capture_rec_t, rcf.h at rcf_chan_capture)
CAPTURE_REC_DTYPE = np.dtype([("kind", "<u4"), ("n_open", "<u4"), ("sample", "<i8"), ("pos", "<i8"), ("peak", "<f4"), ("reserved_", "<u4")])
_RECORD_DTYPE = {HARD_TSBK: TSBK_DTYPE, HARD_EDACS: EDACS_DTYPE, HARD_OSW: OSW_DTYPE, HARD_P25LC: P25LC_DTYPE, HARD_CAPTURE: CAPTURE_REC_DTYPE}


def widen_hits(items, n_symbols):
    """the hit ring's uint32 items -> (k as int64, dist as uint8): k is the largest value <= n_symbols - 1 with the item's low
    26 bits (rcf.h at rcf_chan_slicer), n_symbols the stage's count when the items were read or later"""
    items = np.asarray(items, dtype=np.uint32)
    low = (items & np.uint32(0x3ffffff)).astype(np.int64)
    last = int(n_symbols) - 1
    k = low + ((last - low) >> 26 << 26)
    return k, (items >> np.uint32(26)).astype(np.uint8)


class PumpConfig(C.Structure):
    """rcf_pump_config_t (include/rcf.h)"""
    _fields_ = [("block_samples", C.c_size_t), ("fmt", C.c_int), ("scale", C.c_float), ("offset", C.c_float),
                ("samp_rate", C.c_double), ("rings", C.POINTER(C.c_void_p)), ("ring_blocks", C.POINTER(C.c_size_t)),
                ("phase_s", C.POINTER(C.c_double)), ("written", C.POINTER(C.c_void_p)), ("what", C.c_int),
                ("gain", C.c_float), ("read_members", C.POINTER(C.c_int)), ("read_chans", C.POINTER(C.c_int)),
                ("n_read", C.c_int), ("out_ring_samples", C.c_size_t), ("n_blocks", C.c_int64),
                ("warm_blocks", C.c_int64), ("max_batch", C.c_int), ("cpu", C.c_int), ("start_delay_s", C.c_double),
                ("batch_window_s", C.c_double), ("rt_priority", C.c_int), ("spin_us", C.c_int), ("max_read", C.c_int)]


class PumpStats(C.Structure):
    """rcf_pump_stats_t (include/rcf.h)"""
    _fields_ = [("blocks_done", C.c_int64), ("blocks_judged", C.c_int64), ("late", C.c_int64), ("overruns", C.c_int64),
                ("group_blocks", C.c_int64), ("max_batch", C.c_int64), ("samples_out", C.c_int64),
                ("latency_ms_p50", C.c_double), ("latency_ms_p99", C.c_double), ("latency_ms_max", C.c_double),
                ("host_plan_ms", C.c_double), ("host_wait_ms", C.c_double), ("elapsed_s", C.c_double),
                ("max_plan_ms", C.c_double), ("max_wait_ms", C.c_double), ("max_sleep_overshoot_ms", C.c_double),
                ("slow_plans", C.c_int64), ("slow_waits", C.c_int64), ("slow_sleeps", C.c_int64),
                ("rt_priority_granted", C.c_int),
                ("running", C.c_int), ("error", C.c_int),
                ("cpu", C.c_int), ("runq_ms_total", C.c_double), ("slow_wait_ms_total", C.c_double),
                ("runq_ms_in_slow_waits", C.c_double), ("slow_sleep_ms_total", C.c_double),
                ("runq_ms_in_slow_sleeps", C.c_double), ("involuntary_switches", C.c_int64)]


class RcfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("librcf error %d: %s" % (code, msg))
        self.code = code


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise RuntimeError("librcf.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`"
                           % _SO)
    L = C.CDLL(_SO)
    fp, vp, i64, sz = C.POINTER(C.c_float), C.c_void_p, C.c_int64, C.c_size_t
    ip = C.POINTER(C.c_int)
    sig = {
        "rcf_version": (C.c_char_p, []),
        "rcf_last_error": (C.c_char_p, []),
        "rcf_device_count": (C.c_int, []),
        "rcf_device_pci_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
        "rcf_design_low_pass_2": (C.c_int, [C.c_double] * 5 + [C.c_int, fp, C.c_int]),
        "rcf_design_window": (C.c_int, [C.c_int, C.c_int, fp]),
        "rcf_channel_params": (C.c_int, [C.c_double, C.c_int, ip, ip]),
        "rcf_channel_params_ex": (C.c_int, [C.c_double, C.c_int, C.c_int, ip, ip, C.POINTER(C.c_double)]),
        "rcf_set_decim_rule": (C.c_int, [vp, C.c_int]),
        "rcf_open": (C.c_int, [C.c_int, C.c_double, C.c_double, C.POINTER(vp)]),
        "rcf_open_ex": (C.c_int, [C.c_int, C.c_double, C.c_double, sz, sz, sz, C.POINTER(vp)]),
        "rcf_close": (C.c_int, [vp]),
        "rcf_set_rotator": (C.c_int, [vp, C.c_int]),
        "rcf_set_stage2_lag": (C.c_int, [vp, C.c_int]),
        "rcf_sync": (C.c_int, [vp]),
        "rcf_stream": (vp, [vp]),
        "rcf_device": (C.c_int, [vp]),
        "rcf_push_iq": (C.c_int, [vp, fp, sz]),
        "rcf_ingest_ptr": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz)]),
        "rcf_commit": (C.c_int, [vp, sz]),
        "rcf_ingest_write": (C.c_int, [vp, fp, sz, sz]),
        "rcf_push_raw": (C.c_int, [vp, vp, sz, C.c_int, C.c_float, C.c_float]),
        "rcf_chan_fm_filter": (C.c_int, [vp, C.c_int, C.c_float, fp, C.c_int]),
        "rcf_chan_read_sym": (i64, [vp, C.c_int, fp, sz]),
        "rcf_chan_agc": (C.c_int, [vp, C.c_int, C.c_int, C.c_float]),
        "rcf_chan_read_agc": (i64, [vp, C.c_int, fp, sz]),
        "rcf_chan_agc_ring": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]),
        "rcf_chan_clock_mm": (C.c_int, [vp, C.c_int, C.POINTER(ClockMmParams)]),
        "rcf_chan_clock_produced": (C.c_int, [vp, C.c_int, C.POINTER(i64), C.POINTER(i64)]),
        "rcf_chan_read_clock": (i64, [vp, C.c_int, fp, sz]),
        "rcf_chan_clock_ring": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]),
        "rcf_chan_costas": (C.c_int, [vp, C.c_int, C.POINTER(CostasParams)]),
        "rcf_chan_costas_state": (C.c_int, [vp, C.c_int, C.POINTER(CostasState)]),
        "rcf_chan_read_costas": (i64, [vp, C.c_int, fp, sz]),
        "rcf_chan_costas_ring": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]),
        "rcf_chan_fsk4": (C.c_int, [vp, C.c_int, C.POINTER(Fsk4Params)]),
        "rcf_chan_fsk4_state": (C.c_int, [vp, C.c_int, C.POINTER(Fsk4State)]),
        "rcf_chan_read_fsk4": (i64, [vp, C.c_int, fp, sz]),
        "rcf_chan_fsk4_ring": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]),
        "rcf_chan_slicer": (C.c_int, [vp, C.c_int, C.POINTER(SlicerParams)]),
        "rcf_chan_slicer_state": (C.c_int, [vp, C.c_int, C.POINTER(SlicerState)]),
        "rcf_chan_read_hard": (i64, [vp, C.c_int, C.POINTER(C.c_uint32), sz]),
        "rcf_chan_read_sync": (i64, [vp, C.c_int, C.POINTER(C.c_uint32), sz]),
        "rcf_chan_slicer_rings": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]),
        "rcf_design_mmse_interpolator": (C.c_int, [C.c_int, C.c_int, C.c_double, fp, C.c_int]),
        "rcf_chan_fm_level": (C.c_int, [vp, C.c_int, C.c_float, C.c_int, fp]),
        "rcf_design_firdes": (C.c_int, [C.c_int] + [C.c_double] * 4 + [C.c_int, C.c_double, fp, C.c_int]),
        "rcf_design_optfir_low_pass": (C.c_int, [C.c_double] * 6 + [fp, C.c_int]),
        "rcf_design_fm_deemph": (C.c_int, [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "rcf_design_resampler": (C.c_int, [C.c_int, C.c_int, ip, ip, fp, C.c_int]),
        "rcf_chan_audio_open": (C.c_int, [vp, C.c_int, C.POINTER(AudioParams)]),
        "rcf_chan_audio_close": (C.c_int, [vp, C.c_int]),
        "rcf_chan_audio_produced": (C.c_int, [vp, C.c_int, C.POINTER(i64), C.POINTER(i64)]),
        "rcf_chan_read_audio": (i64, [vp, C.c_int, fp, sz]),
        "rcf_samples_in": (i64, [vp]),
        "rcf_chan_open": (C.c_int, [vp, C.c_int, C.c_double, ip]),
        "rcf_chan_open_taps": (C.c_int, [vp, C.c_int, C.c_int, fp, C.c_int, C.c_double, ip]),
        "rcf_chan_set_offset": (C.c_int, [vp, C.c_int, C.c_double]),
        "rcf_chan_close": (C.c_int, [vp, C.c_int]),
        "rcf_chan_info": (C.c_int, [vp, C.c_int, ip, ip, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "rcf_chan_produced": (i64, [vp, C.c_int]),
        "rcf_chan_start": (i64, [vp, C.c_int]),
        "rcf_chan_read_many": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_float, vp, C.c_size_t,
                                         C.POINTER(C.c_int64)]),
        "rcf_chan_read_iq": (i64, [vp, C.c_int, fp, sz]),
        "rcf_chan_read_fm": (i64, [vp, C.c_int, C.c_float, fp, sz]),
        "rcf_chan_rings": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz)]),
        "rcf_source_shift": (C.c_int, [vp, C.c_double]),
        "rcf_pfb_open": (C.c_int, [vp, C.c_int, C.c_int, fp, C.c_int]),
        "rcf_pfb_close": (C.c_int, [vp]),
        "rcf_pfb_produced": (i64, [vp]),
        "rcf_pfb_read_bin": (i64, [vp, C.c_int, fp, sz]),
        "rcf_pfb_fm_enable": (C.c_int, [vp, C.c_int, C.c_int]),
        "rcf_pfb_read_fm": (i64, [vp, C.c_int, C.c_float, fp, sz]),
        "rcf_chan_squelch": (C.c_int, [vp, C.c_int, C.POINTER(SquelchParams)]),
        "rcf_chan_squelch_state": (C.c_int, [vp, C.c_int, C.POINTER(SquelchState)]),
        "rcf_pfb_squelch": (C.c_int, [vp, C.POINTER(C.c_double), C.c_int, C.c_double]),
        "rcf_pfb_squelch_read": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_uint32), C.c_int,
                                           C.POINTER(i64)]),
        "rcf_pfb_squelch_segment": (C.c_int, []),
        "rcf_chan_capture": (C.c_int, [vp, C.c_int, C.POINTER(CaptureParams)]),
        "rcf_chan_capture_state": (C.c_int, [vp, C.c_int, C.POINTER(CaptureState)]),
        "rcf_chan_read_capture": (i64, [vp, C.c_int, fp, sz]),
        "rcf_chan_read_capture_rec": (i64, [vp, C.c_int, C.POINTER(C.c_uint32), sz]),
        "rcf_chan_capture_rings": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]),
        "rcf_pfb_fm_ring": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(i64)]),
        "rcf_pfb_fm_lost": (i64, [vp]),
        "rcf_pfb_rings": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]),
        "rcf_pfb_chan_open": (C.c_int, [vp, C.c_int, C.c_int, C.c_double, ip]),
        "rcf_pfb_tap_open": (C.c_int, [vp, C.c_int, C.c_int, ip]),
        "rcf_chan_set_fm_only": (C.c_int, [vp, C.c_int, C.c_int]),
        "rcf_pfb_shape_supported": (C.c_int, [C.c_int, C.c_int, C.c_int]),
        "rcf_pfb_shape_family": (C.c_int, [C.c_int, C.c_int, C.c_int]),
        "rcf_pfb_tap_leakage": (C.c_int, [C.c_double, C.c_int, fp, C.c_int, C.c_int, C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]),
        "rcf_scan_start": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
        "rcf_scan_result": (C.c_int, [vp, fp]),
        "rcf_scan_frames_done": (C.c_int, [vp]),
        "rcf_scan_result_device": (C.c_int, [vp, C.POINTER(vp)]),
        "rcf_find_peaks": (C.c_int, [fp, i64, C.c_double, C.c_double, C.c_double, C.POINTER(i64), i64,
                                     C.POINTER(i64), C.POINTER(C.c_double)]),
        "rcf_peak_frequency": (i64, [i64, C.c_double, i64, C.c_double]),
        "rcf_timing_enable": (C.c_int, [vp, C.c_int]),
        "rcf_timing_stride": (C.c_int, [vp, C.c_int]),
        "rcf_timing_read": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(i64), C.c_int]),
        "rcf_scan_find_peaks": (C.c_int, [vp, C.c_double, C.POINTER(i64), i64, C.POINTER(i64),
                                          C.POINTER(C.c_double), C.POINTER(vp)]),
        "rcf_host_alloc": (vp, [sz]),
        "rcf_host_free": (None, [vp]),
        "rcf_comm_unique_id": (C.c_int, [vp]),
        "rcf_comm_init": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "rcf_comm_destroy": (C.c_int, [vp]),
        "rcf_comm_size": (C.c_int, [vp]),
        "rcf_allgather_peaks": (C.c_int, [vp, C.POINTER(i64), C.c_int, C.POINTER(i64), C.c_int, ip]),
        "rcf_allreduce_max": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "rcf_group_open": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(vp)]),
        "rcf_group_close": (C.c_int, [vp]),
        "rcf_group_size": (C.c_int, [vp]),
        "rcf_group_push": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), C.c_int, C.c_float, C.c_float]),
        "rcf_group_commit": (C.c_int, [vp, C.POINTER(sz)]),
        "rcf_group_read_many": (C.c_int, [vp, C.c_int, ip, ip, C.c_int, C.c_float, vp, sz, C.POINTER(i64)]),
        "rcf_group_sync": (C.c_int, [vp]),
        "rcf_pump_start": (C.c_int, [vp, C.POINTER(PumpConfig), C.POINTER(vp)]),
        "rcf_pump_stats": (C.c_int, [vp, C.POINTER(PumpStats)]),
        "rcf_pump_written": (i64, [vp, C.c_int]),
        "rcf_pump_read": (i64, [vp, C.c_int, C.POINTER(i64), vp, sz]),
        "rcf_pump_read_many": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(i64), C.c_int, vp, sz, C.POINTER(i64)]),
        "rcf_pump_subscribe": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(i64)]),
        "rcf_pump_subscribe_hard": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(i64)]),
        "rcf_pump_unsubscribe": (C.c_int, [vp, C.c_int]),
        "rcf_pump_stop": (C.c_int, [vp]),
    }
    for name, params, state in (("tsbk", TsbkParams, TsbkState), ("edacs", EdacsParams, EdacsState), ("osw", OswParams, OswState),
                                ("p25lc", P25lcParams, P25lcState)):
        sig["rcf_chan_" + name] = (C.c_int, [vp, C.c_int, C.POINTER(params)])     # the frame decoders behind the slicer
        sig["rcf_chan_%s_state" % name] = (C.c_int, [vp, C.c_int, C.POINTER(state)])
        sig["rcf_chan_read_" + name] = (i64, [vp, C.c_int, C.POINTER(C.c_uint32), sz])
        sig["rcf_chan_%s_ring" % name] = (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)])
    sig["rcf_chan_p25lc_opt"] = (C.c_int, [vp, C.c_int, C.POINTER(P25lcParams), C.c_uint32])
    sig["rcf_chan_tsbk_ex"] = (C.c_int, [vp, C.c_int, C.POINTER(TsbkParams), C.c_uint32])
    sig["rcf_chan_p25lc_ex"] = (C.c_int, [vp, C.c_int, C.POINTER(P25lcParams), C.c_uint32, C.c_uint32])
    sig["rcf_chan_nid_state"] = (C.c_int, [vp, C.c_int, C.POINTER(NidState)])
    sig["rcf_chan_tsbk_opt"] = (C.c_int, [vp, C.c_int, C.POINTER(TsbkParams), C.c_uint32, C.c_uint32])
    sig["rcf_chan_trellis_state"] = (C.c_int, [vp, C.c_int, C.POINTER(TrellisState)])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _read_what(what, stages=False):
    """the batched readers' and the pump's `what`: "iq", "agc", anything else the discriminator (as it always was).
    stages=True -- how every reader of this module calls it -- also names the stages' streams: "sym", "clock", "costas",
    "fsk4", "audio", the slicer's "hard" and "sync", the TSBK stage's "tsbk", the EDACS stage's "edacs", the OSW stage's "osw" and the P25 voice stage's "p25lc".  The one-argument form keeps its old answers ("sym" was never a
    stream there: the discriminator)."""
    if stages and what in _STAGE_WHAT:
        return _STAGE_WHAT[what]
    if stages and what in _HARD_WHAT:
        return _HARD_WHAT[what]
    if stages and what in _CAPTURE_WHAT:           # the capture stage's "capture" (cf32) and "capture_rec" (CAPTURE_REC_DTYPE)
        return _CAPTURE_WHAT[what]
    return READ_IQ if what == "iq" else READ_AGC if what == "agc" else READ_FM


def _read_dtype(what):
    """item type of stream `what` as the readers deliver it: cf32 for "iq" and "agc", uint32 for the slicer's "hard" and
    "sync", TSBK_DTYPE for "tsbk", EDACS_DTYPE for "edacs", OSW_DTYPE for "osw", P25LC_DTYPE for "p25lc", float32 for everything else"""
    w = _read_what(what, True)
    if w in _RECORD_DTYPE:
        return _RECORD_DTYPE[w]
    return np.complex64 if w in (READ_IQ, READ_AGC, READ_CAPTURE) else np.uint32 if w in (HARD_BITS, HARD_SYNC) else np.float32


def _check(rc):
    if rc < 0:
        raise RcfError(rc, lib().rcf_last_error().decode("utf-8", "replace"))
    return rc


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def pfb_squelch_segment() -> int:
    """frames per segment of the bank's carrier detector (rcf_pfb_squelch_segment; no device needed)"""
    return lib().rcf_pfb_squelch_segment()


def device_count() -> int:
    return lib().rcf_device_count()


def device_pci_bus_id(device: int):
    """'0000:75:00.0' of HIP device `device` (sysfs: /sys/bus/pci/devices/<that>/numa_node), None if unknown"""
    buf = C.create_string_buffer(32)
    return buf.value.decode() if lib().rcf_device_pci_bus_id(device, buf, 32) == 0 else None


def design_low_pass_2(gain, fs, fc, tw, att_db, window=WIN_HAMMING) -> np.ndarray:
    L = lib()
    n = -L.rcf_design_low_pass_2(gain, fs, fc, tw, att_db, window, None, 0)
    if n <= 0:
        _check(-n if n else RCF_EINVAL)
    taps = np.empty(n, dtype=np.float32)
    _check(L.rcf_design_low_pass_2(gain, fs, fc, tw, att_db, window, _fp(taps), n))
    return taps


def design_firdes(kind, gain, fs, fc, tw, window=WIN_HAMMING, beta=6.76) -> np.ndarray:
    """firdes.low_pass / firdes.high_pass(gain, fs, fc, tw, window, beta)"""
    L = lib()
    n = -L.rcf_design_firdes(kind, gain, fs, fc, tw, window, beta, None, 0)
    if n <= 0:
        _check(-n if n else RCF_EINVAL)
    taps = np.empty(n, dtype=np.float32)
    _check(L.rcf_design_firdes(kind, gain, fs, fc, tw, window, beta, _fp(taps), n))
    return taps


def design_optfir_low_pass(gain, fs, freq1, freq2, passband_ripple_db, stopband_atten_db) -> np.ndarray:
    """gr-filter optfir.low_pass(): remezord + Parks-McClellan"""
    L = lib()
    n = -L.rcf_design_optfir_low_pass(gain, fs, freq1, freq2, passband_ripple_db, stopband_atten_db, None, 0)
    if n <= 0:
        _check(-n if n else RCF_EINVAL)
    taps = np.empty(n, dtype=np.float32)
    _check(L.rcf_design_optfir_low_pass(gain, fs, freq1, freq2, passband_ripple_db, stopband_atten_db, _fp(taps), n))
    return taps


def design_fm_deemph(fs, tau=75e-6):
    b, a = (C.c_double * 2)(), (C.c_double * 2)()
    _check(lib().rcf_design_fm_deemph(fs, tau, b, a))
    return [b[0], b[1]], [a[0], a[1]]


def design_resampler(interpolation, decimation):
    """-> (interp, decim, taps) of rational_resampler_fff(interpolation, decimation) with default taps"""
    L = lib()
    i, d = C.c_int(), C.c_int()
    n = -L.rcf_design_resampler(int(interpolation), int(decimation), C.byref(i), C.byref(d), None, 0)
    if n <= 0:
        _check(-n if n else RCF_EINVAL)
    taps = np.empty(n, dtype=np.float32)
    _check(L.rcf_design_resampler(int(interpolation), int(decimation), C.byref(i), C.byref(d), _fp(taps), n))
    return i.value, d.value, taps


def design_mmse_interpolator(ntaps=8, nsteps=128, bw=0.25) -> np.ndarray:
    """[nsteps + 1, ntaps] MMSE fractional-delay interpolator bank (rcf_design_mmse_interpolator): row s interpolates at
    mu = s / nsteps; the default is the bank rcf_chan_clock_mm uses when the caller passes none"""
    L = lib()
    n = -L.rcf_design_mmse_interpolator(int(ntaps), int(nsteps), float(bw), None, 0)
    if n <= 0:
        _check(-n if n else RCF_EINVAL)
    taps = np.empty(n, dtype=np.float32)
    _check(L.rcf_design_mmse_interpolator(int(ntaps), int(nsteps), float(bw), _fp(taps), n))
    return taps.reshape(int(nsteps) + 1, int(ntaps))


def design_window(window, n) -> np.ndarray:
    w = np.empty(n, dtype=np.float32)
    _check(lib().rcf_design_window(window, n, _fp(w)))
    return w


DECIM_EXACT, DECIM_FLOOR = 0, 1


def channel_params(samp_rate, channel_rate, decim_rule=DECIM_EXACT):
    """(decim, ntaps) of rc_frontend/channel.py:31-33; decim_rule=DECIM_FLOOR: the Python-2 reading int(fs/cr) // 2"""
    d, t = C.c_int(), C.c_int()
    _check(lib().rcf_channel_params_ex(samp_rate, int(channel_rate), int(decim_rule), C.byref(d), C.byref(t), None))
    return d.value, t.value


def pfb_shape_supported(n_bins, decim, ntaps) -> bool:
    return bool(lib().rcf_pfb_shape_supported(int(n_bins), int(decim), int(ntaps)))


def pfb_shape_family(n_bins, decim, ntaps) -> int:
    """kernel family of a bank shape: 0 none, 1 power-of-two bins, 2 400 * 2^k bins, 3 mixed radix (160 .. 1280 bins)"""
    return int(lib().rcf_pfb_shape_family(int(n_bins), int(decim), int(ntaps)))


def pfb_tap_leakage(samp_rate, n_bins, taps, bin):
    """(leak_l2, const_phase) of rcf_pfb_tap_leakage: how far bin `bin` of an exact-phase bank is from GNU Radio's
    float32-phase channel at the same offset."""
    t = np.ascontiguousarray(taps, dtype=np.float32)
    l2, cp = C.c_double(), C.c_double()
    _check(lib().rcf_pfb_tap_leakage(float(samp_rate), int(n_bins), _fp(t), len(t), int(bin), C.byref(l2),
                                     C.byref(cp)))
    return l2.value, cp.value


def find_peaks(spectrum, min_w, max_w, prominence=1.0, cap=4096):
    s = np.ascontiguousarray(spectrum, dtype=np.float32)
    idx = np.empty(cap, dtype=np.int64)
    cnt, mean = C.c_int64(), C.c_double()
    _check(lib().rcf_find_peaks(_fp(s), len(s), min_w, max_w, prominence,
                                idx.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(cnt), C.byref(mean)))
    return idx[:min(cnt.value, cap)].copy(), mean.value, cnt.value


def peak_frequency(line, samp_rate, fft_len, center_freq) -> int:
    return lib().rcf_peak_frequency(int(line), samp_rate, int(fft_len), center_freq)


class PinnedArray:
    """numpy view of page-locked host memory (rcf_host_alloc): the buffer an SDR driver fills and hands to
    Frontend.push / push_raw; freed when the object goes away"""

    def __init__(self, n, dtype):
        self.dtype = np.dtype(dtype)
        self.nbytes = int(n) * self.dtype.itemsize
        self._p = lib().rcf_host_alloc(self.nbytes)
        if not self._p:
            raise RcfError(RCF_ENOMEM, lib().rcf_last_error().decode("utf-8", "replace"))
        self.array = np.frombuffer((C.c_char * self.nbytes).from_address(self._p), dtype=self.dtype)

    def free(self):
        if self._p:
            self.array = None
            lib().rcf_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def comm_unique_id() -> bytes:
    """rank 0: the 128-byte RCCL id every rank passes to Frontend.comm_init"""
    buf = C.create_string_buffer(128)
    _check(lib().rcf_comm_unique_id(C.cast(buf, C.c_void_p)))
    return buf.raw


class Frontend:
    """One SDR source: owner of the HBM wideband buffer, channels, PFB and scanner (rcf_t)."""

    def __init__(self, samp_rate, center_freq=0.0, device=0, block_capacity=0, hist_capacity=0,
                 out_capacity=0):
        self._h = C.c_void_p()
        self.samp_rate = float(samp_rate)
        self.center_freq = float(center_freq)
        # the scan's length sizes scan_result()'s buffer: a scan_start() on another thread must not change it between
        # the allocation and the copy
        self._scan_len = 0
        self._scan_lock = threading.Lock()
        _check(lib().rcf_open_ex(device, samp_rate, center_freq, block_capacity, hist_capacity,
                                 out_capacity, C.byref(self._h)))

    # -- lifecycle
    def close(self):
        if self._h:
            lib().rcf_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_rotator(self, exact=True):
        """exact: iterate GNU Radio's float32 rotator per channel (rcf_set_rotator); before the first channel"""
        _check(lib().rcf_set_rotator(self._h, 1 if exact else 0))

    def set_stage2_lag(self, on=True):
        """stage-2 channels of a power-of-two bank ride in the NEXT block's filterbank launch (rcf_set_stage2_lag; default on)"""
        _check(lib().rcf_set_stage2_lag(self._h, 1 if on else 0))

    def set_decim_rule(self, rule):
        """DECIM_EXACT (default) | DECIM_FLOOR (rcf_set_decim_rule): what rcf_chan_open does with an odd int(fs/cr)"""
        _check(lib().rcf_set_decim_rule(self._h, int(rule)))

    def sync(self):
        _check(lib().rcf_sync(self._h))

    @property
    def stream(self):
        return lib().rcf_stream(self._h)

    @property
    def samples_in(self):
        return lib().rcf_samples_in(self._h)

    # -- multi-GPU (one front-end per GPU; the only exchange is the detected-peak lists)
    def comm_init(self, rank, n_ranks, unique_id=None):
        buf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        _check(lib().rcf_comm_init(self._h, int(rank), int(n_ranks), C.cast(buf, C.c_void_p) if buf is not None else None))

    def comm_destroy(self):
        _check(lib().rcf_comm_destroy(self._h))

    def comm_size(self) -> int:
        """ranks of the handle's RCCL communicator (1 without one)"""
        return int(lib().rcf_comm_size(self._h))

    def allgather_peaks(self, mine, cap=1024):
        """-> list (one int64 array per rank) of every rank's values, via ncclAllGather on the handle's device"""
        mine = np.ascontiguousarray(mine, dtype=np.int64)
        w = lib().rcf_comm_size(self._h)
        out = np.empty(w * cap, dtype=np.int64)
        counts = (C.c_int * w)()
        _check(lib().rcf_allgather_peaks(self._h, mine.ctypes.data_as(C.POINTER(C.c_int64)), len(mine),
                                         out.ctypes.data_as(C.POINTER(C.c_int64)), int(cap), counts))
        return [out[r * cap: r * cap + counts[r]].copy() for r in range(w)]

    def allreduce_max(self, value: float) -> float:
        """barrier + max over ranks (syncs the stream first); identity without a communicator"""
        v = C.c_double(float(value))
        _check(lib().rcf_allreduce_max(self._h, C.byref(v)))
        return v.value

    # -- measurement
    def timing_enable(self, on=True, classes=None):
        """classes: iterable of T_* to time only those (each timed launch costs two event records)"""
        v = 1 if on else 0
        if on and classes is not None:
            v = 0
            for c in classes:
                v |= 1 << (int(c) + 1)
        _check(lib().rcf_timing_enable(self._h, v))

    def timing_stride(self, every=1):
        """time only every `every`-th launch of each timed class (an event pair costs ~12 us of queue gap)"""
        _check(lib().rcf_timing_stride(self._h, int(every)))

    def timing_read(self, what, reset=True):
        ms, n = C.c_double(), C.c_int64()
        _check(lib().rcf_timing_read(self._h, int(what), C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    # -- ingest
    def push(self, iq: np.ndarray):
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        _check(lib().rcf_push_iq(self._h, _fp(iq.view(np.float32)), len(iq)))

    def ingest_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().rcf_ingest_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def push_raw(self, raw: np.ndarray, fmt, scale, offset=0.0):
        """raw: interleaved I,Q in the SDR's wire type (uint8 / int8 / int16), 2 values per sample."""
        dt = {FMT_U8: np.uint8, FMT_S8: np.int8, FMT_S16: np.int16}[fmt]
        raw = np.ascontiguousarray(raw, dtype=dt)
        _check(lib().rcf_push_raw(self._h, raw.ctypes.data_as(C.c_void_p), raw.size // 2, int(fmt),
                                  float(scale), float(offset)))

    def ingest_write(self, iq: np.ndarray, at=0):
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        _check(lib().rcf_ingest_write(self._h, _fp(iq.view(np.float32)), len(iq), int(at)))

    def commit(self, n):
        _check(lib().rcf_commit(self._h, int(n)))

    # -- channels
    def chan_open(self, channel_rate, offset_hz) -> int:
        cid = C.c_int()
        _check(lib().rcf_chan_open(self._h, int(channel_rate), float(offset_hz), C.byref(cid)))
        return cid.value

    def chan_open_taps(self, src, decim, taps, offset_hz) -> int:
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        cid = C.c_int()
        _check(lib().rcf_chan_open_taps(self._h, int(src), int(decim), _fp(taps), len(taps),
                                        float(offset_hz), C.byref(cid)))
        return cid.value

    def pfb_chan_open(self, bin_, channel_rate, delta_hz) -> int:
        cid = C.c_int()
        _check(lib().rcf_pfb_chan_open(self._h, int(bin_), int(channel_rate), float(delta_hz), C.byref(cid)))
        return cid.value

    def pfb_tap_open(self, bin_, gr_phase=True) -> int:
        """bin `bin_` of the open filterbank as a channel id (rcf_pfb_tap_open)"""
        cid = C.c_int()
        _check(lib().rcf_pfb_tap_open(self._h, int(bin_), 1 if gr_phase else 0, C.byref(cid)))
        return cid.value

    def chan_set_fm_only(self, cid, on=True):
        """a filterbank tap that is only demodulated: its discriminator ring alone is written (rcf_chan_set_fm_only)"""
        _check(lib().rcf_chan_set_fm_only(self._h, cid, 1 if on else 0))

    def chan_set_offset(self, cid, offset_hz):
        _check(lib().rcf_chan_set_offset(self._h, cid, float(offset_hz)))

    def chan_close(self, cid):
        _check(lib().rcf_chan_close(self._h, cid))

    def chan_info(self, cid):
        d, t, r, o = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        _check(lib().rcf_chan_info(self._h, cid, C.byref(d), C.byref(t), C.byref(r), C.byref(o)))
        return dict(decim=d.value, ntaps=t.value, out_rate=r.value, offset_hz=o.value)

    def chan_start(self, cid):
        """first source-stream sample the channel sees (zero history before it)"""
        return _check(lib().rcf_chan_start(self._h, cid))

    def chan_produced(self, cid):
        return _check(lib().rcf_chan_produced(self._h, cid))

    def _read_ring(self, fn, cid, n, dtype):
        """the unread items of one of channel cid's rings through its single reader fn(h, cid, out, max): at most n"""
        out = np.empty(n, dtype=dtype)
        n = _check(fn(self._h, cid, _fp(out.view(np.float32)), n))
        return out[:n].copy()

    def _ring_of(self, fn, cid):
        """(device pointer, capacity) of one of channel cid's rings through fn(h, cid, &pointer, &capacity)"""
        p, cap = C.c_void_p(), C.c_size_t()
        _check(fn(self._h, cid, C.byref(p), C.byref(cap)))
        return p.value, cap.value

    def _attach(self, fn, cid, params, on=True, **fields):
        """a stage of channel cid through fn(h, cid, &params): a params() with the integer `fields` set; on=False: off (NULL)"""
        if not on:
            _check(fn(self._h, cid, None))
            return
        p = params()
        for k, v in fields.items():
            setattr(p, k, int(v))
        _check(fn(self._h, cid, C.byref(p)))

    def _state_of(self, fn, cid, state) -> dict:
        """a stage's state through fn(h, cid, &state) as a dict of the struct's fields"""
        st = state()
        _check(fn(self._h, cid, C.byref(st)))
        return _state_dict(st)

    def _read_records(self, fn, cid, n, dtype):
        """the unread items of one of channel cid's uint32 rings through its single reader fn(h, cid, out, max): at most n
        items of dtype (whole words)"""
        out = np.empty(n, dtype=dtype)
        n = _check(fn(self._h, cid, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out[:n].copy()

    def chan_read_iq(self, cid, max_samples=1 << 20) -> np.ndarray:
        return self._read_ring(lib().rcf_chan_read_iq, cid, max_samples, np.complex64)

    def chan_read_fm(self, cid, gain, max_samples=1 << 20) -> np.ndarray:
        out = np.empty(max_samples, dtype=np.float32)
        n = _check(lib().rcf_chan_read_fm(self._h, cid, float(gain), _fp(out), max_samples))
        return out[:n].copy()

    def chan_read_many(self, cids, what="iq", gain=1.0, cap_each=1 << 14, out=None):
        """new samples of many channels behind ONE device synchronisation (rcf_chan_read_many) -> list of arrays
        (views into `out`, a [len(cids), cap_each] complex64 / float32 array -- pass a PinnedArray's for overlapping
        copies), None where the channel no longer exists (or lacks the stream).  what: "iq", "fm" (x gain), "agc", or a
        stage's stream -- "sym", "clock", "costas", "fsk4", "audio": float32, from where that stage's single reader stands --
        or the slicer's "hard" (packed words) / "sync" (hit items, see widen_hits): uint32 -- or the TSBK stage's "tsbk":
        TSBK_DTYPE records -- or the EDACS stage's "edacs": EDACS_DTYPE records -- or the OSW stage's "osw": OSW_DTYPE records -- or the P25 voice stage's "p25lc": P25LC_DTYPE records"""
        n = len(cids)
        dt = _read_dtype(what)
        if out is None:
            out = np.empty((max(n, 1), cap_each), dtype=dt)
        out = out.reshape(-1, cap_each)
        ids = (C.c_int * max(n, 1))(*[int(c) for c in cids])
        counts = (C.c_int64 * max(n, 1))()
        _check(lib().rcf_chan_read_many(self._h, _read_what(what, True), ids, n, float(gain),
                                        out.ctypes.data_as(C.c_void_p), int(cap_each), counts))
        return [None if counts[i] < 0 else out[i, :counts[i]] for i in range(n)]

    def chan_read_many_plan(self, cids, what="iq", gain=1.0, cap_each=1 << 14, out=None):
        """chan_read_many for a FIXED channel list called over and over (an egress pump, a real-time loop): the ctypes
        arguments are built once; the returned callable performs one rcf_chan_read_many and returns (counts, out) --
        counts an int64 array (negative: that channel is gone), out the [len(cids), cap_each] array the samples are in.
        Costs ~10 us of interpreter time per call instead of ~1 us per channel."""
        n = len(cids)
        dt = _read_dtype(what)
        if out is None:
            out = np.empty((max(n, 1), cap_each), dtype=dt)
        out2 = out.reshape(-1, cap_each)
        ids = (C.c_int * max(n, 1))(*[int(c) for c in cids])
        counts = np.zeros(max(n, 1), dtype=np.int64)
        f = lib().rcf_chan_read_many
        args = (self._h, _read_what(what, True), ids, n, C.c_float(float(gain)), out2.ctypes.data_as(C.c_void_p),
                C.c_size_t(int(cap_each)), counts.ctypes.data_as(C.POINTER(C.c_int64)))

        def call():
            _check(f(*args))
            return counts, out2
        call.keep = (ids, counts, out2)                     # the buffers the C call writes into live as long as the plan
        return call

    def chan_fm_filter(self, cid, gain, taps):
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        _check(lib().rcf_chan_fm_filter(self._h, cid, float(gain), _fp(taps), len(taps)))

    def chan_read_sym(self, cid, max_samples=1 << 20) -> np.ndarray:
        return self._read_ring(lib().rcf_chan_read_sym, cid, max_samples, np.float32)

    def chan_agc(self, cid, nsamples=1024, reference=1.0):
        """analog.feedforward_agc_cc(nsamples, reference) on the channel's IQ (rcf_chan_agc; p25_control_demod.py:149),
        starting with zero history at the channel's next output; nsamples=0 switches it off"""
        _check(lib().rcf_chan_agc(self._h, cid, int(nsamples), float(reference)))

    def chan_read_agc(self, cid, max_samples=1 << 20) -> np.ndarray:
        return self._read_ring(lib().rcf_chan_read_agc, cid, max_samples, np.complex64)

    def chan_agc_ring(self, cid):
        """(device pointer, capacity) of the channel's cf32 AGC ring (rcf_chan_agc_ring)"""
        return self._ring_of(lib().rcf_chan_agc_ring, cid)

    def chan_clock_mm(self, cid, omega, gain_omega=1.4395919, mu=0.5, gain_mu=0.05, omega_relative_limit=0.005, gain=5.0,
                      interp_taps=None):
        """digital.clock_recovery_mm_ff(omega, gain_omega, mu, gain_mu, omega_relative_limit) on quadrature_demod_cf(gain)
        of the channel (rcf_chan_clock_mm; moto_control_demod.py:113, edacs_control_demod.py:85), starting with zero
        history at the channel's next output; omega=None switches it off.  interp_taps: a [129, 8] interpolator bank
        (GNU Radio's, for a caller who has it); None = design_mmse_interpolator()"""
        if omega is None:
            _check(lib().rcf_chan_clock_mm(self._h, cid, None))
            return
        p = ClockMmParams()
        p.gain, p.omega, p.gain_omega, p.mu = float(gain), float(omega), float(gain_omega), float(mu)
        p.gain_mu, p.omega_relative_limit = float(gain_mu), float(omega_relative_limit)
        taps = _bank_arg(interp_taps)
        if taps is not None:
            p.interp_taps = _fp(taps)
        _check(lib().rcf_chan_clock_mm(self._h, cid, C.byref(p)))

    def chan_clock_produced(self, cid):
        """(soft symbols produced since the clock was enabled, times its guards fired) (rcf_chan_clock_produced)"""
        n, s = C.c_int64(), C.c_int64()
        _check(lib().rcf_chan_clock_produced(self._h, cid, C.byref(n), C.byref(s)))
        return n.value, s.value

    def chan_read_clock(self, cid, max_symbols=1 << 20) -> np.ndarray:
        """unread soft symbols of the channel's clock, oldest first; the bits are (out >= 0)"""
        return self._read_ring(lib().rcf_chan_read_clock, cid, max_symbols, np.float32)

    def chan_clock_ring(self, cid):
        """(device pointer, capacity) of the channel's float32 soft-symbol ring (rcf_chan_clock_ring)"""
        return self._ring_of(lib().rcf_chan_clock_ring, cid)

    def chan_costas(self, cid, omega, gain_mu=0.025, gain_omega=6.25e-5, alpha=0.04, beta=2e-4, max_freq=0.0, omega_limit=0.005,
                    interp_taps=None):
        """op25's repeater.gardner_costas_cc(omega, gain_mu, gain_omega, alpha, beta, max_freq, -max_freq) -> diff_phasor_cc
        -> complex_to_arg -> multiply_const_ff(4 / pi) on the channel's AGC ring (rcf_chan_costas, which defines the
        stage: unpinned against op25; p25_control_demod.py:150-183), starting with zero history at the channel's next
        output; omega=None switches it off.  The channel must carry an AGC (chan_agc).  interp_taps: a [129, 8]
        interpolator bank; None = design_mmse_interpolator()"""
        if omega is None:
            _check(lib().rcf_chan_costas(self._h, cid, None))
            return
        p, _keep = costas_params_struct(omega, gain_mu, gain_omega, alpha, beta, max_freq, omega_limit, interp_taps)
        _check(lib().rcf_chan_costas(self._h, cid, C.byref(p)))

    def chan_costas_state(self, cid) -> dict:
        """the loop's state as of the last block: n_symbols, n_slips, mu, omega, freq (radians per channel sample, of the
        sign opposite to the carrier's offset), phase (rcf_chan_costas_state; syncs the stream)"""
        return self._state_of(lib().rcf_chan_costas_state, cid, CostasState)

    def chan_read_costas(self, cid, max_symbols=1 << 20) -> np.ndarray:
        """unread soft symbols of the channel's Gardner / Costas stage (+-1, +-3 on a locked signal), oldest first"""
        return self._read_ring(lib().rcf_chan_read_costas, cid, max_symbols, np.float32)

    def chan_costas_ring(self, cid):
        """(device pointer, capacity) of the stage's float32 soft-symbol ring (rcf_chan_costas_ring)"""
        return self._ring_of(lib().rcf_chan_costas_ring, cid)

    def chan_fsk4(self, cid, sample_rate, symbol_rate=4800.0, k_spread=0.01, k_timing=0.025, k_fine=0.125, k_coarse=0.00125,
                  spread_min=1.6, spread_max=2.4, interp_taps=None):
        """op25's fsk4_demod_ff(queue, sample_rate, symbol_rate) on the channel's symbol-filter ring (rcf_chan_fsk4, which
        defines the stage: unpinned against op25; p25_control_demod.py:118-135), starting with zero history at the
        channel's next output; sample_rate=None switches it off.  The channel must carry a symbol filter
        (chan_fm_filter).  interp_taps: a [129, 8] interpolator bank; None = design_mmse_interpolator()"""
        if sample_rate is None:
            _check(lib().rcf_chan_fsk4(self._h, cid, None))
            return
        p, _keep = fsk4_params_struct(sample_rate, symbol_rate, k_spread, k_timing, k_fine, k_coarse, spread_min, spread_max,
                                      interp_taps)
        _check(lib().rcf_chan_fsk4(self._h, cid, C.byref(p)))

    def chan_fsk4_state(self, cid) -> dict:
        """the loop's state as of the last block: n_symbols, n_slips, clock, spread, fine, coarse (the slow average of the
        level offset, of the carrier offset's sign: what op25 posts to its autotune queue) (rcf_chan_fsk4_state; syncs
        the stream)"""
        return self._state_of(lib().rcf_chan_fsk4_state, cid, Fsk4State)

    def chan_read_fsk4(self, cid, max_symbols=1 << 20) -> np.ndarray:
        """unread soft symbols of the channel's C4FM loop (+-1, +-3 on a locked signal), oldest first"""
        return self._read_ring(lib().rcf_chan_read_fsk4, cid, max_symbols, np.float32)

    def chan_squelch(self, cid, threshold_db, alpha=0.1):
        """analog.simple_squelch_cc(threshold_db, alpha) as a carrier detector on the channel's IQ stream (rcf_chan_squelch,
        which defines the stage; scanning_receiver.py:53): it reports and gates nothing.  Level 0 from the channel's next
        output on, again on every call; threshold_db=None detaches it"""
        if threshold_db is None:
            _check(lib().rcf_chan_squelch(self._h, cid, None))
            return
        p = SquelchParams(float(threshold_db), float(alpha))
        _check(lib().rcf_chan_squelch(self._h, cid, C.byref(p)))

    def chan_squelch_state(self, cid) -> dict:
        """the detector's state as of the last block: level, n_seen, n_open, first_open, last_open (channel-sample indices,
        -1: none), unmuted (rcf_chan_squelch_state; syncs the stream)"""
        st = self._state_of(lib().rcf_chan_squelch_state, cid, SquelchState)
        st.pop("reserved_", None)
        return st

    def chan_capture(self, cid, threshold_db, alpha=0.1, pre=0, hang=0, capacity=0, rec_capacity=0):
        """the carrier detector as a gate on the channel's IQ stream (rcf_chan_capture, which defines the stage): the
        samples of the channel's transmissions only, `pre` samples of lead-in and `hang` samples of hang time included, and
        an OPEN and a CLOSE record per transmission.  Every call starts both streams again at item 0, from the channel's
        next output on; threshold_db=None detaches the stage"""
        if threshold_db is None:
            _check(lib().rcf_chan_capture(self._h, cid, None))
            return
        p = CaptureParams(float(threshold_db), float(alpha), int(pre), int(hang), int(capacity), int(rec_capacity))
        _check(lib().rcf_chan_capture(self._h, cid, C.byref(p)))

    def chan_capture_state(self, cid) -> dict:
        """the stage's state as of the last block: level, n_seen, n_decided, n_kept, n_records, n_windows, last_open (-1:
        none), in_window, unmuted (rcf_chan_capture_state; syncs the stream)"""
        return self._state_of(lib().rcf_chan_capture_state, cid, CaptureState)

    def chan_read_capture(self, cid, max_samples=1 << 20) -> np.ndarray:
        """unread samples of the captured stream, oldest first (complex64)"""
        return self._read_ring(lib().rcf_chan_read_capture, cid, max_samples, np.complex64)

    def chan_read_capture_rec(self, cid, max_records=1 << 12) -> np.ndarray:
        """unread records of the capture stage, oldest first: a structured array of CAPTURE_REC_DTYPE"""
        return self._read_records(lib().rcf_chan_read_capture_rec, cid, max_records, CAPTURE_REC_DTYPE)

    def chan_capture_rings(self, cid):
        """(captured ring's device pointer, its capacity in samples, record ring's device pointer, its capacity in records)
        (rcf_chan_capture_rings)"""
        p, cap, r, rcap = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        _check(lib().rcf_chan_capture_rings(self._h, cid, C.byref(p), C.byref(cap), C.byref(r), C.byref(rcap)))
        return p.value, cap.value, r.value, rcap.value

    def chan_slicer(self, cid, source, mode=None, levels=(-2.0, 0.0, 2.0, 4.0), sync_word=0, sync_bits=0, sync_max_errors=0,
                    hit_capacity=0, sync_both=0):
        """hard decisions behind one of the channel's symbol loops (rcf_chan_slicer): source READ_CLOCK / READ_COSTAS /
        READ_FSK4, mode SLICE_BINARY (binary_slicer_fb) or SLICE_FSK4 (op25 fsk4_slicer_fb(levels)); packed MSB first as
        unpacked_to_packed_bb does, with a search for the low sync_bits bits of sync_word (hits: Hamming distance <=
        sync_max_errors; with sync_both=1 also those within sync_max_errors of the inverted word, which carry dist >
        sync_bits / 2).  It starts at the loop's next symbol; source=None switches it off."""
        if source is None:
            _check(lib().rcf_chan_slicer(self._h, cid, None))
            return
        p = SlicerParams()
        p.source, p.mode = int(source), int(mode)
        p.levels = (C.c_float * 4)(*[float(v) for v in levels])
        p.sync_word, p.sync_bits, p.sync_max_errors = int(sync_word), int(sync_bits), int(sync_max_errors)
        p.hit_capacity, p.sync_both = int(hit_capacity), int(sync_both)
        _check(lib().rcf_chan_slicer(self._h, cid, C.byref(p)))

    def chan_slicer_state(self, cid) -> dict:
        """n_symbols, n_words, n_hits of the slicer as of the last block (rcf_chan_slicer_state; syncs the stream)"""
        return self._state_of(lib().rcf_chan_slicer_state, cid, SlicerState)

    def chan_read_hard(self, cid, max_words=1 << 18) -> np.ndarray:
        """unread packed decisions as bytes, 4 per word: GNU Radio's unpacked_to_packed_bb(bps, MSB_FIRST) stream"""
        out = np.empty(max_words, dtype=np.uint32)
        n = _check(lib().rcf_chan_read_hard(self._h, cid, out.ctypes.data_as(C.POINTER(C.c_uint32)), max_words))
        return out[:n].copy().view(np.uint8)

    def chan_read_sync(self, cid, max_hits=1 << 16):
        """unread sync hits -> (k as int64: the last symbol of the window, counted from the stage's start and widened
        against the stage's symbol count; dist as uint8)"""
        out = np.empty(max_hits, dtype=np.uint32)
        n = _check(lib().rcf_chan_read_sync(self._h, cid, out.ctypes.data_as(C.POINTER(C.c_uint32)), max_hits))
        return widen_hits(out[:n], self.chan_slicer_state(cid)["n_symbols"])

    def chan_slicer_rings(self, cid):
        """(word ring device pointer, its capacity, hit ring device pointer, its capacity) (rcf_chan_slicer_rings)"""
        wp, wc, hp, hc = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        _check(lib().rcf_chan_slicer_rings(self._h, cid, C.byref(wp), C.byref(wc), C.byref(hp), C.byref(hc)))
        return wp.value, wc.value, hp.value, hc.value

    def chan_tsbk(self, cid, capacity=0, on=True, nid=False, viterbi=False):
        """P25 trunking blocks behind the channel's slicer (rcf_chan_tsbk_opt): frames from the sync hits, status symbols
        stripped, NID read, every block deinterleaved, trellis-decoded and CRC-checked on the GPU; records of TSBK_DTYPE
        in a ring of `capacity` (0: 256).  nid=True (RCF_NID_BCH): the NID's BCH(63,16,23) word is decoded first and the
        decoded DUID decides whether blocks are decoded (nid_fields: nid_fix, nid_decoded; chan_nid_state).  viterbi=True
        (RCF_TRELLIS_VITERBI): a block's trellis is decoded as a whole, by the least-cost path that ends in state 0, instead of
        the reference's word-by-word walk (trellis_fields: cost, viterbi; chan_trellis_state).  It considers the hits from now
        on; on=False switches it off."""
        self._attach(lambda h, c, p: lib().rcf_chan_tsbk_opt(h, c, p, int(nid), int(viterbi)), cid, TsbkParams, on, capacity=capacity)

    def chan_trellis_state(self, cid) -> dict:
        """n_decoded, n_clean, n_bits, n_words of the trellis decoder of the channel's TSBK stage as of the last block
        (rcf_chan_trellis_state; syncs the stream): all 0 for a stage attached without viterbi"""
        return self._state_of(lib().rcf_chan_trellis_state, cid, TrellisState)

    def chan_nid_state(self, cid) -> dict:
        """n_decoded, n_fixed, n_bits, n_bad of the NID decoder of the channel's TSBK or P25 voice stage as of the last block
        (rcf_chan_nid_state; syncs the stream): all 0 for a stage attached without nid"""
        return self._state_of(lib().rcf_chan_nid_state, cid, NidState)

    def chan_tsbk_state(self, cid) -> dict:
        """n_records, n_frames, n_blocks, n_crc_bad, n_lost of the TSBK stage as of the last block (rcf_chan_tsbk_state;
        syncs the stream)"""
        return self._state_of(lib().rcf_chan_tsbk_state, cid, TsbkState)

    def chan_read_tsbk(self, cid, max_records=1 << 12) -> np.ndarray:
        """unread records of the TSBK stage, oldest first: a structured array of TSBK_DTYPE (tsbk_fields takes `flags` apart)"""
        return self._read_records(lib().rcf_chan_read_tsbk, cid, max_records, TSBK_DTYPE)

    def chan_tsbk_ring(self, cid):
        """(device pointer, capacity in records) of the stage's record ring (rcf_chan_tsbk_ring)"""
        return self._ring_of(lib().rcf_chan_tsbk_ring, cid)

    def chan_edacs(self, cid, capacity=0, esk=False, on=True):
        """EDACS control frames behind the channel's binary slicer (rcf_chan_edacs): frames from the sync hits of either
        polarity, six copies per frame BCH-decoded and two messages elected on the GPU; records of EDACS_DTYPE in a ring of
        `capacity` (0: 256); esk: extended addressing.  It considers the hits from now on; on=False switches it off."""
        self._attach(lib().rcf_chan_edacs, cid, EdacsParams, on, capacity=capacity, esk=bool(esk))

    def chan_edacs_state(self, cid) -> dict:
        """n_records, n_frames, n_msgs, n_msgs_none, n_lost of the EDACS stage as of the last block (rcf_chan_edacs_state;
        syncs the stream)"""
        return self._state_of(lib().rcf_chan_edacs_state, cid, EdacsState)

    def chan_read_edacs(self, cid, max_records=1 << 12) -> np.ndarray:
        """unread records of the EDACS stage, oldest first: a structured array of EDACS_DTYPE (edacs_fields takes `flags`
        apart, rcf.control.edacs_messages gives the reference's strings)"""
        return self._read_records(lib().rcf_chan_read_edacs, cid, max_records, EDACS_DTYPE)

    def chan_edacs_ring(self, cid):
        """(device pointer, capacity in records) of the stage's record ring (rcf_chan_edacs_ring)"""
        return self._ring_of(lib().rcf_chan_edacs_ring, cid)

    def chan_osw(self, cid, capacity=0, on=True):
        """SmartNet OSWs behind the channel's binary slicer (rcf_chan_osw): the 84-bit framing with its lock counter,
        deinterleave, parity syndrome and correction on the GPU; records of OSW_DTYPE in a ring of `capacity` (0: 256).  It
        starts at the slicer's next symbol with locked = 0; on=False switches it off."""
        self._attach(lib().rcf_chan_osw, cid, OswParams, on, capacity=capacity)

    def chan_osw_state(self, cid) -> dict:
        """n_records, n_frames (the reference's packets), n_bad (packets_bad), n_rejects, n_lost, locked, is_locked of the OSW
        stage as of the last block (rcf_chan_osw_state; syncs the stream)"""
        return self._state_of(lib().rcf_chan_osw_state, cid, OswState)

    def chan_read_osw(self, cid, max_records=1 << 12) -> np.ndarray:
        """unread records of the OSW stage, oldest first: a structured array of OSW_DTYPE (osw_fields takes `flags` apart,
        rcf.control.smartnet_osws gives the fields the reference publishes)"""
        return self._read_records(lib().rcf_chan_read_osw, cid, max_records, OSW_DTYPE)

    def chan_osw_ring(self, cid):
        """(device pointer, capacity in records) of the stage's record ring (rcf_chan_osw_ring)"""
        return self._ring_of(lib().rcf_chan_osw_ring, cid)

    def chan_p25lc(self, cid, capacity=0, correct=True, on=True, es=False, erasures=False):
        """P25 voice data units behind the channel's slicer (rcf_chan_p25lc_opt): frames from the sync hits, status symbols
        stripped, NID read, and for an HDU, an LDU1 or a TLC the inner Golay / Hamming words and the outer Reed-Solomon
        word decoded on the GPU (correct=False: p25_general's uncorrected reading); records of P25LC_DTYPE in a ring of
        `capacity` (0: 256).  es=True decodes LDU2's encryption sync as well (kind 4); erasures=True (needs correct) hands
        the inner words given up to the Reed-Solomon decoder as erasures.  It considers the hits from now on and excludes
        the TSBK stage; on=False switches it off.  chan_p25lc_ex is this with the NID option."""
        self.chan_p25lc_ex(cid, capacity, correct, on, es, erasures)

    def chan_p25lc_ex(self, cid, capacity=0, correct=True, on=True, es=False, erasures=False, nid=False):
        """chan_p25lc with rcf_chan_p25lc_ex's last argument: nid=True (RCF_NID_BCH) decodes the NID's BCH(63,16,23) word
        first, and the decoded DUID names the unit (nid_fields takes nid_fix and nid_decoded out of the records;
        chan_nid_state has the counters)"""
        options = (P25LC_ES if es else 0) | (P25LC_ERASURES if erasures else 0)
        self._attach(lambda h, c, p: lib().rcf_chan_p25lc_ex(h, c, p, options, int(nid)), cid, P25lcParams, on, capacity=capacity, correct=int(correct))

    def chan_p25lc_state(self, cid) -> dict:
        """n_records, n_frames, n_decoded, n_rs_bad, n_lost of the P25 voice stage as of the last block
        (rcf_chan_p25lc_state; syncs the stream)"""
        return self._state_of(lib().rcf_chan_p25lc_state, cid, P25lcState)

    def chan_read_p25lc(self, cid, max_records=1 << 12) -> np.ndarray:
        """unread records of the P25 voice stage, oldest first: a structured array of P25LC_DTYPE (p25lc_fields takes
        `flags` and `tail` apart, rcf.p25.voice_units gives the fields the reference publishes)"""
        return self._read_records(lib().rcf_chan_read_p25lc, cid, max_records, P25LC_DTYPE)

    def chan_p25lc_ring(self, cid):
        """(device pointer, capacity in records) of the stage's record ring (rcf_chan_p25lc_ring)"""
        return self._ring_of(lib().rcf_chan_p25lc_ring, cid)

    def chan_fsk4_ring(self, cid):
        """(device pointer, capacity) of the stage's float32 soft-symbol ring (rcf_chan_fsk4_ring)"""
        return self._ring_of(lib().rcf_chan_fsk4_ring, cid)

    def chan_fm_level(self, cid, gain, window=10000) -> float:
        v = C.c_float()
        _check(lib().rcf_chan_fm_level(self._h, cid, float(gain), int(window), C.byref(v)))
        return v.value

    def chan_audio_open(self, cid, squelch_db, squelch_alpha, quad_gain, deemph_b, deemph_a, lpf_taps, hpf_taps,
                        interpolation, decimation, rs_taps):
        """analog voice chain behind a channel (rcf_chan_audio_open); rcf.audio.analog_chain_params builds the
        arguments the way the reference's GNU Radio calls do"""
        lpf = np.ascontiguousarray(lpf_taps, dtype=np.float32)
        hpf = np.ascontiguousarray(hpf_taps, dtype=np.float32)
        rs = np.ascontiguousarray(rs_taps, dtype=np.float32)
        p = AudioParams()
        p.squelch_db, p.squelch_alpha, p.quad_gain = float(squelch_db), float(squelch_alpha), float(quad_gain)
        p.deemph_b[0], p.deemph_b[1] = float(deemph_b[0]), float(deemph_b[1])
        p.deemph_a[0], p.deemph_a[1] = float(deemph_a[0]), float(deemph_a[1])
        p.lpf_taps, p.n_lpf = _fp(lpf), len(lpf)
        p.hpf_taps, p.n_hpf = _fp(hpf), len(hpf)
        p.rs_taps, p.n_rs = _fp(rs), len(rs)
        p.interpolation, p.decimation = int(interpolation), int(decimation)
        _check(lib().rcf_chan_audio_open(self._h, cid, C.byref(p)))

    def chan_audio_close(self, cid):
        _check(lib().rcf_chan_audio_close(self._h, cid))

    def chan_audio_produced(self, cid):
        a, u = C.c_int64(), C.c_int64()
        _check(lib().rcf_chan_audio_produced(self._h, cid, C.byref(a), C.byref(u)))
        return a.value, u.value

    def chan_read_audio(self, cid, max_samples=1 << 20) -> np.ndarray:
        return self._read_ring(lib().rcf_chan_read_audio, cid, max_samples, np.float32)

    def source_shift(self, delta_hz):
        _check(lib().rcf_source_shift(self._h, float(delta_hz)))

    # -- PFB
    def pfb_open(self, n_bins, decim, taps):
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        _check(lib().rcf_pfb_open(self._h, int(n_bins), int(decim), _fp(taps), len(taps)))

    def pfb_close(self):
        _check(lib().rcf_pfb_close(self._h))

    def pfb_produced(self):
        return _check(lib().rcf_pfb_produced(self._h))

    def pfb_read_bin(self, bin_, max_samples=1 << 20) -> np.ndarray:
        out = np.empty(max_samples, dtype=np.complex64)
        n = _check(lib().rcf_pfb_read_bin(self._h, int(bin_), _fp(out.view(np.float32)), max_samples))
        return out[:n].copy()

    def pfb_fm_enable(self, mode=1, gr_phase=True):
        """the discriminator of EVERY bin in the bank's own kernel (rcf_pfb_fm_enable): mode 1 beside the bins ring, 2
        instead of it, 0 off"""
        _check(lib().rcf_pfb_fm_enable(self._h, int(mode), 1 if gr_phase else 0))

    def pfb_squelch(self, threshold_db, alpha=0.1):
        """the carrier detector on EVERY bin of the open bank (rcf_pfb_squelch): one threshold in dB for all bins or one per
        bin; None switches it off.  Takes effect with the next block; every call resets every bin"""
        if threshold_db is None:
            _check(lib().rcf_pfb_squelch(self._h, None, 0, float(alpha)))
            return
        thr = np.ascontiguousarray(np.atleast_1d(threshold_db), dtype=np.float64)
        _check(lib().rcf_pfb_squelch(self._h, thr.ctypes.data_as(C.POINTER(C.c_double)), len(thr), float(alpha)))

    def pfb_squelch_read(self, n_bins) -> dict:
        """per bin of the bank's carrier detector: level (float64), n_open and last_open (int64; frame index since pfb_open,
        -1: none), unmuted (bool, the mask unpacked), and frames_seen (rcf_pfb_squelch_read; syncs the stream)"""
        n_bins = int(n_bins)
        level = np.empty(n_bins, np.float64)
        n_open, last_open = np.empty(n_bins, np.int64), np.empty(n_bins, np.int64)
        mask = np.zeros((n_bins + 31) // 32, np.uint32)
        seen = C.c_int64()
        p64 = C.POINTER(C.c_int64)
        _check(lib().rcf_pfb_squelch_read(self._h, level.ctypes.data_as(C.POINTER(C.c_double)), n_open.ctypes.data_as(p64),
                                          last_open.ctypes.data_as(p64), mask.ctypes.data_as(C.POINTER(C.c_uint32)), n_bins,
                                          C.byref(seen)))
        unmuted = (mask[np.arange(n_bins) // 32] >> (np.arange(n_bins) % 32).astype(np.uint32)) & 1
        return dict(level=level, n_open=n_open, last_open=last_open, unmuted=unmuted.astype(bool), mask=mask,
                    frames_seen=seen.value)

    def pfb_fm_lost(self):
        return _check(lib().rcf_pfb_fm_lost(self._h))

    def pfb_read_fm(self, bin_, gain=1.0, max_samples=1 << 20) -> np.ndarray:
        out = np.empty(max_samples, dtype=np.float32)
        n = _check(lib().rcf_pfb_read_fm(self._h, int(bin_), float(gain), _fp(out), max_samples))
        return out[:n].copy()

    # -- scan
    def scan_start(self, fft_len, n_frames=1000, avg_len=100):
        with self._scan_lock:
            _check(lib().rcf_scan_start(self._h, int(fft_len), int(n_frames), int(avg_len)))
            self._scan_len = int(fft_len)            # (only once librcf has accepted the scan)

    def scan_frames_done(self):
        return _check(lib().rcf_scan_frames_done(self._h))

    def scan_result(self):
        with self._scan_lock:
            if not self._scan_len:
                return None                          # no scan was ever started
            out = np.empty(self._scan_len, dtype=np.float32)
            rc = lib().rcf_scan_result(self._h, _fp(out))
        if rc == RCF_EAGAIN:
            return None
        _check(rc)
        return out

    def scan_find_peaks(self, prominence=1.0, cap=1024, want_device=False):
        idx = np.empty(cap, dtype=np.int64)
        cnt, mean, dev = C.c_int64(), C.c_double(), C.c_void_p()
        _check(lib().rcf_scan_find_peaks(self._h, prominence, idx.ctypes.data_as(C.POINTER(C.c_int64)), cap,
                                         C.byref(cnt), C.byref(mean), C.byref(dev) if want_device else None))
        return idx[:min(cnt.value, cap)].copy(), mean.value, dev.value


_WIRE_DTYPE = {FMT_CF32: np.complex64, FMT_U8: np.uint8, FMT_S8: np.int8, FMT_S16: np.int16}


class Group:
    """G front-ends of one device whose blocks go out as ONE launch per stage (rcf_group_t): the reference's receiver with
    all its sources in one top block (rc_frontend/receiver.py:67-70,170-204).  The members stay usable one by one (channel
    control, reads); close the group before closing them."""

    def __init__(self, frontends):
        self.frontends = list(frontends)
        self._g = C.c_void_p()
        arr = (C.c_void_p * len(self.frontends))(*[fe._h for fe in self.frontends])
        _check(lib().rcf_group_open(arr, len(self.frontends), C.byref(self._g)))

    def close(self):
        if self._g:
            _check(lib().rcf_group_close(self._g))
            self._g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.frontends)

    def push(self, blocks, fmt=FMT_CF32, scale=1.0, offset=0.0):
        """blocks[i]: member i's next block (complex64 for FMT_CF32, interleaved I,Q in the wire type otherwise), or
        None / empty to skip the member this time."""
        n = len(self.frontends)
        if len(blocks) != n:
            raise ValueError("one block (or None) per member")
        dt = _WIRE_DTYPE[fmt]
        keep, ptrs, cnt = [], (C.c_void_p * n)(), (C.c_size_t * n)()
        for i, b in enumerate(blocks):
            if b is None or len(b) == 0:
                ptrs[i], cnt[i] = None, 0
                continue
            b = np.ascontiguousarray(b, dtype=dt)
            keep.append(b)
            ptrs[i] = b.ctypes.data
            cnt[i] = len(b) if fmt == FMT_CF32 else b.size // 2
        _check(lib().rcf_group_push(self._g, ptrs, cnt, int(fmt), float(scale), float(offset)))

    def commit(self, counts):
        n = len(self.frontends)
        cnt = (C.c_size_t * n)(*[int(c) for c in counts])
        _check(lib().rcf_group_commit(self._g, cnt))

    def sync(self):
        _check(lib().rcf_group_sync(self._g))

    def read_many(self, pairs, what="iq", gain=1.0, cap_each=1 << 14):
        """pairs: [(member index, channel id), ...] -> list of arrays (None where the channel is gone), ONE gather launch
        and one synchronisation for all of them (rcf_group_read_many)"""
        n = len(pairs)
        dt = _read_dtype(what)
        out = np.empty((max(n, 1), cap_each), dtype=dt)
        ms = (C.c_int * max(n, 1))(*[int(m) for m, _ in pairs])
        cs = (C.c_int * max(n, 1))(*[int(c) for _, c in pairs])
        counts = (C.c_int64 * max(n, 1))()
        _check(lib().rcf_group_read_many(self._g, _read_what(what, True), ms, cs, n, float(gain),
                                         out.ctypes.data_as(C.c_void_p), int(cap_each), counts))
        return [None if counts[i] < 0 else out[i, :counts[i]].copy() for i in range(n)]


class Pump:
    """The native real-time loop of a group (rcf_pump_t): one C++ thread takes whichever members' blocks are complete,
    pushes them as one group block, gathers the subscribed channels' new output into pinned host rings.  `rings[i]`: a
    PinnedArray (or any pinned uint8 / int8 / int16 / complex64 array) holding whole blocks of member i -- replayed
    cyclically at `samp_rate` of wall-clock time, block boundaries shifted by phase_s[i], or, where `written[i]` is a
    one-element uint64 array, taken block by block as its producer counts them complete.  Subscriptions may be given at
    start ((member, channel id) pairs delivered as `what` x `gain`) and change while it runs (subscribe / unsubscribe, up to
    `max_read` at a time).  what: "iq", "fm", "agc" or a stage's stream ("sym", "clock", "costas", "fsk4", "audio").
    subscribe() also takes what lies behind a slicer -- "hard", "sync" (uint32 items), "tsbk", "edacs", "osw", "p25lc"
    (records, their structured dtypes) --, and the capture stage's "capture" (cf32) and "capture_rec" (CAPTURE_REC_DTYPE
    records); the pump cannot be STARTED with one of those (RCF_EINVAL)."""

    def __init__(self, group, rings, block_samples, samp_rate, subscriptions=(), fmt=FMT_U8, scale=1.0, offset=0.0,
                 what="fm", gain=1.0, phase_s=None, out_ring_samples=4096, n_blocks=0, warm_blocks=0, max_batch=0,
                 cpu=-1, start_delay_s=0.05, batch_window_s=0.0, rt_priority=0, spin_us=0, written=None, max_read=0):
        self.group = group
        n = len(group)
        if len(rings) != n:
            raise ValueError("one source ring per member")
        self._keep = []
        bps = {FMT_CF32: 8, FMT_U8: 2, FMT_S8: 2, FMT_S16: 4}[fmt]
        rp, rb = (C.c_void_p * n)(), (C.c_size_t * n)()
        for i, r in enumerate(rings):
            a = r.array if isinstance(r, PinnedArray) else r
            self._keep.append(r)
            rp[i] = a.ctypes.data
            rb[i] = a.nbytes // (bps * int(block_samples))
            if rb[i] < 1:
                raise ValueError("source ring %d is shorter than one block" % i)
        ph = (C.c_double * n)(*([0.0] * n if phase_s is None else [float(x) for x in phase_s]))
        wr = None
        if written is not None and any(w is not None for w in written):
            wr = (C.c_void_p * n)()
            for i, w in enumerate(written):
                if w is None:
                    wr[i] = None
                    continue
                if w.dtype != np.uint64 or w.size < 1:
                    raise ValueError("written[%d] must be a uint64 array" % i)
                self._keep.append(w)
                wr[i] = w.ctypes.data
        ne = len(subscriptions)
        ms = (C.c_int * max(ne, 1))(*[int(m) for m, _ in subscriptions])
        cs = (C.c_int * max(ne, 1))(*[int(c) for _, c in subscriptions])
        cfg = PumpConfig()
        cfg.block_samples, cfg.fmt, cfg.scale, cfg.offset = int(block_samples), int(fmt), float(scale), float(offset)
        cfg.samp_rate = float(samp_rate)
        cfg.rings, cfg.ring_blocks, cfg.phase_s, cfg.written = rp, rb, ph, wr
        cfg.what, cfg.gain = _read_what(what, True), float(gain)
        cfg.read_members, cfg.read_chans, cfg.n_read = ms, cs, ne
        cfg.out_ring_samples, cfg.n_blocks, cfg.warm_blocks = int(out_ring_samples), int(n_blocks), int(warm_blocks)
        cfg.max_batch, cfg.cpu, cfg.start_delay_s = int(max_batch), int(cpu), float(start_delay_s)
        cfg.batch_window_s = float(batch_window_s)
        cfg.rt_priority = int(rt_priority)
        cfg.spin_us = int(spin_us)
        cfg.max_read = int(max_read)
        self.what = what
        self.n_entries = ne
        self.n_slots = max(ne, int(max_read), 1)
        self._cursors = [C.c_int64(0) for _ in range(self.n_slots)]
        self._what = [what] * self.n_slots
        for i, (_, c) in enumerate(subscriptions):
            if int(c) >= SRC_PFB_BIN0:                 # a bin of the member's fused discriminator ring: floats whatever `what` says
                self._what[i] = "fm"
        self._p = C.c_void_p()
        _check(lib().rcf_pump_start(group._g, C.byref(cfg), C.byref(self._p)))

    def stats(self):
        st = PumpStats()
        lib().rcf_pump_stats(self._p, C.byref(st))
        d = {k: getattr(st, k) for k, _ in PumpStats._fields_}
        if st.error:
            d["error_text"] = lib().rcf_last_error().decode("utf-8", "replace")
        return d

    def running(self):
        return bool(self.stats()["running"])

    def wait(self, timeout_s=60.0, poll_s=0.02):
        """until the pump has finished its n_blocks (or timeout) -> stats"""
        import time
        t_end = time.monotonic() + timeout_s
        while time.monotonic() < t_end:
            st = self.stats()
            if not st["running"]:
                return st
            time.sleep(poll_s)
        return self.stats()

    def subscribe(self, member, chan_id, what="iq", gain=1.0):
        """channel `chan_id` of member `member` from its next output on -> the slot (rcf_pump_subscribe; a stream behind the
        slicer: rcf_pump_subscribe_hard, counted in words, hits or records)"""
        cur = C.c_int64(0)
        if what in _HARD_WHAT or what == "capture_rec":
            e = _check(lib().rcf_pump_subscribe_hard(self._p, int(member), int(chan_id), _read_what(what, True), C.byref(cur)))
        else:
            e = _check(lib().rcf_pump_subscribe(self._p, int(member), int(chan_id), _read_what(what, True),
                                                float(gain), C.byref(cur)))
        self._cursors[e] = cur
        self._what[e] = what
        return e

    def subscribe_bin(self, member, bin_, gain=1.0):
        """bin `bin_` of member `member`'s fused discriminator ring (Frontend.pfb_fm_enable) from the bank's next frame on"""
        return self.subscribe(member, SRC_PFB_BIN0 + int(bin_), "fm", gain)

    def unsubscribe(self, entry):
        _check(lib().rcf_pump_unsubscribe(self._p, int(entry)))

    def written(self, entry):
        return _check(lib().rcf_pump_written(self._p, int(entry)))

    def read(self, entry, max_items=1 << 16):
        dt = _read_dtype(self._what[entry])
        out = np.empty(max_items, dtype=dt)
        n = _check(lib().rcf_pump_read(self._p, int(entry), C.byref(self._cursors[entry]),
                                       out.ctypes.data_as(C.c_void_p), int(max_items)))
        return out[:n].copy()

    def read_many_plan(self, entries, cap_each=1 << 13):
        """-> call() -> list of arrays (views into one buffer that the next call overwrites; None: no such slot): the new
        items of every listed slot with ONE native call (rcf_pump_read_many).  The call's arguments are built once.  Every
        row is cap_each x 8 bytes: cap_each items of up to 8 bytes, cap_each // 4 records of a frame decoder's slot (any
        cap_each: a record row is viewed over its whole records' bytes, the rest of the row stays unused)."""
        n = len(entries)
        ents = (C.c_int * max(n, 1))(*[int(e) for e in entries])
        curs = (C.c_int64 * max(n, 1))(*[self._cursors[e].value for e in entries])
        counts = (C.c_int64 * max(n, 1))()
        out = np.empty((max(n, 1), cap_each), dtype=np.complex64)
        rows = []                                                # each row as its slot's items
        for i, e in enumerate(entries):
            dt = np.dtype(_read_dtype(self._what[e]))
            per = max(1, dt.itemsize // 8)                        # 8-byte units of the row per item (records: 4)
            rows.append(out[i, :cap_each // per * per].view(dt))
        fn, pp, op = lib().rcf_pump_read_many, self._p, out.ctypes.data_as(C.c_void_p)

        def call():
            _check(fn(pp, ents, curs, n, op, int(cap_each), counts))
            res = []
            for i in range(n):
                c = counts[i]
                self._cursors[entries[i]].value = curs[i]
                res.append(None if c < 0 else rows[i][:c])
            return res
        return call

    def stop(self):
        if self._p:
            lib().rcf_pump_stop(self._p)
            self._p = C.c_void_p()
            self._keep = []

    def __del__(self):
        try:
            self.stop()
        except Exception:
            pass
