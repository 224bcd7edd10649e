"""The binding's names for the stages' streams (RCF_READ_SYM .. RCF_READ_AUDIO) without a GPU: the constants, the mapping
every reader of rcf.native uses, the item types -- and that "iq" / "fm" / "agc" map as they always did."""
import re

import numpy as np

from rcf import native


def test_read_constants_are_the_headers():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rcf.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define RCF_READ_(\w+)\s+(\d+)", hdr)}
    assert vals == {"IQ": 0, "FM": 1, "AGC": 2, "SYM": 16, "CLOCK": 17, "COSTAS": 18, "FSK4": 19, "AUDIO": 20}
    for name, v in vals.items():
        assert getattr(native, "READ_" + name) == v


def test_stage_names_map_to_their_streams_and_the_old_three_are_unchanged():
    want = {"sym": native.READ_SYM, "clock": native.READ_CLOCK, "costas": native.READ_COSTAS, "fsk4": native.READ_FSK4,
            "audio": native.READ_AUDIO}
    for name, v in want.items():
        assert native._read_what(name, True) == v
        assert native._read_dtype(name) == np.float32
    for stages in (False, True):
        assert native._read_what("iq", stages) == native.READ_IQ == 0
        assert native._read_what("fm", stages) == native.READ_FM == 1
        assert native._read_what("agc", stages) == native.READ_AGC == 2
        for other in ("FM", None, "bits"):                     # anything unknown stays the discriminator
            assert native._read_what(other, stages) == native.READ_FM
    assert native._read_what("iq") == native.READ_IQ and native._read_what("agc") == native.READ_AGC
    for name in list(want) + ["fm"]:                           # the one-argument form answers as it always has
        assert native._read_what(name) == native.READ_FM
    assert native._read_dtype("iq") == native._read_dtype("agc") == np.complex64
    assert native._read_dtype("fm") == np.float32
    assert len(set(want.values()) | {0, 1, 2}) == 8 and min(want.values()) >= 16   # 3 .. 15 are nobody's
