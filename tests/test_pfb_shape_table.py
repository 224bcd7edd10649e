"""The filterbank shape table (radiocapture-rf_amd/csrc/pfb_shape.h) answers what the scattered host functions it replaced
answered: tests/golden/pfb_shapes.json holds those answers, taken from the commit before the table over a grid of bin counts
(every family, and counts with no kernel: 25, 32, 200, 228, 2048, 6400), decimations NB / {1, 2, 3, 4, 8} and prototype
lengths of 1 .. 17 taps per branch (P NB and (P - 1) NB + 1 taps).  The C ABI gives the first two columns; the header itself,
compiled alone with g++ (tests/native/pfb_shape_check.cpp), gives every column, and the same program holds
pfb_zero_history to the written-out predicate for n_lo in [-2, 40], three start samples and both halo values."""
import json
import os
import subprocess

from rcf import native

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NBS = [25, 32, 64, 128, 160, 192, 200, 228, 256, 400, 480, 512, 640, 800, 960, 1024, 1280, 1600, 2048, 3200, 6400]


def _golden():
    g = json.load(open(os.path.join(HERE, "golden", "pfb_shapes.json")))
    assert g["columns"][:5] == ["NB", "D", "ntaps", "supported", "family"] and len(g["columns"]) == 14
    want = [(nb, nb // dv, nt) for nb in NBS for dv in (1, 2, 3, 4, 8) if nb % dv == 0
            for p in range(1, 18) for nt in (p * nb, (p - 1) * nb + 1)]
    assert [tuple(r[:3]) for r in g["rows"]] == want            # the whole grid, nothing dropped
    return g


def test_abi_answers_supported_and_family_over_the_grid():
    g = _golden()
    bad = [r[:5] for r in g["rows"]
           if (int(native.pfb_shape_supported(r[0], r[1], r[2])), native.pfb_shape_family(r[0], r[1], r[2])) != (r[3], r[4])]
    assert not bad, bad[:10]
    assert sum(r[3] for r in g["rows"]) == 400


def test_shape_table_alone_answers_every_column_and_the_zero_history_predicate():
    g = _golden()
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "pfb_shape_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "radiocapture-rf_amd", "csrc"),
                           os.path.join(HERE, "native", "pfb_shape_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    got = json.loads(p.stdout.decode())
    assert len(got["rows"]) == len(g["rows"])
    bad = [(a, b) for a, b in zip(got["rows"], g["rows"]) if a != b]
    assert not bad, bad[:10]
    # 400 supported rows x 3 start samples x 2 halo values x 43 first frames
    assert got["zero_history_checked"] == 400 * 3 * 2 * 43 and got["zero_history_mismatches"] == 0
