"""The dense code-word streams (tests/codewords_ref.py) without a GPU: the generators alone meet their censuses under the
restatements (p25es_ref, nid_ref), nothing skipped, and the kernels' arithmetic headers compiled for the host
(tests/native/p25es_core_check.cpp, tests/native/nid_core_check.cpp: the stand-alone programs of tests/test_p25es_cpu.py and
tests/test_nid_cpu.py) answer the same records and counters on them.  This is the check that the inputs of
tests/test_gpu_codewords.py are right before a device sees them."""
import numpy as np
import pytest

import codewords_ref as CW
import nid_ref as N
import p25es_ref as E
from rcf import native
from test_nid_cpu import check_programs as nid_programs, through_header as nid_through_header      # noqa: F401 (a fixture)
from test_p25es_cpu import check_programs as es_programs, slicer_streams, through_header as es_through_header      # noqa: F401

BOTH, ES_ALONE = E.ES | E.ERASURES, E.ES


@pytest.fixture(scope="module")
def dense_rs():
    """-> (dibits, plan, words, k, dist) of the dense Reed-Solomon stream, sliced by the restatement"""
    d, plan = CW.dense_rs_dibits()
    return (d, plan) + slicer_streams(d)


@pytest.fixture(scope="module")
def dense_nid():
    d, plan = CW.dense_nid_dibits()
    return (d, plan) + slicer_streams(d)


def test_dense_reed_solomon_stream_meets_its_census(dense_rs):
    d, plan, words, k, dist = dense_rs
    assert 150000 < len(d) < 220000 and len(plan) == 302
    assert sum(p["what"] == "inside" for p in plan) == 81 + 49 + 28 + 25
    assert (np.asarray(k) - 23).tolist() == [p["start"] for p in plan] and not np.any(dist)       # every planted frame, and nothing else
    recs, st = E.run(words, k, dist, options=BOTH)
    plain, plain_st = E.run(words, k, dist, options=ES_ALONE)
    CW.check_rs_census(recs, plain, plan)
    n_beyond = sum(p["what"] == "beyond" for p in plan)
    assert st["n_lost"] == plain_st["n_lost"] == 0 and st["n_frames"] == st["n_records"] == st["n_decoded"] == len(plan)
    assert 0 < st["n_rs_bad"] <= n_beyond < plain_st["n_rs_bad"]             # inside the bound nothing is given up; without the option much is
    f = native.p25lc_fields(recs)
    inside = np.array([p["what"] != "beyond" for p in plan])
    assert not np.any(f["rs_bad"][inside]) and int(f["n_rs"][inside].max()) == 16 and set(f["kind"].tolist()) == {0, 1, 2, 4}
    # a census that does its work: a unit's n_rs off by one, a frame dropped
    wrong = recs.copy()
    wrong["flags"][5] ^= 1 << 4
    with pytest.raises(AssertionError):
        CW.check_rs_census(wrong, plain, plan)
    with pytest.raises(AssertionError):
        CW.check_rs_census(recs[1:], plain[1:], plan)


def test_one_series_alone_meets_its_census():
    for kind in CW.SERIES:
        d, plan = CW.dense_rs_dibits(series=(kind,))
        words, k, dist = slicer_streams(d)
        assert (np.asarray(k) - 23).tolist() == [p["start"] for p in plan] and {p["kind"] for p in plan} == {kind}
        CW.check_rs_census(E.run(words, k, dist, options=BOTH)[0], E.run(words, k, dist, options=ES_ALONE)[0], plan, series=(kind,))


@pytest.mark.parametrize("options", [BOTH, ES_ALONE])
def test_header_programs_equal_the_restatement_on_the_dense_reed_solomon_stream(es_programs, tmp_path, dense_rs, options):
    d, plan, words, k, dist = dense_rs
    want, want_st = E.run(words, k, dist, options=options)
    for cuts in ([], list(range(0, len(d), 9973))):
        got, st, _ = es_through_header(es_programs, tmp_path, words, k, dist, cuts, len(d), options=options)
        assert got.tobytes() == want.tobytes() and st == want_st, (options, cuts[:4])


def restate_nid(stage, words, k, dist, nid):
    return N.run_tsbk(words, k, dist, nid=nid) if stage == "tsbk" else N.run_voice(words, k, dist, nid=nid, options=BOTH)


@pytest.mark.parametrize("stage", ["tsbk", "voice"])
def test_dense_nid_stream_meets_its_census_and_header_programs_equal_the_restatement(nid_programs, tmp_path, dense_nid, stage):
    d, plan, words, k, dist = dense_nid
    assert len(plan) == 64 + 10 * 14 + 2 * 12 + 6 and len(d) < 25000
    assert (np.asarray(k) - 23).tolist() == [p["start"] for p in plan] and not np.any(dist)
    recs, st, nst = restate_nid(stage, words, k, dist, 1)
    raw, raw_st, raw_nst = restate_nid(stage, words, k, dist, 0)
    CW.check_nid_census(stage, recs, raw, plan, nst)
    assert st["n_lost"] == raw_st["n_lost"] == 0 and st["n_frames"] == raw_st["n_frames"] == len(plan)
    assert raw_nst == dict(n_decoded=0, n_fixed=0, n_bits=0, n_bad=0) and nst["n_bad"] >= 10
    wrong = recs.copy()
    wrong["frame_dibits" if stage == "tsbk" else "tail"][7] ^= 1 << (16 if stage == "tsbk" else 28)
    with pytest.raises(AssertionError):
        CW.check_nid_census(stage, wrong, raw, plan, nst)
    opt = 0 if stage == "tsbk" else BOTH
    for nid, want in ((1, (recs, st, nst)), (0, (raw, raw_st, raw_nst))):
        for cuts in ([], list(range(0, len(d), 997))):
            got, got_st, got_nst, _ = nid_through_header(nid_programs, tmp_path, stage, words, k, dist, cuts, len(d), nid, options=opt)
            assert got.tobytes() == want[0].tobytes() and (got_st, got_nst) == want[1:], (nid, cuts[:4])
