"""The polyline stage alone (rd_polyline_planes_device: rdk::polyline + rdk::polyline_ids) on the crafted masks of tests/polycases.py, in both forms -
0 = the multi-launch form (oclpolyline_execute, the detectors' repeat), 1 = the single-block kernel k_poly_persistent, which the detectors try first
and which the suite otherwise reaches through whole frames only.  List and id plane against rdo_polyline bit for bit; the single-block kernel's
overflow flag against what each case expects; where it flags, the multi-launch form still gives the oracle's list.  The tie fixtures (orphan records:
two join steps with one right neighbour) three times per form with identical bytes - on lists of more than 1024 records the old schedule raced."""
import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers, polycases as pc

CASES = pc.all_cases()
FORMS = (0, 1)


def run(case, form):
    mask, nbytes, _ = pc.resolve(case)
    return ra.polyline_planes_device(mask, case.ring, case.minerror, case.size_thre, nbytes, form)


def check_equal(case, got, form):
    _, _, (want, want_ids, _) = pc.resolve(case)
    segs, ids, ctr = got
    assert helpers.segments_equal(segs, want), f"{case.name} form {form}: {int(segs.view('i4')[0])} records, oracle {int(want.view('i4')[0])}"
    m = want[1:]["polyid"] != 0
    assert segs[1:][m].tobytes() == want[1:][m].tobytes()
    assert np.array_equal(ids, want_ids), f"{case.name} form {form}: id plane"


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(case, form):
    got = run(case, form)
    ctr = got[2]
    print(case.name, "form", form, "chain pixels", int(ctr[0]), "chains", int(ctr[1]), "live", int(ctr[24]), "overflow", int(ctr[25]), "records", int(got[0].view("i4")[0]))
    info = pc.resolve(case)[2][2]
    assert int(ctr[1]) == info["chains"] and int(ctr[24]) == info["live"]
    if form == 1:
        assert (int(ctr[25]) != 0) == case.flag1, f"{case.name}: overflow flag {int(ctr[25])}, expected {case.flag1}"
        if case.flag1:
            return      # (the flagged kernel's list means nothing; the multi-launch form of the same case is checked by form 0)
    else:
        assert int(ctr[25]) == 0
    check_equal(case, got, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", [c for c in CASES if c.tie], ids=repr)
def test_tie_fixture_is_stable(case, form):
    """three runs, identical bytes (the whole list: records with polyid == 0 included), each the oracle's"""
    runs = [run(case, form) for _ in range(3)]
    for got in runs:
        assert int(got[2][25]) == 0
        check_equal(case, got, form)
    assert runs[0][0].tobytes() == runs[1][0].tobytes() == runs[2][0].tobytes()
    assert runs[0][1].tobytes() == runs[1][1].tobytes() == runs[2][1].tobytes()


@pytest.mark.gpu
def test_invalid_arguments():
    L = ra.lib()
    m = np.ones((16, 16), np.int32)
    out, ids, ctr = np.zeros(16 * 16 * 4, np.int32), np.zeros(256, np.int32), np.zeros(64, np.int32)
    call = lambda iw=16, ih=16, nbytes=4096, form=0, size_thre=1: L.rd_polyline_planes_device(0, m.ctypes.data, iw, ih, 0, 1.0, size_thre, nbytes, form, out.ctypes.data, ids.ctypes.data, ctr.ctypes.data)
    assert call() == 0
    assert call(iw=4) == -1 and call(ih=0) == -1 and call(nbytes=111) == -1 and call(nbytes=4097) == -1 and call(form=2) == -1 and call(size_thre=-1) == -1
