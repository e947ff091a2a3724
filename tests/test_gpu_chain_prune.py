"""The polyline stage alone (rd_polyline_planes_device) on the masks of tests/prunecases.py, in both forms (0 = multi-launch, 1 = the single-block kernel): list and
id plane against rdo_polyline bit for bit, ctr[1] / ctr[24] against the oracle's chains / live pixels as tests/test_gpu_polycases.py does, and the prefilter's own
counters - ctr[0] chain pixels, ctr[26] chain pixels in components of more than size_thre pixels - against what the oracle's taps give.  Each case three times with
identical bytes: the order in which concurrent unions land differs from run to run, the result must not."""
import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers, prunecases as pr

CASES = pr.all_cases()
FORMS = (0, 1)


def run(case, form):
    mask, nbytes, _ = pr.resolve(case)
    return ra.polyline_planes_device(mask, case.ring, case.minerror, case.size_thre, nbytes, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(case, form):
    _, _, (want, want_ids, info) = pr.resolve(case)
    f = pr.facts(case)
    runs = [run(case, form) for _ in range(3)]
    for segs, ids, ctr in runs:
        print(case.name, "form", form, "chain pixels", int(ctr[0]), "survivors", int(ctr[26]), "chains", int(ctr[1]), "live", int(ctr[24]), "overflow", int(ctr[25]), "records", int(segs.view("i4")[0]))
        assert int(ctr[0]) == f["chain_pixels"] and int(ctr[26]) == f["survivors"]
        assert int(ctr[1]) == info["chains"] and int(ctr[24]) == info["live"]
        if form == 1:
            assert (int(ctr[25]) != 0) == case.flag1, f"{case.name}: overflow flag {int(ctr[25])}, expected {case.flag1}"
            if case.flag1:
                continue      # (the flagged kernel's list means nothing; form 0 of the same case is compared)
        else:
            assert int(ctr[25]) == 0
        assert helpers.segments_equal(segs, want), f"{case.name} form {form}: {int(segs.view('i4')[0])} records, oracle {int(want.view('i4')[0])}"
        m = want[1:]["polyid"] != 0
        assert segs[1:][m].tobytes() == want[1:][m].tobytes()
        assert np.array_equal(ids, want_ids), f"{case.name} form {form}: id plane"
    if not (form == 1 and case.flag1):
        assert runs[0][0].tobytes() == runs[1][0].tobytes() == runs[2][0].tobytes()
        assert runs[0][1].tobytes() == runs[1][1].tobytes() == runs[2][1].tobytes()
