"""The region stage alone (rd_region_planes_device: region_merge, region_size, despeckle2 / despeckle2_slow, label8_boundary) on the crafted planes of tests/regioncases.py.
All five planes against the oracle bit for bit - rdo_region_concurrent limited to the budget the ladder ends on, the junction counts + rdo_region_size, rdo_despeckle2 in
serial raster order, rdo_mark_boundary, rdo_label8 - and, from the tap's info block, the path each case was built for: final budget, settled or not, the flags of the
launches, the absorption's status words, slow path or not.  A case that stops reaching its edge fails.  No tolerances."""
import os

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import regioncases as rc

LIM = rc.LIM
STAGE0 = [c for c in rc.CASES if c.stage == 0]
STAGE1 = [c for c in rc.CASES if c.stage == 1]


def run(case, force_slow=False):
    if case.stage == 0:
        return ra.region_planes_device(*case.planes, launches=case.launches, force_slow=force_slow)
    return ra.region_planes_device(region0=case.planes[0], rsize=case.planes[1], force_slow=force_slow)


def check_planes(case, got, what=""):
    e = rc.expected(case)
    for name in ("region0", "rsize", "region", "boundarysrc", "boundary"):
        a, b = getattr(got, name).reshape(-1), e[name]
        assert np.array_equal(a, b), f"{case.name}{what}: plane {name} differs from the oracle in {int((a != b).sum())} elements"
    assert (got.region >= 0).all(), f"{case.name}{what}: undecided words left in region"


def check_status(case, got, forced):
    """the absorption's path: status[0] (gave up), status[1] (undecided pixels: the count the case names, else inside the range the tile kernel's rule allows), status[2]
    (sweeps: none without undecided pixels or beyond the tail's capacity, AT_SWEEPS where the case is built to exhaust them), slow path exactly where asked for"""
    e = rc.expected(case)
    lo, hi = e["undecided"]
    reccap = ra.region_limits(case.iw, case.ih)["reccap"]
    s0, s1, s2, _ = got.status
    assert lo <= s1 <= hi, (case.name, got.status, (lo, hi))
    if "undecided" in case.expect:
        assert s1 == case.expect["undecided"]
    if s1 == 0 or s1 > reccap:
        assert s2 == 0 and (s0 != 0) == (s1 > reccap)
    else:
        assert 1 <= s2 <= LIM["AT_SWEEPS"] and (s0 != 0) == (s2 == LIM["AT_SWEEPS"] and "sweeps" in case.expect)
    if "status0" in case.expect:
        assert (s0 != 0) == bool(case.expect["status0"])
    if "sweeps" in case.expect:
        assert s2 == case.expect["sweeps"] == LIM["AT_SWEEPS"]
    assert got.slow == (forced or s0 != 0)
    if "slow" in case.expect:
        assert (s0 != 0) == case.expect["slow"]
    if got.slow:
        bound = ra.region_limits(case.iw, case.ih)["slow_bound"]
        # (the slow path counts launches of two Jacobi rounds each, eight at a time)
        assert (e["jacobi_rounds"] + 1) // 2 <= got.slow_launches + 1 and got.slow_launches <= (e["jacobi_rounds"] + 1) // 2 + 9 and got.slow_launches < bound, (got.slow_launches, e["jacobi_rounds"], bound)
    else:
        assert got.slow_launches == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", STAGE0, ids=repr)
def test_stage0(case):
    e = rc.expected(case)
    got = run(case)
    print(case.name, f"{case.iw}x{case.ih}", "needed", e["needed"], "budget", got.budget, "settled", got.settled, "status", got.status, "slow", got.slow, got.slow_launches)
    assert (got.budget, got.settled) == (e["budget"], e["settled"])
    changed = np.arange(got.budget) < max(e["needed"], 2) - 1      # launch r changed something <=> it is not the quiet one or behind it
    assert np.array_equal(got.flags != 0, changed), (case.name, got.flags.tolist())
    assert not got.info[got.budget:LIM["max_launches"]].any()
    check_planes(case, got)
    check_status(case, got, False)


@pytest.mark.gpu
@pytest.mark.parametrize("forced", (False, True), ids=("fast", "forced_slow"))
@pytest.mark.parametrize("case", STAGE1, ids=repr)
def test_stage1(case, forced):
    got = run(case, forced)
    print(case.name, f"{case.iw}x{case.ih}", "forced" if forced else "fast", "status", got.status, "slow", got.slow, got.slow_launches, "undecided", rc.expected(case)["undecided"])
    assert got.budget == 0 and got.settled and not got.info[:LIM["max_launches"]].any()
    check_planes(case, got, " forced slow" if forced else "")
    check_status(case, got, forced)


@pytest.mark.gpu
def test_two_wave_cascade_with_a_forced_slow_absorption():
    """stage 0 honours force_slow as well: same planes"""
    case = rc.BY_NAME[f"two_wave_h{rc.MIN_SIDE}"]
    got = run(case, True)
    assert got.slow
    check_planes(case, got)


@pytest.mark.gpu
def test_invalid_arguments_and_the_call_after():
    L = ra.lib()
    case = rc.BY_NAME["asym_edge"]
    iw, ih, n = case.iw, case.ih, case.iw * case.ih
    pix, mask, edge = (np.ascontiguousarray(p, dtype=np.int32) for p in case.planes)
    lab, size = np.zeros(n, np.int32), np.ones(n, np.int32)
    outs = [np.zeros(n, np.int32) for _ in range(5)]
    info = np.zeros(ra.REGION_INFO_INTS, np.int32)

    def call(stage=0, iw=iw, ih=ih, a=(pix, mask, edge), launches=0, b=(lab, size), outs=outs, info=info):
        p = lambda x: None if x is None else x.ctypes.data
        return L.rd_region_planes_device(0, stage, iw, ih, p(a[0]), p(a[1]), p(a[2]), launches, p(b[0]), p(b[1]), 0, *[p(o) for o in outs], p(info))

    assert call() == 0
    assert call(a=(None, mask, edge)) == -1 and call(a=(pix, None, edge)) == -1 and call(a=(pix, mask, None)) == -1
    assert call(outs=outs[:4] + [None]) == -1 and call(info=None) == -1 and call(stage=1, b=(None, size)) == -1 and call(stage=1, b=(lab, None)) == -1
    assert call(iw=15) == -1 and call(ih=15) == -1 and call(iw=1 << 13, ih=1 << 12) == -1 and call(iw=0) == -1
    assert call(launches=1) == -1 and call(launches=7) == -1 and call(launches=-2) == -1 and call(launches=LIM["max_launches"] + 2) == -1
    assert call(launches=2) == 0 and call(launches=LIM["max_launches"]) == 0
    assert call(stage=2) == -1 and call(stage=-1) == -1
    bad = lab.copy()
    bad[5] = n
    assert call(stage=1, b=(bad, size)) == -1
    bad[5] = -1
    assert call(stage=1, b=(bad, size)) == -1
    big = size.copy()
    big[0] = 1 << LIM["size_bits"]
    assert call(stage=1, b=(lab, big)) == -1
    big[0] = -1
    assert call(stage=1, b=(lab, big)) == -1
    big[0] = (1 << LIM["size_bits"]) - 1
    assert call(stage=1, b=(lab, big)) == 0
    check_planes(case, run(case), " after the refused calls")


@pytest.mark.gpu
def test_calls_in_a_row_do_not_see_each_other():
    """the unsettled cascade, a plane that takes the slow path, a settled one, the first again: each its own result, the repeat identical in every byte"""
    names = (f"cascade_n65_h{rc.MIN_SIDE}", "all_small_64x64", "asym_edge", "undecided_1025", f"cascade_n65_h{rc.MIN_SIDE}")
    runs = []
    for n in names:
        runs.append(run(rc.BY_NAME[n]))
        check_planes(rc.BY_NAME[n], runs[-1], " in a row")
    assert not runs[0].settled and runs[1].slow and runs[2].settled and not runs[2].slow and runs[3].status[1] == 1025
    for name in ("region0", "rsize", "region", "boundarysrc", "boundary"):
        assert getattr(runs[0], name).tobytes() == getattr(runs[4], name).tobytes()
    assert runs[0].info[:136].tobytes() == runs[4].info[:136].tobytes()


@pytest.mark.gpu
def test_frame_path_counters_still_move():
    """the ladder is one function now (region_ladder): on the RD_REGION_ROUNDS_FIXED=8 fixture of test_region_round_budget_does_not_change_results frames are still
    repeated (counter 4, n_redo_rounds), none of them ends unsettled (counter 6, n_unsettled), and the repeated frames give the planes of a budget of 20"""
    iw, ih = 1920, 1080
    frames = [synth.frame(synth.SEED0 + 9, iw, ih, t) for t in range(3)]
    regions = []
    for fixed in ("8", "20"):
        old = os.environ.get("RD_REGION_ROUNDS_FIXED")
        os.environ["RD_REGION_ROUNDS_FIXED"] = fixed
        det = ra.Detector(iw, ih, nslots=1)
        os.environ.pop("RD_REGION_ROUNDS_FIXED") if old is None else os.environ.__setitem__("RD_REGION_ROUNDS_FIXED", old)
        out = []
        for f in frames:
            det.enqueue(f)
            det.poll(np.tan(np.pi / 5))
            out.append(det.plane("region").copy())
        redo, unsettled = int(ra.lib().rd_detector_counter(det.h, 4)), int(ra.lib().rd_detector_counter(det.h, 6))
        print("fixed", fixed, "repeated frames", redo, "unsettled", unsettled)
        assert unsettled == 0 and (redo > 0) == (fixed == "8") and det.region_round_budget()[1] == redo
        det.close()
        regions.append(out)
    for a, b in zip(*regions):
        assert np.array_equal(a, b)
