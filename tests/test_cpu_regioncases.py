"""What every crafted plane of tests/regioncases.py claims about itself, asserted from the oracle alone (no GPU): launches the merge needs, the lag table of the two-wave
cascade, small-pixel counts, which pixels tie, that the serial sweep equals the Jacobi fixed point - and one CONDITION: no case comes near the launches after which
despeckle2_slow calls a missing fixed point an internal error (rd_region_limits).  A case that cannot pass here is not sent to a GPU."""
import numpy as np
import pytest

import rectdetect_amd as ra
from tests import regioncases as rc

LIM = rc.LIM
STAGE0 = [c for c in rc.CASES if c.stage == 0]
STAGE1 = [c for c in rc.CASES if c.stage == 1]


def test_limits_are_the_documented_ones():
    """the constants as the kernels' comments and DESIGN.md state them: a change of one of them is a change of the cases, which this makes visible"""
    assert LIM["first_budget"] == 20 and LIM["ladder"] == [32, 64, 128] and LIM["max_launches"] == LIM["ladder"][-1]
    assert LIM["AT_CAP"] == 16383 and LIM["AT_SWEEPS"] == 64 and LIM["AT_NT"] == 1024 and LIM["AB_HK"] == 16 and LIM["AB_OWNED"] == 2048
    assert LIM["merge_tile"] == (64, 32) and LIM["absorb_tile"] == (64, 64) and LIM["thre"] == 16 and LIM["size_bits"] == 26
    assert LIM["EPT"] == sorted(LIM["EPT"]) and LIM["EPT"][-1] * LIM["AT_NT"] > LIM["AT_CAP"]
    assert LIM["slow_bound"] == 0 and LIM["reccap"] == 0
    l = ra.region_limits(128, 128)
    assert l["slow_bound"] == 128 + 2 * 128 + 16 and l["reccap"] == 128 * 128 // 4
    assert ra.region_limits(1920, 1080)["reccap"] == LIM["AT_CAP"]


@pytest.mark.parametrize("h", rc.CASCADE_H_ORACLE)
@pytest.mark.parametrize("n", rc.CASCADE_N)
def test_cascade_needs_2n_launches(n, h):
    pix, mask, edge = rc.cascade(n, h)
    assert pix.shape == (h, 2 * n + 4)
    lab, needed = rc.oracle_merge(pix, mask, edge, 1000)
    assert needed == 2 * n
    # the last stripe's label (its corridor's first pixel) has reached every stripe
    assert all(lab[(h // 2) * pix.shape[1] + 2 + 2 * i] == pix.shape[1] + 1 for i in range(n))
    one_less, _ = rc.oracle_merge(pix, mask, edge, needed - 2)
    assert not np.array_equal(one_less, lab)


def test_cascade_ends_on_every_rung():
    ends = {n: rc.ladder_end(2 * n) for n in rc.CASCADE_N}
    f, (a, b, c) = LIM["first_budget"], LIM["ladder"]
    assert ends == {9: (f, True), 10: (f, True), 11: (a, True), 16: (a, True), 17: (b, True), 32: (b, True), 33: (c, True), 64: (c, True), 65: (c, False)}
    assert [2 * n for n in rc.CASCADE_N] == [f - 2, f, f + 2, a, a + 2, b, b + 2, c, c + 2]


@pytest.mark.parametrize("case", [c for c in STAGE0 if "budget" in c.name], ids=repr)
def test_fixed_budget_keeps_what_its_launches_made(case):
    e = rc.expected(case)
    assert e["needed"] == 32 and e["budget"] == case.launches and e["settled"] is False
    full, _ = rc.oracle_merge(*case.planes, 1000)
    assert not np.array_equal(e["region0"], full)


@pytest.mark.parametrize("h", (rc.MIN_SIDE, 70))
def test_two_wave_lag_table(h):
    pix, mask, edge = rc._two_wave(h)
    if h == rc.MIN_SIDE:
        assert pix.shape == (16, 48)
    table, needed = rc.lag_table(pix, mask, edge)
    print("two-wave cascade, h =", h, "launches", needed, "lags:", sorted(table.items()))
    assert needed == rc.TWO_WAVE["launches"] <= LIM["ladder"][0]
    for lag in range(1, 29):
        assert table.get(lag, 0) >= 9, (lag, table)
    assert all(table[l] > 0 for l in rc.TWO_WAVE["lags"])


def _labels(e, case):
    return e["region0"].reshape(case.ih, case.iw)


def test_asym_edge_claim():
    c = rc.BY_NAME["asym_edge"]
    lab = _labels(rc.expected(c), c)
    assert len(set(lab[6:13, 4])) == 1 and len(set(lab[4:13, 5])) == 1 and lab[10, 4] != lab[10, 5]          # edges on the right pixels of the pairs: two regions
    assert set(lab[6:13, 14]) == set(lab[4:13, 15]) == {4 * c.iw + 15}                                       # edges on the left pixels: one
    for kind, (ny, nx) in (("up", (7, 1)), ("left", (9, -1)), ("down", (11, 1))):
        refused, allowed = rc.ASYM_BLOCKS[kind]
        assert set(lab[8:11, refused:refused + 3].reshape(-1)) == {8 * c.iw + refused}, kind                 # the edge on the pixel the test reads: the block keeps its label
        assert lab[ny, allowed + nx] < 8 * c.iw + allowed and set(lab[8:11, allowed:allowed + 3].reshape(-1)) == {lab[ny, allowed + nx]}, kind      # on the other pixel: the neighbour's


def merge_restated(pix, mask, edge, flip=None):
    """rdo_region_concurrent in Python, run until a launch changes nothing; flip = a direction (up, left, right, down) whose edge test reads the OTHER pixel of the pair"""
    ih, iw = pix.shape
    pix, mask, edge = (p.reshape(-1) for p in (pix, mask, edge))
    label, _ = rc.oracle_merge(pix.reshape(ih, iw), mask.reshape(ih, iw), edge.reshape(ih, iw), 0)
    label = label.copy()
    for _ in range(200):
        nxt = label.copy()
        changed = False
        for y in range(1, ih - 1):
            for x in range(1, iw - 1):
                p0 = y * iw + x
                og = g = int(label[p0])
                for kind, p1, reads_neighbour in (("up", p0 - iw, False), ("left", p0 - 1, False), ("right", p0 + 1, True), ("down", p0 + iw, True)):
                    e = p1 if reads_neighbour != (kind == flip) else p0
                    s = int(label[p1])
                    if s < g and (pix[p0] == pix[p1] or mask[p0] != 0) and edge[e] <= 0:
                        g = s
                for _j in range(8):
                    g = int(label[g])
                if g != og:
                    nxt[og] = min(nxt[og], g)
                    nxt[p0] = min(nxt[p0], g)
                    changed = True
        label = nxt
        if not changed:
            return label
    raise AssertionError("the restated merge did not settle")


@pytest.mark.parametrize("flip", (None, "up", "left", "right", "down"))
def test_asym_edge_catches_every_wrong_edge_test(flip):
    """a merge that read the edge plane at the wrong pixel of the pair, in any one direction, gives other labels on the plane; the restatement itself equals the oracle"""
    c = rc.BY_NAME["asym_edge"]
    got = merge_restated(*c.planes, flip=flip)
    assert np.array_equal(got, rc.expected(c)["region0"]) == (flip is None)


def test_mask_directions_claim():
    c = rc.BY_NAME["mask_directions"]
    lab = _labels(rc.expected(c), c)
    joined = [bool(lab[12, x0 + 1] == lab[12, x0 + 4]) for x0 in (2, 12, 22, 32)]
    # (low right, mask left): joins; (low left, mask right): joins; (low right, mask right) and (low left, mask left): the masked side has nothing to adopt
    assert joined == [True, True, False, False]


def test_ring_parent_claim():
    c = rc.BY_NAME["ring_parent"]
    pix, mask, edge = c.planes
    lab = _labels(rc.expected(c), c)
    init, _ = rc.oracle_merge(pix, mask, edge, 0)
    init = init.reshape(c.ih, c.iw)
    assert lab[9, 0] == 9 * c.iw and lab[17, 10] == 17 * c.iw + 10            # masked ring pixels adopt nothing
    assert lab[9, 1] != 9 * c.iw + 1                                          # the masked interior pixel does
    ring = np.ones(lab.shape, bool)
    ring[1:-1, 1:-1] = False
    assert (lab[ring] != init[ring]).any()                                    # ring pixels were hooked: they serve as parents
    assert len(np.unique(lab[pix == 3])) == 1


@pytest.mark.parametrize("case", [c for c in STAGE0 if c.name.startswith("word_straddle")], ids=repr)
def test_word_straddle_claim(case):
    pix, mask, edge = case.planes
    e = rc.expected(case)
    assert e["settled"] and e["budget"] == LIM["first_budget"]
    for plane, what in ((mask, "mask"), (edge, "edge")):      # every masked / edge pixel matters: without the plane the merge gives other labels
        other, _ = rc.oracle_merge(pix, mask * (what != "mask"), edge * (what != "edge"), 1000)
        assert not np.array_equal(other, e["region0"]), what
    lab = _labels(e, case)
    assert pix[11, case.iw - 2] != pix[11, case.iw - 1] and edge[17, case.iw - 1] and not edge[20, case.iw - 1]
    assert lab[17, case.iw - 2] == 17 * case.iw + case.iw - 2 and lab[20, case.iw - 2] == case.iw - 1      # the last column's edge bit decides
    if case.iw >= 72:
        assert pix[11, 63] != pix[11, 64] and mask[11, 63] and edge[11, 64]


def test_junction_threshold_claim():
    c = rc.BY_NAME["junction_threshold"]
    pix, _, _ = c.planes
    e = rc.expected(c)
    region = e["region"].reshape(c.ih, c.iw)
    sizes = [int(e["rsize"][5 * c.iw + 4 + 10 * k]) for k in range(4)]
    assert sizes == [15, 17, 16, 18] and LIM["thre"] == 16
    kept = [bool((region[pix == k + 1] == 5 * c.iw + 4 + 10 * k).all()) for k in range(4)]
    gone = [bool((region[pix == k + 1] != 5 * c.iw + 4 + 10 * k).all()) for k in range(4)]
    assert kept == [False, True, False, True] and gone == [True, False, True, False]


@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_case_condition_and_fixed_point(case):
    """the serial sweep equals the Jacobi fixed point, and the launches the slow path would take (two rounds each) stay below its internal-error bound; stage 0 after the
    merge.  Also what a case says about its undecided pixels and about its seed."""
    e = rc.expected(case)
    jac, rounds = rc.jacobi_rounds(e["region0"], e["rsize"], case.iw, case.ih)
    assert np.array_equal(jac, e["region"])
    bound = ra.region_limits(case.iw, case.ih)["slow_bound"]
    print(case.name, f"{case.iw}x{case.ih}", "jacobi rounds", rounds, "launches", (rounds + 1) // 2, "bound", bound, "undecided", e["undecided"])
    assert (rounds + 1) // 2 < bound
    assert (e["region"] >= 0).all()
    if case.stage == 0:
        assert e["needed"] == case.expect.get("needed", e["needed"])
        assert e["budget"] <= LIM["max_launches"]
    lo, hi = e["undecided"]
    if "undecided" in case.expect:
        assert lo == hi == case.expect["undecided"]
    if "seed_reaches" in case.expect:
        region0 = e["region0"]
        seed = int(np.flatnonzero(e["rsize"] == rc.SEED_SIZE)[0])
        small = e["rsize"][region0] <= LIM["thre"]
        assert int(small.sum()) >= case.expect["seed_reaches"] and (e["region"][small] == seed).all()
    if case.stage == 1:
        reccap = ra.region_limits(case.iw, case.ih)["reccap"]
        if case.expect["status0"] == 0:
            assert hi <= reccap      # the fast path has room for every undecided pixel
        elif "sweeps" not in case.expect:
            assert lo > reccap       # it has not


@pytest.mark.parametrize("kind", ("row", "last", "col", "diag", "anti"))
def test_chain_lengths_against_the_halo(kind):
    """chains up to AB_HK + 1 links that start beside a tile edge are decided by the tile kernel whichever side they start on; the long ones are not"""
    hk = LIM["AB_HK"]
    for c in STAGE1:
        if c.name.startswith(f"chain_{kind}_"):
            length = c.expect["seed_reaches"]
            lo, hi = rc.expected(c)["undecided"]
            if length <= hk + 1:
                assert (lo, hi) == (0, 0), c.name
            else:
                assert 0 < lo <= hi < length, c.name


def test_undecided_counts_sit_on_every_edge():
    nt, cap = LIM["AT_NT"], LIM["AT_CAP"]
    counts = rc._undecided_counts()
    for edge in [nt] + [e * nt for e in LIM["EPT"][:-1]] + [cap]:
        assert {edge - 1, edge, edge + 1} <= set(counts)
    for n in counts:
        c = rc.BY_NAME[f"undecided_{n}"]
        assert ra.region_limits(c.iw, c.ih)["reccap"] >= min(n, cap) and c.iw == LIM["absorb_tile"][0]


def test_all_small_counts():
    got = {c.name: rc.expected(c)["undecided"][0] for c in STAGE1 if c.name.startswith("all_small")}
    assert got["all_small_128x128"] == 16378 > 128 * 128 // 4 and got["all_small_64x64"] == 4090 > 64 * 64 // 4


def test_ties_cover_the_scan_order():
    """first maxima: between them the tie planes hold, for every position but the last, a pixel where that position wins a tie, and for every position but the first one
    where it loses one; the Python restatement that finds them equals the oracle"""
    wins, loses = set(), set()
    for c in STAGE1:
        if c.name.startswith("ties"):
            res, ties = rc.absorb_with_ties(*c.planes)
            assert np.array_equal(res.reshape(-1), rc.expected(c)["region"])
            for pos in ties.values():
                wins.add(pos[0])
                loses.update(pos[1:])
    assert wins == set(range(8)) and loses == set(range(1, 9))


def test_threshold_claim():
    c = rc.BY_NAME["threshold"]
    region = rc.expected(c)["region"].reshape(c.ih, c.iw)
    assert (region[4:8, 4:8] == rc.BG).all() and (region[4:8, 16:20] == 6).all()


def test_zigzag_is_longer_than_the_sweeps_reach():
    c = rc.BY_NAME["zigzag_sweeps"]
    lo, hi = rc.expected(c)["undecided"]
    reach = LIM["AT_SWEEPS"] * rc.sweep_steps(c.iw, c.ih)
    assert lo >= 2 * reach - LIM["absorb_tile"][1] and hi <= LIM["AT_CAP"] and hi <= ra.region_limits(c.iw, c.ih)["reccap"]
