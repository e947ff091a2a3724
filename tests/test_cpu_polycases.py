"""What tests/test_gpu_polycases.py relies on, asserted from rdo_polyline alone (no GPU): every claim of every crafted mask in tests/polycases.py - the
orphan records of the tie fixtures and what the join's old round schedule makes of them, the counts that put a mask on a capacity of the single-block
kernel (taken from rd_polyline_limits, not copied) - and the restated join itself."""
import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers, polycases as pc

CASES = pc.all_cases()


def test_limits():
    lim = ra.polyline_limits()
    assert lim["PP_LIVE"] > 0 and lim["PP_MAXCAND"] > 0 and 4 <= lim["PP_MAXSEG"] <= 1 << lim["PP_ID_BITS"]
    # the masks of the capacity cases stay small: about 1100 x 300 at the most
    for c in pc.capacity_cases():
        ih, iw = pc.resolve(c)[0].shape
        assert iw <= 1100 and ih <= 300, c.name


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_claims(case):
    f = pc.facts(case)
    print(case.name, pc.resolve(case)[0].shape, {k: v for k, v in f.items() if k != "orphans"}, f.get("orphans"))
    for k, v in case.claims.items():
        assert f[k] == v, (case.name, k, f[k], v)


@pytest.mark.parametrize("case", [c for c in CASES if c.tie], ids=repr)
def test_tie_fixture_holds_an_orphan(case):
    """a valid record with rightPtr != 0 whose right neighbour's leftPtr is another record; the serial join restated in Python (float32 step by step) is the
    oracle's list bit for bit, so what old_schedule_join differs from is the join and not the restatement"""
    _, _, (ls, _, info) = pc.resolve(case)
    orph = pc.orphans(ls)
    assert orph
    for o, h, t in orph:
        assert ls["polyid"][o] != 0 and ls["rightPtr"][o] == h != 0 and ls["leftPtr"][h] == t != o
    assert pc.serial_join(info["before_join"])[1:].tobytes() == ls[1:].tobytes()


def test_tie_kinds_are_all_there():
    kinds = {k for k, seeds in pc.TIE_SEEDS.items() if seeds}
    assert kinds == {"sibling_left_of_h", "sibling_split_again", "benign", "across64"}


def test_restated_join_on_plain_lists():
    """without an orphan the old schedule, the serial join and the oracle agree (the schedule was right for clean chains)"""
    for c in CASES:
        if c.name.startswith(("minerror_", "size_", "frame_chain")):
            _, _, (ls, _, info) = pc.resolve(c)
            assert not pc.orphans(ls), c.name
            assert helpers.segments_equal(pc.serial_join(info["before_join"]), ls), c.name
            assert helpers.segments_equal(pc.old_schedule_join(info["before_join"])[0], ls), c.name


def test_value_cases_say_what_they_mean():
    by = {c.name: pc.facts(c) for c in pc.value_cases()}
    n = [by["minerror_%g" % m]["header"] for m in (0.5, 1.0, 2.5, 4.0)]
    assert n[0] > n[1] > n[2] > n[3] > 0, n                                  # the threshold matters on this mask
    a, b = (pc.resolve(c)[2] for c in pc.value_cases() if c.name.startswith("frame_chain"))
    assert not helpers.segments_equal(a[0], b[0]) or not np.array_equal(a[1], b[1])      # and so does the ring's value
    assert by["size_thre_edge"]["mask_pixels"] == sum(k for _, k in pc.SIZE_THRE_LINES)


def test_short_lists_drop_records():
    """the list cases: one record short drops exactly the last record and keeps counting ids in the header, as FITS (pl:456, pl:589) has it"""
    by = {c.name: c for c in pc.capacity_cases()}
    full = pc.resolve(by["list_fits"])[2][0]
    short = pc.resolve(by["list_one_short"])[2][0]
    assert len(full) == len(short) == 46 and int(short.view("i4")[0]) > 45
    assert short["polyid"][45] == 0 and full["polyid"][45] != 0
