"""The crafted inputs of tests/postcases.py through the host post-process (csrc/rd_post.c + rd_post_core.h: rd_postprocess_planes) against THE REFERENCE'S OWN
compiled executeCPUTask (oclrect.c:1049-1226) on the same planes: every list equal in bits and in order.  The reference's lists are recorded in
tests/golden/postcases_ref.npz (tools/make_golden_postcases.py) with the CRCs of the planes it was given; where oracle/_ref is built the reference runs again
and must reproduce them.  That makes the reference the truth for these inputs; tests/test_gpu_post_device.py then holds the device post-process to the host's lists."""
import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers, postcases as pc

IDS = [pc.case_id(fn, kw) for fn, kw in pc.ALL_CASES]
APERTURES = (("a36", pc.TAN36), ("a25", pc.TAN25))


@pytest.fixture(scope="module")
def golden():
    return np.load(helpers.GOLDEN + "/postcases_ref.npz")


@pytest.mark.parametrize("fn,kw", pc.ALL_CASES, ids=IDS)
def test_host_postprocess_equals_the_reference_on_crafted_case(fn, kw, golden):
    c = pc.get(fn, kw)
    key = pc.case_id(fn, kw)
    assert pc.planes_crc(c) == [int(v) for v in golden[key + "_planes_crc"]], "not the planes the reference was given (tools/make_golden_postcases.py)"
    assert pc.candidate_count(c) < 4096       # (helpers.RefRect.host_postprocess returns at most 4096 records: one per candidate and the header)
    for name, tan in APERTURES:
        theirs = golden[key + "_" + name + "_rects"]
        mine = ra.postprocess_planes(*c.planes(), tan)
        assert helpers.rects_equal(mine, theirs), (key, name, len(mine), len(theirs))
    theirs = golden[key + "_a36_rects"]
    assert len(theirs) >= c.meta["min_valid"], (key, len(theirs))
    assert int(((theirs["status"] & 2) != 0).sum()) >= c.meta.get("min_status2", 0)


@pytest.fixture(scope="module")
def reference():
    """one instance of the reference per frame size, shared by the cases"""
    open_ = {}

    def get(iw, ih):
        if (iw, ih) not in open_:
            open_[(iw, ih)] = helpers.RefRect(iw, ih)
        return open_[(iw, ih)]

    yield get
    for r in open_.values():
        r.close()


@pytest.mark.ref
@pytest.mark.parametrize("fn,kw", pc.ALL_CASES, ids=IDS)
def test_recorded_lists_are_what_the_reference_returns(fn, kw, golden, reference):
    c = pc.get(fn, kw)
    key = pc.case_id(fn, kw)
    r = reference(c.iw, c.ih)
    for name, tan in APERTURES:
        assert helpers.rects_equal(r.host_postprocess(c.segs, c.boundary, c.table, tan), golden[key + "_" + name + "_rects"]), (key, name)


def test_bucket_order_case_separates_the_rankings(golden):
    """The reference's list for `bucket_order` comes in (bucket of the id, first insertion) order, and that order differs from every ranking that forgets a part
    of it: by id, by first insertion alone, by (bucket, id), and by a bucket that leaves out the id's bits 10-19 or its bits from 20 up."""
    c = pc.get(pc.bucket_order)
    ids, cells = c.meta["ids"], c.meta["cells"]
    rects = golden["bucket_order_a36_rects"]
    assert len(rects) == len(ids)          # every quad is in the list, so the list's order is an order of all ids
    centres = rects["c2"].mean(axis=1)
    order = [int(np.argmin([(cx - x) ** 2 + (cy - y) ** 2 for cx, cy, _ in cells])) for x, y in centres]      # quad q = cell q = insertion rank q
    assert sorted(order) == list(range(len(ids)))
    quads = list(range(len(ids)))
    assert order == sorted(quads, key=lambda q: (pc.am_bucket(ids[q]), q))
    assert order != sorted(quads, key=lambda q: ids[q])
    assert order != quads
    assert order != sorted(quads, key=lambda q: (pc.am_bucket(ids[q]), ids[q]))
    assert order != sorted(quads, key=lambda q: ((ids[q] ^ (ids[q] >> 20)) & 1023, q))
    assert order != sorted(quads, key=lambda q: ((ids[q] ^ (ids[q] >> 10)) & 1023, q))
    buckets = [pc.am_bucket(v) for v in ids]
    assert max(buckets.count(b) for b in set(buckets)) >= 4 and max(ids) >= 1 << 20
    low = {}
    for v in ids:
        low.setdefault(v & 1023, []).append(v)
    assert any(sum(1 for w in vs if w >> 20 == 0) >= 3 for vs in low.values())                                 # differ only in bits 10-19
    assert any(len({(w >> 10) & 1023 for w in vs if w >> 20}) == 1 and sum(1 for w in vs if w >> 20) >= 3 for vs in low.values())      # differ only from bit 20 up


def test_capacity_cases_sit_on_the_limits():
    """what the device test relies on: the counts of each capacity case against rd_post_device_limits, from the case's own planes"""
    lim = ra.post_device_limits()
    for over in (False, True):
        c = pc.get(pc.maxc_chains, {"over": over})
        assert pc.candidate_count(c) == lim["POST_MAXC"] + over and not pc.memberships(c)
        c = pc.get(pc.maxc_mixed, {"over": over})
        assert pc.candidate_count(c) == lim["POST_MAXC"] + over and sum(len(m) >= 4 for m in pc.memberships(c).values()) == 10
        c = pc.get(pc.cap_members_per_candidate, {"over": over})
        assert max(len(m) for m in pc.memberships(c).values()) == lim["POST_CAP"] + over
        c = pc.get(pc.ht, {"over": over})
        m = pc.memberships(c)
        assert len(m) == lim["POST_HT"] + over and sum(len(v) >= 4 for v in m.values()) == 10
        c = pc.get(pc.members_total, {"over": over})
        m = pc.memberships(c)
        assert sum(len(v) for v in m.values() if len(v) >= 4) == lim["POST_MEMBERS"] + over and pc.candidate_count(c) <= lim["POST_MAXC"]
        c = pc.get(pc.maxg, {"over": over})
        ng = sum(len(v) >= 4 for v in pc.memberships(c).values())
        assert ng > lim["POST_MAXG"] if over else lim["POST_MAXC"] < ng < lim["POST_MAXG"]
    assert pc.candidate_count(pc.get(pc.waves, {"factor": 1})) == lim["POST_WAVES"] + 1
    assert pc.candidate_count(pc.get(pc.waves, {"factor": 3})) == 3 * lim["POST_WAVES"]


def test_hull_cases_reach_the_bound_they_are_named_for():
    """From the end points of each hull case alone (postcases.hull_nesting: the quick hull's nesting in doubles, with the device's accounting of its pending
    calls): 44 segments of hull_deep fit both bounds, 50 run out of pending calls (RDP_HULL_DEPTH) with the index lists far from full, and hull_pool fills
    the index lists (RDP_HULL_POOL = 16 * POST_CAP) at a nesting far from RDP_HULL_DEPTH.  Neither is bounded on the host: the recorded lists are the
    reference's, which has no such bounds."""
    lim = ra.post_device_limits()
    cap, pool, depth = lim["POST_CAP"], lim["RDP_HULL_POOL"], lim["RDP_HULL_DEPTH"]
    assert pool == 16 * cap
    got = {pc.case_id(fn, kw): pc.hull_nesting(pc.get(fn, kw), cap, pool, depth) for fn, kw in pc.HULL_CASES}
    print(got)
    what, deep, asked = got["hull_deep-nseg44"]
    assert what == "fits" and depth - 4 <= deep < depth and asked <= pool
    what, deep, asked = got["hull_deep-nseg50"]
    assert what == "depth" and deep == depth and asked < pool * 4 // 5
    what, deep, asked = got["hull_pool"]
    assert what == "pool" and asked > pool and deep < depth // 2
    for fn, kw in pc.HULL_CASES:      # without the bounds every one nests further still, and to the end
        c = pc.get(fn, kw)
        n = len(c.meta["hull_segments"])
        what, deeper, _ = pc.hull_nesting(c, n, 1 << 30, 1 << 30)
        assert what == "fits" and deeper >= got[pc.case_id(fn, kw)][1]
