"""The device post-process (rd_k_post.hip: k_post_candidates, k_post_solve, k_post_header) on the crafted inputs of tests/postcases.py, through its test tap
rd_postprocess_planes_device: every case that fits the device's fixed capacities gives the host post-process's list in bits and in order (which
tests/test_cpu_postcases.py holds to the reference's own compiled host code), every case one past a capacity is flagged and leaves nothing behind that a
later frame trips over, and in the product such a frame is handed to the host path and counted.  The capacities come from rd_post_device_limits."""
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers, postcases as pc

pytestmark = pytest.mark.gpu

FITS = [(fn, {}) for fn in pc.VALUE_CASES] + [(fn, kw) for fn, kw, fits in pc.CAPACITY_CASES if fits]
OVER = [(fn, kw) for fn, kw, fits in pc.CAPACITY_CASES if not fits]
_host = {}


def ids(cases):
    return [pc.case_id(fn, kw) for fn, kw in cases]


def host_list(fn, kw=None, tan=None):
    c = pc.get(fn, kw)
    tan = c.tan_aov if tan is None else tan
    key = (pc.case_id(fn, kw or {}), tan)
    if key not in _host:
        _host[key] = ra.postprocess_planes(*c.planes(), tan)
    return _host[key]


def device_list(fn, kw=None, tan=None):
    c = pc.get(fn, kw)
    return ra.postprocess_planes_device(*c.planes(), c.tan_aov if tan is None else tan)


def quads_are_exact():
    rects, info = device_list(pc.quads)
    return rects is not None and info[1] == 0 and info[0] == pc.candidate_count(pc.get(pc.quads)) and helpers.rects_equal(rects, host_list(pc.quads))


@pytest.mark.parametrize("fn,kw", FITS, ids=ids(FITS))
def test_case_that_fits_equals_the_host_postprocess(fn, kw):
    c = pc.get(fn, kw)
    rects, info = device_list(fn, kw)
    want = host_list(fn, kw)
    print("%s: %d segments, %d candidates counted (%d expected), overflow word %d, %d rectangles (host %d)" % (
        pc.case_id(fn, kw), int(c.segs.view("i4")[0]), info[0], pc.candidate_count(c), info[1], -1 if rects is None else len(rects), len(want)))
    assert info[1] == 0 and rects is not None
    assert info[0] == pc.candidate_count(c)
    assert helpers.rects_equal(rects, want)
    assert len(want) >= c.meta["min_valid"]


@pytest.mark.parametrize("fn,kw", OVER, ids=ids(OVER))
def test_case_past_a_limit_is_flagged_and_leaves_nothing_behind(fn, kw):
    rects, info = device_list(fn, kw)
    print("%s: overflow word %d, candidates counted %d" % (pc.case_id(fn, kw), info[1], info[0]))
    assert rects is None and info[1] != 0
    assert quads_are_exact(), "the call after an overflowed one"


@pytest.mark.parametrize("fn,kw", pc.HULL_CASES, ids=ids(pc.HULL_CASES))
def test_hull_deep_is_exact_or_flagged(fn, kw):
    """hull_deep with 44 segments nests just below the hull's stack, with 50 past it; hull_pool fills the index lists of the hull's pending calls at a quarter
    of that depth (tests/test_cpu_postcases.py asserts from the end points which bound each reaches).  Exact or flagged, and the call after it is exact."""
    rects, info = device_list(fn, kw)
    want = host_list(fn, kw)
    print("%s: %s" % (pc.case_id(fn, kw), "overflow flagged (word %d)" % info[1] if rects is None else "fits: %d rectangles (host %d)" % (len(rects), len(want))))
    if rects is None:
        assert info[1] != 0
    else:
        assert info[1] == 0 and info[0] == pc.candidate_count(pc.get(fn, kw)) and helpers.rects_equal(rects, want)
    assert len(want) >= 10 and quads_are_exact()


@pytest.mark.parametrize("fn", [pc.quads, pc.chains, pc.branches], ids=lambda f: f.__name__)
def test_two_apertures_on_the_same_case(fn):
    for tan in (pc.TAN36, pc.TAN25, pc.TAN36):
        rects, info = device_list(fn, None, tan)
        assert info[1] == 0 and helpers.rects_equal(rects, host_list(fn, None, tan)), tan
    assert not helpers.rects_equal(host_list(fn, None, pc.TAN36), host_list(fn, None, pc.TAN25))


def test_frame_past_the_candidate_capacity_is_handed_to_the_host_path(monkeypatch):
    """In the product: a still whose polyline heads alone exceed POST_MAXC goes through a detector with the device post-process.  Its list is the default
    (host) detector's, counter 12 (host post-process) counts it and counter 11 does not, and the ordinary frame after it comes from the device again."""
    lim = ra.post_device_limits()
    iw, ih = 1280, 720
    busy, plain = synth.hard_frame("tiles", 5, iw, ih), synth.frame(synth.SEED0 + 31, iw, ih, 0)
    orc = helpers.OracleRect(iw, ih)
    orc.frame(busy)
    osegs = orc.segments()
    orc.close()
    v = osegs[1:]
    heads = int(((v["polyid"] != 0) & (v["leftPtr"] <= 0)).sum())
    assert heads > lim["POST_MAXC"], heads
    out = {}
    for mode in ("default", "1"):
        monkeypatch.delenv("RD_DEVICE_POST", raising=False) if mode == "default" else monkeypatch.setenv("RD_DEVICE_POST", mode)
        det = ra.Detector(iw, ih, nslots=1, aperture=pc.TAN36)
        res, counts = [], []
        for f in (busy, plain):
            det.enqueue(f)
            res.append((det.poll(pc.TAN36), det.last_segments()))
            counts.append((ra.lib().rd_detector_counter(det.h, 11), ra.lib().rd_detector_counter(det.h, 12)))
        det.close()
        out[mode] = (res, counts)
    (host, hc), (dev, dc) = out["default"], out["1"]
    print("busy still: %d polyline heads (capacity %d), %d rectangles; counters (device, host) after each frame: default detector %s, device detector %s" % (
        heads, lim["POST_MAXC"], len(dev[0][0]), hc, dc))
    v = dev[0][1][1:]
    assert int(((v["polyid"] != 0) & (v["leftPtr"] <= 0)).sum()) > lim["POST_MAXC"]      # (the detector's own list of the still)
    for t in range(2):
        assert helpers.rects_equal(host[t][0], dev[t][0]) and helpers.segments_equal(host[t][1], dev[t][1]), t
    assert dc == [(0, 1), (1, 1)]
