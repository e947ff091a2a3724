"""Rectified patches, the host side (no GPU): the new entry points exist; rd_rectify_coefficients, rd_rect_quads and rd_rect_aspect agree in every bit with the
numpy restatement of the header's contract (tests/rectify.py) on every rectangle the reference left in tests/golden; validity; bad arguments."""
import ctypes
import glob
import os

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers
from tests import rectify

SYMBOLS = ("rd_rect_quads", "rd_rect_aspect", "rd_rectify_coefficients", "rd_rectifier_create", "rd_rectifier_destroy", "rd_rectifier_enqueue",
           "rd_rectifier_wait", "rd_detector_rectify_polled")


def golden_rects():
    """every rectangle list of tests/golden/rect_*.npz and hard_rect.npz"""
    out = []
    for path in sorted(glob.glob(os.path.join(helpers.GOLDEN, "rect_*.npz"))) + [os.path.join(helpers.GOLDEN, "hard_rect.npz")]:
        with np.load(path, allow_pickle=False) as g:
            out += [g[k] for k in g.files if k.endswith("_rects")]
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_exist_in_library_and_module():
    L = ra.lib()
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    for name in ("rect_quads", "rect_aspect", "rectify_coefficients", "Rectifier"):
        assert hasattr(ra, name)
    assert hasattr(ra.Detector, "rectify_polled") and hasattr(ra.PolylineDetector, "rectify_polled")
    assert all(hasattr(ra.Rectifier, m) for m in ("enqueue", "wait", "close", "rectify"))


def test_rect_quads_is_the_stated_permutation():
    lists = [r for r in golden_rects() if len(r)]
    assert lists
    for r in lists:
        q = ra.rect_quads(r)
        assert q.shape == (len(r), 4, 2)
        for k, src in enumerate((0, 3, 2, 1)):
            assert np.array_equal(bits(q[:, k, :]), bits(r["c2"][:, src, :]))
        assert np.array_equal(bits(q), bits(rectify.rect_quads(r)))
    assert ra.rect_quads(lists[0][:0]).shape == (0, 4, 2)


def test_coefficients_match_numpy_bit_for_bit_on_every_golden_rectangle():
    n = 0
    for r in golden_rects():
        for q in ra.rect_quads(r):
            got, st = ra.rectify_coefficients(q)
            want, wst = rectify.coefficients(q)
            assert st == wst == 1, "the reference's rectangles are strictly convex"
            assert np.array_equal(bits(got), bits(want)), (q, got, want)
            n += 1
    assert n > 100


def test_golden_rectangles_run_counter_clockwise_on_screen():
    """what rd_rect_quads' order rests on: with y down every cross product of c2 is negative, so c2[0], c2[3], c2[2], c2[1] runs clockwise"""
    for r in golden_rects():
        c = r["c2"]
        for i in range(4):
            u, v = c[:, (i + 1) % 4] - c[:, i], c[:, (i + 2) % 4] - c[:, (i + 1) % 4]
            assert (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0] < 0).all()


CONVEX = [(10.0, 20.0), (90.5, 25.0), (100.0, 80.25), (5.0, 70.0)]
INVALID = {
    "repeated corner": [(10, 20), (10, 20), (100, 80), (5, 70)],
    "repeated opposite corner": [(10, 20), (90, 25), (10, 20), (5, 70)],
    "three collinear corners": [(0, 0), (50, 0), (100, 0), (50, 60)],
    "bow-tie": [(10, 20), (100, 80), (90, 25), (5, 70)],
    "concave": [(0, 0), (100, 0), (20, 20), (0, 100)],
    "nan": [(10, 20), (float("nan"), 25), (100, 80), (5, 70)],
    "inf": [(10, 20), (90, 25), (100, float("inf")), (5, 70)],
    "all equal": [(3, 3)] * 4,
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_quads_have_status_zero_and_zero_coefficients(name):
    for shift in range(4):      # whichever corner comes first
        q = np.roll(np.array(INVALID[name], np.float64), shift, axis=0)
        coef, st = ra.rectify_coefficients(q)
        assert st == 0 and not coef.any(), name
        assert rectify.coefficients(q)[1] == 0
        coef, st = ra.rectify_coefficients(q[::-1])
        assert st == 0 and not coef.any(), name


def test_convex_quad_is_valid_in_both_orientations_and_maps_corners_to_corners():
    for q in (np.array(CONVEX), np.array(CONVEX)[::-1], np.roll(np.array(CONVEX), 1, axis=0)):
        coef, st = ra.rectify_coefficients(q)
        want, wst = rectify.coefficients(q)
        assert st == wst == 1
        assert np.array_equal(bits(coef), bits(want))
        a, b, c, d, e, f, g, h = coef
        for (s, t), (x, y) in zip(((0, 0), (1, 0), (1, 1), (0, 1)), q):
            w = g * s + h * t + 1.0
            assert w > 0
            assert abs((a * s + b * t + c) / w - x) < 1e-9 and abs((d * s + e * t + f) / w - y) < 1e-9


def test_coefficients_that_overflow_are_invalid():
    q = np.array(CONVEX) * 1e200      # finite corners, cross products and coefficients are not
    coef, st = ra.rectify_coefficients(q)
    assert st == 0 and not coef.any()
    assert rectify.coefficients(q)[1] == 0


def test_rect_aspect_matches_numpy():
    n = 0
    for r in golden_rects():
        for k in range(len(r)):
            assert np.array_equal(bits(ra.rect_aspect(r[k])), bits(rectify.rect_aspect(r[k])))
            n += 1
    assert n > 100
    r = np.zeros(1, ra.RECT_DTYPE)
    r["c3"][0] = [(0, 0, 5), (3, 4, 5), (3, 4, 7), (0, 0, 7)]
    assert ra.rect_aspect(r[0]) == 2.5


def test_rectifier_create_refuses_bad_arguments():
    L = ra.lib()
    for args in ((0, 0, 64, 4, 2), (0, 64, 0, 4, 2), (0, 64, 64, 0, 2), (0, 64, 64, 4, 0), (0, -3, 64, 4, 2), (0, 64, 64, -1, 2), (-1, 64, 64, 4, 2),
                 (1 << 20, 64, 64, 4, 2), (0, 1 << 20, 64, 4, 2)):
        assert not L.rd_rectifier_create(*args), args
    L.rd_rectifier_destroy(None)      # (a no-op)


def test_restatement_gives_the_crop_for_an_axis_aligned_quad_at_pixel_pitch():
    """the restatement's own anchor: s = (i + 0.5) / 64 on a quad from x0 - 0.5 to x0 + 63.5 lands on pixel centres, where the blend is the pixel itself"""
    frame = np.random.default_rng(3).integers(0, 256, (217, 333, 3), dtype=np.uint8)
    for x0, y0 in ((37, 21), (0, 0), (333 - 64, 217 - 64)):
        a, b = (x0 - 0.5, y0 - 0.5), (x0 + 63.5, y0 + 63.5)
        got, st = rectify.patch(frame, [a, (b[0], a[1]), b, (a[0], b[1])], 64, 64)
        assert st == 1 and np.array_equal(got, frame[y0:y0 + 64, x0:x0 + 64])
        got, st = rectify.patch(frame, [a, (a[0], b[1]), b, (b[0], a[1])], 64, 64)
        assert st == 1 and np.array_equal(got.transpose(1, 0, 2), frame[y0:y0 + 64, x0:x0 + 64])
    got, st = rectify.patch(frame, [a, a, b, (a[0], b[1])], 8, 8)      # an invalid quad: zeros
    assert st == 0 and got.shape == (8, 8, 3) and not got.any()


def test_rdpatches_example_is_built():
    src = open(os.path.join(helpers.ROOT, "examples", "rdpatches.c")).read()
    assert "rd_rect_quads" in src and "rd_rectifier_enqueue" in src and "rd_rectifier_wait" in src
    assert os.access(os.path.join(helpers.ROOT, "examples", "rdpatches"), os.X_OK)


def test_rect_aspect_is_height_over_width_in_the_order_of_rect_quads():
    """c3[i] is the pose of c2[i], and a patch's columns run along c2[0] -> c2[3], its rows along c2[0] -> c2[1]: for a rectangle that faces the camera - its
    corners on screen a scaled copy of its corners in space - rd_rect_aspect is exactly the quad's 2-D height / width, not its reciprocal"""
    for w, h in ((4.0, 1.0), (1.0, 4.0), (3.0, 2.0)):
        r = np.zeros(1, ra.RECT_DTYPE)
        space = np.array([(0, 0, 8), (0, h, 8), (w, h, 8), (w, 0, 8)], np.float64)      # counter-clockwise on screen (y down), as the detector's
        r["c3"][0] = space
        r["c2"][0] = space[:, :2] * 32.0 + (100.0, 50.0)
        q = ra.rect_quads(r)[0]
        assert ra.rectify_coefficients(q)[1] == 1
        width, height = np.linalg.norm(q[1] - q[0]), np.linalg.norm(q[3] - q[0])      # s runs q0 -> q1, t runs q0 -> q3
        assert ra.rect_aspect(r[0]) == height / width == h / w


def test_rect_aspect_of_screen_like_golden_rectangles_sides_with_height_over_width():
    """the estimated pose is not the on-screen edge ratio (perspective, poor fits), but were the convention the other way round, most of the reference's
    screen-like rectangles (status bit 0) with a clearly oblong quad would lie nearer the quad's width / height than its height / width"""
    nearer = total = 0
    for r in golden_rects():
        q = ra.rect_quads(r)
        for k in range(len(r)):
            width, height = np.linalg.norm(q[k, 1] - q[k, 0]), np.linalg.norm(q[k, 3] - q[k, 0])
            if not (r[k]["status"] & 1) or abs(np.log(height / width)) < np.log(1.2):
                continue
            a = np.log(ra.rect_aspect(r[k]))
            total += 1
            nearer += abs(a - np.log(height / width)) < abs(a - np.log(width / height))
    assert total > 50 and nearer > total / 2, (nearer, total)
