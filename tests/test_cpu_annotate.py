"""CPU tests of annotated frames: the shared coverage test (rd_annot_covers: what the draw kernel evaluates per pixel) against the restatement of the contract's
DEFINITION (tests/annotate.py), the binning test (never misses a tile), and the host helpers that make primitives from the detector's lists.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import annotate
from tests import helpers

L = ra.lib


def golden(name):
    return np.load(os.path.join(helpers.GOLDEN, name + ".npz"), allow_pickle=False)


def one_prim(x0, y0, x1, y1, t):
    return annotate.prims([(x0, y0, x1, y1, 0, 0, 0, t)])


# ---------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_covers_equals_the_definition_exhaustively(t):
    """every endpoint pair in [-2, 6]^2 x [-2, 6]^2 over the 15 x 15 window of pixels [-5, 9]^2: 6561 primitives x 225 pixels per thickness"""
    covers = L().rd_annot_covers
    window = [(x, y) for y in range(-5, 10) for x in range(-5, 10)]
    p = one_prim(0, 0, 0, 0, t)
    ptr = p.ctypes.data
    tests = covered = 0
    for x0 in range(-2, 7):
        for y0 in range(-2, 7):
            for x1 in range(-2, 7):
                for y1 in range(-2, 7):
                    p[0] = (x0, y0, x1, y1, 0, 0, 0, t)
                    want = (annotate.owners(p, 15, 15, origin=(-5, -5)) >= 0).reshape(-1)
                    got = np.array([covers(ptr, x, y) for x, y in window], bool)
                    assert np.array_equal(got, want), ((x0, y0, x1, y1, t), got.reshape(15, 15).astype(int), want.reshape(15, 15).astype(int))
                    tests += 225
                    covered += int(want.sum())
    assert tests == 6561 * 225 and covered > 0


def test_owners_window_equals_the_scalar_definition():
    """the two forms of the restatement agree (numpy int64 rows against Python integers pixel by pixel), so that either may stand for the definition"""
    rng = np.random.default_rng(3)
    for _ in range(300):
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-6, 20, 4))
        t = int(rng.integers(1, 9))
        own = annotate.owners(one_prim(x0, y0, x1, y1, t), 24, 22, origin=(-4, -3))
        want = np.array([[annotate.covers(x0, y0, x1, y1, t, x, y) for x in range(-4, 20)] for y in range(-3, 19)])
        assert np.array_equal(own >= 0, want), (x0, y0, x1, y1, t)


def test_covers_at_the_largest_coordinates():
    """the overflow check: 20 000 primitives with coordinates up to +-1048575 (and the corners of the legal range) and t up to 255, probed on the line, at and
    just past the brush's two edges, before and behind the span and far away - against Python integers"""
    covers = L().rd_annot_covers
    rng = np.random.default_rng(17)
    lo_c, hi_c = annotate.COORD_MIN, annotate.COORD_MAX
    cases = [(lo_c, lo_c, hi_c, hi_c, 255), (hi_c, lo_c, lo_c, hi_c, 255), (lo_c, hi_c, hi_c, hi_c - 1, 1), (lo_c, lo_c, lo_c, hi_c, 254), (hi_c, hi_c, hi_c, hi_c, 255)]
    while len(cases) < 20000:
        span = int(rng.choice([8, 1000, 1048575]))
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-span, span + 1, 4))
        if rng.integers(0, 4) == 0:      # far-apart ends near the range's corners
            x0, y1 = int(rng.integers(lo_c, lo_c + 50)), int(rng.integers(hi_c - 50, hi_c + 1))
        cases.append((x0, y0, x1, y1, int(rng.integers(1, 256))))
    probes = hits = 0
    p = one_prim(0, 0, 0, 0, 1)
    for (x0, y0, x1, y1, t) in cases:
        p[0] = (x0, y0, x1, y1, 0, 0, 0, t)
        xmajor, ua, va, ub, vb = annotate._major(x0, y0, x1, y1)
        D, lo, hi = ub - ua, (t - 1) // 2, t // 2
        pts = []
        for u in {ua, ub, int(rng.integers(ua, ub + 1)), int(rng.integers(ua, ub + 1)), ua - 1, ub + 1}:
            uc = min(max(u, ua), ub)
            V = va if D == 0 else va + (2 * (uc - ua) * (vb - va) + D) // (2 * D)
            pts += [(u, V), (u, V - lo), (u, V - lo - 1), (u, V + hi), (u, V + hi + 1)]
        pts += [(int(rng.integers(0, 65536)), int(rng.integers(0, 65536))) for _ in range(3)] + [(lo_c, hi_c), (hi_c, lo_c), (65535, 65535), (0, 0)]
        for u, v in pts:
            x, y = (u, v) if xmajor else (v, u)
            want = annotate.covers(x0, y0, x1, y1, t, x, y)
            assert bool(covers(p.ctypes.data, x, y)) == want, ((x0, y0, x1, y1, t), (x, y), want)
            probes += 1
            hits += want
    print("probes %d, covered %d" % (probes, hits))
    assert hits > probes // 4 and probes - hits > probes // 4


def test_endpoint_order_does_not_matter():
    covers = L().rd_annot_covers
    rng = np.random.default_rng(5)
    for _ in range(400):
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-3, 12, 4))
        t = int(rng.integers(1, 6))
        a, b = one_prim(x0, y0, x1, y1, t), one_prim(x1, y1, x0, y0, t)
        for y in range(-6, 15):
            for x in range(-6, 15):
                assert covers(a.ctypes.data, x, y) == covers(b.ctypes.data, x, y)


# ---------------------------------------------------------------------------------------------- binning
def tiles_touched(p, iw, ih):
    lim = ra.annot_limits()
    tw, th = lim["tile_w"], lim["tile_h"]
    touches = L().rd_annot_touches
    return {(tx, ty) for ty in range((ih + th - 1) // th) for tx in range((iw + tw - 1) // tw)
            if touches(p.ctypes.data, tx * tw, ty * th, min(tx * tw + tw, iw) - 1, min(ty * th + th, ih) - 1)}, tw, th


def test_binning_never_misses_a_tile_and_keeps_a_diagonal_thin():
    rng = np.random.default_rng(23)
    iw, ih = 333, 217
    cases = [(0, 0, iw - 1, ih - 1, 1), (iw - 1, 0, 0, ih - 1, 7), (-500, -300, 900, 600, 255), (63, 0, 63, ih, 1), (64, 0, 64, ih, 2), (0, 31, iw, 31, 1), (0, 32, iw, 32, 3), (100, 100, 100, 100, 255)]
    cases += [tuple(int(v) for v in rng.integers(-100, 450, 4)) + (int(rng.choice([1, 2, 3, 8, 40])),) for _ in range(400)]
    extra = total = 0
    for c in cases:
        p = one_prim(*c)
        got, tw, th = tiles_touched(p, iw, ih)
        ys, xs = np.nonzero(annotate.owners(p, iw, ih) >= 0)
        need = set(zip((xs // tw).tolist(), (ys // th).tolist()))
        assert need <= got, (c, sorted(need - got))
        extra += len(got - need)
        total += len(got)
    print("tiles handed a primitive: %d, of which the primitive covers no pixel in %d" % (total, extra))
    assert extra <= total // 3      # (the test may over-include; it must stay a band test, not the bounding box)
    # the frame diagonal of a 1920 x 1080 frame: the tiles it crosses, not all of them
    got, tw, th = tiles_touched(one_prim(0, 0, 1919, 1079, 2), 1920, 1080)
    ntiles = ((1920 + tw - 1) // tw) * ((1080 + th - 1) // th)
    print("frame diagonal: %d of %d tiles" % (len(got), ntiles))
    assert len(got) <= 1920 // tw + 1080 // th + 8 and len(got) * 8 < ntiles


# ---------------------------------------------------------------------------------------------- primitives from rectangles
def assert_prims_equal(got, want, what=""):
    assert got.dtype == ra.PRIM_DTYPE and len(got) == len(want), (what, len(got), len(want))
    assert got.tobytes() == want.tobytes(), (what, [k for k in range(len(got)) if got[k] != want[k]][:5])


@pytest.mark.parametrize("name", ["rect_640x480_s0", "rect_1920x1080_s0"])
def test_rects_on_the_golden_lists(name):
    rects = golden(name)["f0_rects"]
    assert len(rects) > 0
    for scale in (1, 2):
        got = ra.annot_rects(rects, scale=scale)
        assert_prims_equal(got, annotate.rects_prims(rects, scale), "%s scale %d" % (name, scale))
        assert len(got) == 6 * len(rects)
    k = ra.annot_rects(rects)
    r0 = rects[0]
    assert (k[0]["x0"], k[0]["y0"], k[0]["x1"], k[0]["y1"]) == (int(r0["c2"][0][0]), int(r0["c2"][0][1]), int(r0["c2"][1][0]), int(r0["c2"][1][1]))
    assert (k[4]["x1"], k[4]["y1"]) == (int(r0["c2"][2][0]), int(r0["c2"][2][1])) and (k[5]["x0"], k[5]["y0"]) == (int(r0["c2"][1][0]), int(r0["c2"][1][1]))
    assert k[4]["thickness"] == 1 and k[5]["thickness"] == 1


def crafted_rects():
    r = np.zeros(10, ra.RECT_DTYPE)
    base = np.array([(10.9, 20.2), (10.1, 80.7), (90.5, 81.99), (91.0, 19.5)])
    for k in range(len(r)):
        r[k]["c2"] = base + 7 * k
        r[k]["status"] = k % 4
    r[1]["c2"] = [(-0.9, -1.5), (-7.99, 30.2), (40.5, 33.0), (41.0, -0.2)]      # truncation toward zero: -0.9 -> 0, -1.5 -> -1, -7.99 -> -7
    r[4]["c2"][2][0] = np.nan
    r[5]["c2"][0][1] = np.inf
    r[6]["c2"][3][0] = -np.inf
    r[7]["c2"][1][1] = 1e9
    r[8]["c2"] = [(-1048576.9, 5.0), (3.0, 1048575.9), (9.0, 9.0), (4.0, -3.0)]      # still inside after truncation
    r[9]["c2"][0][0] = 1048576.0      # just outside
    return r


def test_rects_on_crafted_lists():
    r = crafted_rects()
    got = ra.annot_rects(r)
    assert_prims_equal(got, annotate.rects_prims(r), "crafted")
    assert len(got) == 6 * 5      # 4, 5, 6, 7 and 9 are skipped as a whole
    assert (got[6]["x0"], got[6]["y0"], got[6]["x1"], got[6]["y1"]) == (0, -1, -7, 30)
    assert (got[24]["x0"], got[24]["y0"], got[24]["y1"]) == (-1048576, 5, 1048575)
    # vidrect.cpp's table: status -> b, g, r, thickness of the edges; diagonals 1
    table = {0: (0, 255, 0, 1), 1: (0, 200, 255, 2), 2: (255, 0, 0, 1), 3: (0, 0, 255, 2)}
    for k, status in enumerate((0, 1, 2, 3, 0)):
        for e in range(6):
            p = got[6 * k + e]
            assert (p["b"], p["g"], p["r"]) == table[status][:3] and p["thickness"] == (table[status][3] if e < 4 else 1)
    style = np.array([(1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 200), (13, 14, 15, 255)], np.uint8)
    for scale in (1, 2):
        got = ra.annot_rects(r, scale=scale, style=style)
        assert_prims_equal(got, annotate.rects_prims(r, scale, style), "crafted, custom style, scale %d" % scale)
    assert got[0]["thickness"] == 8 and got[4]["thickness"] == 2 and got[12]["thickness"] == 255      # doubled, capped
    assert (got[0]["x0"], got[0]["y0"]) == (int(10.9 * 2.0 + 0.5), int(20.2 * 2.0 + 0.5))
    assert (got[6]["x0"], got[6]["y0"]) == (int(-0.9 * 2.0 + 0.5), int(-1.5 * 2.0 + 0.5)) == (-1, -2)
    assert len(ra.annot_rects(r[:0])) == 0
    status9 = r[:1].copy()
    status9["status"] = 9
    assert len(ra.annot_rects(status9)) == 0


# ---------------------------------------------------------------------------------------------- primitives from segment lists
@pytest.mark.parametrize("name", ["poly_640x480_s0", "poly_1280x720_s1_vid"])
def test_segments_on_the_golden_lists(name):
    segs = golden(name)["segments"]
    n = int(segs.view("<i4")[0])
    assert n == len(segs) - 1 and n > 20
    for scale in (1, 2):
        allp = ra.annot_segments(segs, ra.ANNOT_SEG_ALL, scale)
        assert_prims_equal(allp, annotate.segments_prims(segs, ra.ANNOT_SEG_ALL, scale), name + " all")
        assert len(allp) == n and (allp["thickness"] == scale).all() and (allp["b"] == 255).all() and (allp["r"] == 255).all()
        chains = ra.annot_segments(segs, ra.ANNOT_SEG_CHAINS, scale)
        assert_prims_equal(chains, annotate.segments_prims(segs, ra.ANNOT_SEG_CHAINS, scale), name + " chains")
        assert 0 < len(chains) <= n and set(chains["r"].tolist()) == {100, 255}


def crafted_segments():
    s = np.zeros(9, ra.LS_DTYPE)
    s.view("<i4")[0] = 8
    for k in range(1, 9):
        s[k]["x0"], s[k]["y0"], s[k]["x1"], s[k]["y1"] = 10.7 * k, 3.2 * k, 10.7 * k + 20.9, 3.2 * k - 5.5
        s[k]["polyid"] = 1
        s[k]["leftPtr"] = -1
        s[k]["rightPtr"] = -1
    # chain 1 -> 2 -> 3 -> 2 ...: a cycle, walked for n = 8 steps; 4: a lone head; 5: not a head (leftPtr > 0); 6: polyid 0; 7 -> 8, 8 out of range and then a link beyond n
    s[1]["rightPtr"], s[2]["rightPtr"], s[3]["rightPtr"] = 2, 3, 2
    s[2]["leftPtr"], s[3]["leftPtr"] = 1, 2
    s[5]["leftPtr"] = 4
    s[6]["polyid"] = 0
    s[7]["rightPtr"], s[8]["leftPtr"], s[8]["rightPtr"] = 8, 7, 99
    s[8]["x1"] = 3e6
    s[4]["x0"] = -2.75
    return s


def test_segments_on_crafted_lists():
    s = crafted_segments()
    for scale in (1, 2):
        for mode in (ra.ANNOT_SEG_ALL, ra.ANNOT_SEG_CHAINS):
            assert_prims_equal(ra.annot_segments(s, mode, scale), annotate.segments_prims(s, mode, scale), "mode %d scale %d" % (mode, scale))
    allp = ra.annot_segments(s, ra.ANNOT_SEG_ALL)
    assert len(allp) == 7      # record 8 is out of range
    assert allp[3]["x0"] == -2 and ra.annot_segments(s, ra.ANNOT_SEG_ALL, 2)[3]["x0"] == int(-2.75 * 2.0 + 0.5) == -5
    chains = ra.annot_segments(s, ra.ANNOT_SEG_CHAINS)
    assert len(chains) == 8 + 1 + 1      # the cycle's 8 steps, record 4, record 7 (8 is skipped, 99 ends the chain)
    assert [(int(p["b"]), int(p["r"])) for p in chains[:4]] == [(255, 100), (100, 255), (255, 100), (100, 255)]
    # a max smaller than the count: the count is returned, max primitives are written and nothing behind them
    out = np.zeros(5, ra.PRIM_DTYPE)
    out[3:] = (7, 7, 7, 7, 7, 7, 7, 7)
    n = L().rd_annot_segments(s.ctypes.data, ra.ANNOT_SEG_CHAINS, 1, out.ctypes.data, 3)
    assert n == 10 and out[:3].tobytes() == chains[:3].tobytes() and (out[3:]["x0"] == 7).all()
    assert len(ra.annot_segments(s, ra.ANNOT_SEG_CHAINS, max_prims=4)) == 4
    assert L().rd_annot_segments(s.ctypes.data, 2, 1, out.ctypes.data, 3) == 0      # unknown mode


# ---------------------------------------------------------------------------------------------- colour, limits
def test_yuv_against_the_formula():
    vals = sorted(set(range(0, 256, 5)) | {255})
    out = (ctypes.c_uint8 * 3)()
    fn = L().rd_annot_yuv
    b, g, r = (a.reshape(-1) for a in np.meshgrid(vals, vals, vals, indexing="ij"))
    Y, U, V = annotate.yuv(b, g, r)
    assert Y.min() >= 16 and Y.max() <= 235 and U.min() >= 16 and U.max() <= 240 and V.min() >= 16 and V.max() <= 240
    for k in range(len(b)):
        fn(int(b[k]), int(g[k]), int(r[k]), out)
        assert (out[0], out[1], out[2]) == (Y[k], U[k], V[k]), (b[k], g[k], r[k])
    fn(0, 0, 0, out)
    assert tuple(out) == (16, 128, 128)
    fn(255, 255, 255, out)
    assert tuple(out) == (235, 128, 128)


def test_limits():
    out = np.full(4, -1, np.int32)
    L().rd_annot_limits(out.ctypes.data)
    tw, th, chunk, zero = (int(v) for v in out)
    assert tw > 0 and th > 0 and tw % 2 == 0 and th % 2 == 0 and chunk >= 1 and zero == 0
    assert ra.annot_limits() == {"tile_w": tw, "tile_h": th, "chunk": chunk}
