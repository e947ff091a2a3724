"""The labelling tile kernel (k_label_tile, rectdetect_amd/csrc/rd_k_label.hip: 64 x 32 tiles, four waves, wave w owns the tile's rows 8w .. 8w + 7) at the
sizes where its strips and tiles end: the operator on crafted planes against the oracle's labelling, and the frame paths of both detector kinds - whose tile
kernels compute their pixel values themselves (edge tidy, region-boundary marks, the poly kind's mask) - against the oracle, frame by frame and in group
launches.  A labelling is unique (label = smallest pixel index of the 8-connected component of equal value, -1 for the background value), so every comparison
is np.array_equal.  What the crafted planes must contain for that to mean something is asserted on the CPU (test_fixtures_are_what_they_claim; it needs no GPU)."""
import functools
import os
import re

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
LT_W, LT_H, STRIP = 64, 32, 8      # the tile and a wave's strip of rows: LT_W, LT_H and LT_H / LT_TY of rd_k_label.hip - keep them equal
# (iw, ih): heights one short of / equal to / one over a strip (7 8 9) and a tile (31 32 33), widths 63 64 65, and several tiles both ways
SHAPES = [(63, 7), (64, 8), (65, 9), (63, 31), (64, 32), (65, 33), (129, 65)]
BIG = (129, 65)


def spiral(iw, ih):
    """one 1-pixel line from the corner inwards with 1-pixel gaps: a single component that winds through every strip and tile boundary (and so does the gap)"""
    m = np.zeros((ih, iw), np.int32)
    inb = lambda x, y: 0 <= x < iw and 0 <= y < ih
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 1
    while True:
        for _ in range(2):
            nx, ny, ax, ay = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if inb(nx, ny) and m[ny, nx] == 0 and (not inb(ax, ay) or m[ay, ax] == 0):
                x, y = nx, ny
                m[y, x] = 1
                break
            dx, dy = -dy, dx
        else:
            return m


def comb(iw, ih, period, join, blank):
    """teeth in every other column; per `period` rows they are joined by one full row `join` (mod period) and cut by one empty row `blank` (None: never cut)"""
    yy, xx = np.indices((ih, iw))
    m = ((xx & 1) == 0).astype(np.int32)
    m[yy % period == join] = 1
    if blank is not None:
        m[yy % period == blank] = 0
    return m


@functools.lru_cache(maxsize=None)
def planes(iw, ih):
    """name -> plane (read-only, made once per shape)"""
    rng = np.random.default_rng(1000 * iw + ih)
    yy, xx = np.indices((ih, iw))
    p = {
        "ones": np.ones((ih, iw), np.int32),
        "checkerboard": ((xx + yy) & 1).astype(np.int32),                      # each colour one component, connected diagonally only; every inner pixel issues two unions
        "vertical stripes": (xx & 1).astype(np.int32),                          # 64 runs per tile row
        "horizontal stripes": (yy & 1).astype(np.int32),
        "random 50%": (rng.random((ih, iw)) < 0.5).astype(np.int32),
        "random 26%": (rng.random((ih, iw)) < 0.26).astype(np.int32),         # the density of the tidied edge mask on the benchmark stream
        "sparse values 1..3": (rng.random((ih, iw)) < 0.08).astype(np.int32) * rng.integers(1, 4, (ih, iw)).astype(np.int32),
        "diagonals NE": ((xx + yy) % 4 == 0).astype(np.int32),                  # lines connected through NE / SW only
        "diagonals NW": ((xx - yy) % 4 == 0).astype(np.int32),                  # ... through NW / SE only
        "spiral": spiral(iw, ih),
        "combs joined in a strip's last row": comb(iw, ih, STRIP, STRIP - 1, 0),          # rows 7, 15, 23, 31: separate trees merge at the end of a strip
        "combs joined in a tile's last row": comb(iw, ih, LT_H, LT_H - 1, 0),             # row 31 only: teeth through all four strips
        "combs joined below a boundary": comb(iw, ih, STRIP, 0, STRIP - 1),               # rows 8, 16, 24, 32: joined by the first row of the next strip / tile
    }
    u = np.ones((ih, iw), np.int32)                                             # a uniform tile next to one that is not
    sel = (xx >= LT_W) & (yy < LT_H) if iw > LT_W else (yy >= STRIP)
    u[sel] = (rng.random((ih, iw)) < 0.5).astype(np.int32)[sel]
    p["uniform tile beside a busy one"] = u
    for a in p.values():
        a.setflags(write=False)
    return p


def oracle_label(m, bgc):
    ih, iw = m.shape
    want = np.zeros(iw * ih, np.int32)
    helpers.oracle().rdo_label8(helpers.P(want), helpers.P(np.ascontiguousarray(m)), bgc, iw, ih)
    return want


@pytest.fixture(scope="module")
def ctx():
    c = ra.Context(0)
    yield c
    c.close()


# ---- 1. the operator on crafted planes
@pytest.mark.gpu
@pytest.mark.parametrize("iw,ih", SHAPES)
def test_operator_on_crafted_planes(ctx, iw, ih):
    L = ra.lib()
    iu = L.init_oclimgutil(ctx.device, ctx.context)
    for name, m in planes(iw, ih).items():
        for bgc in (0, -1, 1):      # (1 occurs in every plane)
            a, b, t = ctx.buffer(np.ascontiguousarray(m)), ctx.buffer(iw * ih * 4), ctx.buffer(iw * ih * 4)
            L.oclimgutil_label8x_int_int(iu, b, a, t, bgc, iw, ih, ctx.queue, None)
            got = ctx.read(b, np.int32, iw * ih)
            ctx.release(a, b, t)
            want = oracle_label(m, bgc)
            assert np.array_equal(got, want), f"{iw}x{ih} {name}, background {bgc}: {int((got != want).sum())} labels differ, first at {np.flatnonzero(got != want)[:4].tolist()}"
    L.dispose_oclimgutil(iu)


# ---- 2. the fixtures are what they claim (no GPU)
def unions_issued(m):
    """per pixel, the unions k_label_tile's rule issues inside 64 x 32 tiles with every value labelled (background -1)"""
    ih, iw = m.shape
    yy, xx = np.indices((ih, iw))

    def same(dx, dy):
        ny, nx = yy + dy, xx + dx
        ok = (ny >= 0) & (nx >= 0) & (nx < iw) & (ny // LT_H == yy // LT_H) & (nx // LT_W == xx // LT_W)
        return ok & (m[np.clip(ny, 0, ih - 1), np.clip(nx, 0, iw - 1)] == m)
    w, e, n, nw, ne = same(-1, 0), same(1, 0), same(0, -1), same(-1, -1), same(1, -1)
    return (n & ~(w & nw)).astype(int) + (~n & nw & ~w).astype(int) + (~n & ne & ~e).astype(int)


def runs_in_tile_row(row):
    """runs of equal value in the first 64-pixel segment of a row"""
    seg = row[:LT_W]
    return 1 + int((seg[1:] != seg[:-1]).sum())


def test_fixtures_are_what_they_claim():
    src = open(os.path.join(helpers.ROOT, "rectdetect_amd", "csrc", "rd_k_label.hip")).read()
    geometry = tuple(int(re.search(r"#define %s (\d+)" % n, src).group(1)) for n in ("LT_W", "LT_H", "LT_TY"))
    assert geometry == (LT_W, LT_H, LT_H // STRIP), "the fixtures are placed by the kernel's tile and strips"
    iw, ih = BIG
    p = planes(iw, ih)
    # a component crossing every strip boundary, the tile boundary below row 31 and the one right of column 63 - in one plane, and it is ONE component
    sp = p["spiral"]
    lab = oracle_label(sp, 0).reshape(ih, iw)
    assert len(np.unique(lab[sp != 0])) == 1
    for r in (7, 15, 23, 31):
        assert ((sp[r] != 0) & (sp[r + 1] != 0)).any(), f"the spiral crosses rows {r}/{r + 1}"
    assert ((sp[:, 63] != 0) & (sp[:, 64] != 0)).any()
    for r in (7, 15, 23, 31):      # and diagonally only
        for name, dx in (("diagonals NE", -1), ("diagonals NW", 1)):
            d = p[name]
            xs = np.flatnonzero(d[r] != 0)
            xs = xs[(xs + dx >= 0) & (xs + dx < iw)]
            assert (d[r + 1, xs + dx] != 0).all() and not ((d[r] != 0) & (d[r + 1] != 0)).any(), name
    assert runs_in_tile_row(p["vertical stripes"][3]) == 64
    assert unions_issued(p["checkerboard"]).max() == 2 and unions_issued(p["random 50%"]).max() == 2 and unions_issued(p["random 26%"]).max() == 2
    # the bench stream's tidied edge mask has 27.8 runs per 64-pixel tile row: the 26 % plane is of that kind
    r26 = np.mean([runs_in_tile_row(row) for row in p["random 26%"]])
    assert 22 <= r26 <= 32, r26
    # teeth that meet only in a strip's / a tile's last row: without that row they are separate components, with it one
    for name, last in (("combs joined in a strip's last row", STRIP - 1), ("combs joined in a tile's last row", LT_H - 1)):
        c = p[name]
        teeth = np.flatnonzero(c[1, :LT_W] != 0)
        assert len(teeth) == LT_W // 2
        assert len(np.unique(oracle_label(c[1:last], 0).reshape(last - 1, iw)[0, teeth])) == len(teeth)
        assert len(np.unique(oracle_label(c[1:last + 1], 0).reshape(last, iw)[0, teeth])) == 1
    c = p["combs joined below a boundary"]
    teeth = np.flatnonzero(c[STRIP + 1, :LT_W] != 0)
    assert len(np.unique(oracle_label(c[STRIP + 1:2 * STRIP - 1], 0).reshape(STRIP - 2, iw)[0, teeth])) == len(teeth)
    assert len(np.unique(oracle_label(c[STRIP:2 * STRIP - 1], 0).reshape(STRIP - 1, iw)[1, teeth])) == 1
    # a uniform tile next to one that is not
    u = p["uniform tile beside a busy one"]
    assert (u[:LT_H, :LT_W] == 1).all() and len(np.unique(u[:LT_H, LT_W:2 * LT_W])) == 2


# ---- 3. the frame path of the rect kind: the tile kernel computes the tidy (SRC 2) and the boundary marks (SRC 1) itself
RECT_PLANES = [("tidy", "tidy"), ("label1", "label1"), ("strsum", "str_sum"), ("boundarysrc", "boundary_src"), ("boundary", "boundary")]
NFRAMES = 2                    # the second frame's sums carry the first frame's strong mask


@functools.lru_cache(maxsize=None)
def oracle_frames(iw, ih, seed, n=NFRAMES):
    """the oracle's planes of frames 0 .. n-1 of a synthetic stream (computed once, shared, read-only); the region merge as the order-free spec the HIP path reproduces"""
    orc = helpers.OracleRect(iw, ih, helpers.REGION_SPEC)
    out = []
    for t in range(n):
        orc.frame(synth.frame(synth.SEED0 + seed, iw, ih, t))
        got = {g: orc.plane(o).view(np.int32) for g, o in RECT_PLANES}
        for a in got.values():
            a.setflags(write=False)
        out.append(got)
    orc.close()
    return tuple(out)


def rect_planes(det):
    return {g: det.plane(g, np.int32) for g, _ in RECT_PLANES}


@pytest.mark.gpu
@pytest.mark.parametrize("iw,ih,seed", [(63, 29, 0), (64, 32, 0), (65, 33, 0), (129, 47, 0), (130, 109, 3)])
def test_rect_frame_path_against_oracle(iw, ih, seed):
    det = ra.Detector(iw, ih, nslots=1)
    for t, want in enumerate(oracle_frames(iw, ih, seed)):
        det.enqueue(synth.frame(synth.SEED0 + seed, iw, ih, t))
        det.poll(TAN36)
        for g, a in rect_planes(det).items():
            assert np.array_equal(a, want[g]), f"{iw}x{ih} frame {t}: plane {g} differs in {int((a != want[g]).sum())} pixels, first at {np.flatnonzero(a != want[g])[:4].tolist()}"
    det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nslots,group", [(6, 2), (32, 8)])
@pytest.mark.parametrize("iw,ih,seed", [(130, 109, 3), (64, 32, 0)])
def test_rect_group_launches_equal_the_single_slot_detector(iw, ih, seed, nslots, group):
    """the second and later frames of a group work on planes `zs` bytes behind the first's, and a group of 8 maps frames to XCDs: planes and lists must equal the
    single-slot detector's (whose first frames are pinned to the oracle as well)"""
    n = 2 * group
    frames = [synth.frame(synth.SEED0 + seed, iw, ih, t) for t in range(n)]
    outs = []
    for slots in (1, nslots):
        det = ra.Detector(iw, ih, nslots=slots, nworkers=1 if slots > 1 else 0)
        got = []
        if slots == 1:
            for f in frames:
                det.enqueue(f)
                got.append((det.poll(TAN36), det.last_segments(), rect_planes(det)))
        else:
            for f in frames:
                det.enqueue(f)
            for _ in frames:
                got.append((det.poll(TAN36), det.last_segments(), rect_planes(det)))
            assert det.frames_per_launch() == group
        det.close()
        outs.append(got)
    for t, want in enumerate(oracle_frames(iw, ih, seed)):
        for g in want:
            assert np.array_equal(outs[0][t][2][g], want[g]), f"single slot, frame {t}, plane {g}"
    for t, ((r1, s1, p1), (r2, s2, p2)) in enumerate(zip(*outs)):
        for g in p1:
            assert np.array_equal(p1[g], p2[g]), f"frame {t} of {n} in groups of {group}: plane {g} differs in {int((p1[g] != p2[g]).sum())} pixels"
        assert helpers.rects_equal(r1, r2) and helpers.segments_equal(s1, s2), f"frame {t} of {n} in groups of {group}: lists differ"


# ---- 4. the frame path of the poly kind: the tile kernel computes the mask (SRC 3)
@pytest.mark.gpu
@pytest.mark.parametrize("iw,ih,seed", [(130, 109, 3), (65, 33, 0)])
def test_poly_frame_path_against_oracle(iw, ih, seed):
    frames = [synth.frame(synth.SEED0 + seed, iw, ih, t) for t in range(2)]
    det = ra.PolylineDetector(iw, ih)
    for f in frames:
        det.enqueue(f)
    for t, f in enumerate(frames):
        segs, _ = det.poll()
        want, _ = helpers.oracle_poly(f)
        assert helpers.segments_equal(segs, want), f"{iw}x{ih} frame {t}: segment lists differ"
    det.close()
