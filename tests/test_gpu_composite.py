"""Composited quads on the GPU (rd_compositor, rd_detector_composite_polled): every frame equals, in every byte - pitch padding and a guard behind each plane
included - what the restatement of the header's contract gives (tests/composite.py: the adjugate, the per-pixel map in float64, fill and paste, painter's order,
the chroma mean).  Perspective quads inside, across and outside the frame, all six pixel formats and the ways a frame and a patch array can travel, the round trip
through the real rectifier, tile geometry, stacked items, the chroma rule, invalid items, jobs in flight, argument errors, behind the poll of both detector kinds,
the example program.  No tolerance anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import annotate
from tests import composite
from tests import helpers
from tests import jobframes
from tests import pixfmt
from tests import rectify
from tests.jobframes import FILL, MODES, L, assert_planes, cframe, into, padded, shapes

pytestmark = pytest.mark.gpu
LIM = ra.comp_limits()
TW, TH, CHUNK = LIM["tile_w"], LIM["tile_h"], LIM["chunk"]
PW, PH = 16, 12      # the module's compositor: neither square nor a power of two


@pytest.fixture
def mem():
    m = jobframes.Mem()
    yield m
    m.close()


@pytest.fixture(scope="module")
def comp():
    c = ra.Compositor(PW, PH, max_items=512, njobs=1)
    yield c
    c.close()


class Pending(jobframes.Pending):
    def enqueue(self, comp, items, patches=None, patches_kind="host"):
        kw = dict(self.kw)
        if patches is not None and patches_kind != "host":
            self.patch_src, self.patch_kind = np.ascontiguousarray(patches), patches_kind
            self.patch_ptr = self.mem.put(patches_kind, self.patch_src)
            patches = (self.patch_ptr, len(self.patch_src))
            kw["patches_on_device" if patches_kind == "device" else "patches_pinned"] = True
        return comp.enqueue(self.fmt, self.args, self.pitches, self.iw, self.ih, items, patches, **kw)


def run(comp, mem, fmt, src, iw, ih, items, patches=None, mode="inplace", out_pad=3, patches_kind="host", want=None, what=""):
    """one job, waited for and compared with the restatement (or with `want` = (planes, status) when the caller has it already); returns the frame's planes"""
    job = Pending(mem, fmt, src, iw, ih, mode, out_pad)
    job.enqueue(comp, items, patches, patches_kind)
    status = comp.wait()
    got = job.result()
    wplanes, wstatus = composite.draw(fmt, src, iw, ih, items, patches) if want is None else want
    assert status.tolist() == wstatus.tolist(), what
    assert_planes(got, into(job.out_init, wplanes, fmt, iw, ih), what or "%s %dx%d %s" % (ra.PIX_NAMES[fmt], iw, ih, mode))
    return got


def square(x0, y0, w, h=None):
    """the axis-aligned quad that covers exactly the pixels [x0, x0 + w) x [y0, y0 + h)"""
    h = w if h is None else h
    return np.array([(x0 - 0.5, y0 - 0.5), (x0 + w - 0.5, y0 - 0.5), (x0 + w - 0.5, y0 + h - 0.5), (x0 - 0.5, y0 + h - 0.5)])


def colour(k):
    return ((37 * k + 11) % 256, (91 * k + 60) % 256, (151 * k + 200) % 256)


def mixed_items(iw, ih, seed, n=12, npatches=3):
    """random perspective quads, both orientations: inside the frame, across each border, wholly outside; fills and pastes alternate"""
    rng = np.random.default_rng(seed)
    centres = [(iw * 0.5, ih * 0.5), (iw * 0.25, ih * 0.3), (2.0, ih * 0.5), (iw - 3.0, ih * 0.4), (iw * 0.6, 1.0), (iw * 0.4, ih - 2.0), (-1.0, -1.0), (iw + 1.0, ih + 1.0),
               (-80.0, ih * 0.5), (iw * 0.5, ih + 90.0), (iw * 0.7, ih * 0.7), (iw * 0.5, ih * 0.5)]
    rows = []
    for k in range(n):
        cx, cy = centres[k % len(centres)]
        q = composite.random_quad(rng, cx, cy, (30.0, 14.0, 22.0)[k % 3], flip=bool(k & 1))
        rows.append((q, (k // 2) % npatches if k % 2 else -1, colour(k)))
    return composite.items(rows)


def random_patches(seed, n=3, pw=PW, ph=PH):
    return np.random.default_rng(seed).integers(0, 256, (n, ph, pw, 3), dtype=np.uint8)


def size_for(fmt):
    """97 x 61 for the packed formats, 98 x 62 for 4:2:0: four tiles each way, tails in both directions"""
    return (97, 61) if fmt <= ra.PIX_RGBA else (98, 62)


# ---------------------------------------------------------------------------------------------- 1. formats and the ways frames and patches travel
@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_fill_and_paste_in_every_format_and_every_way_a_frame_travels(fmt, comp, mem):
    sizes = [(98, 62)] + ([(97, 61)] if fmt <= ra.PIX_RGBA else [])
    patches = random_patches(300 + fmt)
    for iw, ih in sizes:
        src = padded(fmt, iw, ih, 13, 3000 + fmt)
        items = mixed_items(iw, ih, 40 + fmt)
        want = composite.draw(fmt, src, iw, ih, items, patches)
        assert want[1].all() and 0.05 < (want[0][0] != src[0]).mean() < 0.95
        for k, mode in enumerate(MODES):
            got = run(comp, mem, fmt, src, iw, ih, items, patches, mode=mode, out_pad=0 if k % 2 else 9, patches_kind=("host", "device", "pinned")[k % 3], want=want,
                      what="%s %dx%d %s" % (ra.PIX_NAMES[fmt], iw, ih, mode))
            if fmt in (ra.PIX_BGRA, ra.PIX_RGBA):      # A is never written: in place it is the frame's own, out of place it came with the source's pixel
                assert np.array_equal(got[0][:, 3:iw * 4:4], src[0][:, 3:iw * 4:4])
            mem.close()


def test_a_larger_frame_with_quads_partly_and_wholly_outside(comp, mem):
    iw, ih = 200, 120
    for fmt in (ra.PIX_RGB, ra.PIX_NV12):
        src = padded(fmt, iw, ih, 5, 3100 + fmt)
        items = mixed_items(iw, ih, 77, n=24)
        patches = random_patches(78)
        run(comp, mem, fmt, src, iw, ih, items, patches, patches_kind="device")
        outside = composite.items([(composite.random_quad(np.random.default_rng(3), cx, cy, 30.0), -1, (1, 2, 3)) for cx, cy in ((-60.0, 40.0), (300.0, 40.0), (80.0, -70.0), (80.0, 200.0), (1e6, 1e6))])
        got = run(comp, mem, fmt, src, iw, ih, outside, what="wholly outside")
        assert_planes(got, src, "quads wholly outside changed the frame")
        mem.close()


# ---------------------------------------------------------------------------------------------- 2. the round trip through the rectifier
@pytest.mark.parametrize("fmt", [ra.PIX_BGR, ra.PIX_BGRA], ids=["BGR", "BGRA"])
def test_rectify_then_composite_is_the_identity_at_a_power_of_two(fmt, mem):
    iw, ih, n = 200, 120, 64
    src = padded(fmt, iw, ih, 4, 3200 + fmt)
    quads = [square(10, 10, n), square(130, 50, n), square(70, 0, n)]
    rect = ra.Rectifier(n, n, max_quads=4, njobs=1)
    c64 = ra.Compositor(n, n, max_items=8, njobs=1)
    try:
        frame = mem.put("device", src[0])
        pitch = src[0].shape[1]
        dpatches = mem.put("device", np.zeros(3 * n * n * 3, np.uint8))
        rect.enqueue(fmt, (frame,), (pitch,), iw, ih, quads, dpatches, on_device=True)
        assert rect.wait().tolist() == [1, 1, 1]
        # black over the three squares first: the paste has something to undo
        c64.enqueue(fmt, (frame,), (pitch,), iw, ih, ra.comp_items(quads), on_device=True)
        assert c64.wait().tolist() == [1, 1, 1]
        blacked = mem.get("device", frame, src[0].shape)
        assert not np.array_equal(blacked, src[0])
        c64.enqueue(fmt, (frame,), (pitch,), iw, ih, ra.comp_items(quads, patch=[0, 1, 2]), (dpatches, 3), on_device=True, patches_on_device=True)
        assert c64.wait().tolist() == [1, 1, 1]
        assert_planes([mem.get("device", frame, src[0].shape)], src, "rectify followed by composite")
    finally:
        rect.close()
        c64.close()


# ---------------------------------------------------------------------------------------------- 3. painter's order
def test_overlapping_fills_and_pastes_in_one_job(comp, mem):
    iw, ih = 97, 61
    src = padded(ra.PIX_BGRA, iw, ih, 4, 3300)
    rng = np.random.default_rng(33)
    patches = random_patches(34)
    rows = [(composite.random_quad(rng, 48 + 6 * np.cos(k), 30 + 5 * np.sin(k), 28.0 - k, flip=bool(k & 1)), k % 3 if k % 2 else -1, colour(k)) for k in range(10)]
    fwd, rev = composite.items(rows), composite.items(rows[::-1])
    want_f, want_r = (composite.draw(ra.PIX_BGRA, src, iw, ih, it, patches) for it in (fwd, rev))
    assert not np.array_equal(want_f[0][0], want_r[0][0])
    for it, want in ((fwd, want_f), (rev, want_r)):
        a = run(comp, mem, ra.PIX_BGRA, src, iw, ih, it, patches, want=want, what="painter's order")
        b = run(comp, mem, ra.PIX_BGRA, src, iw, ih, it, patches, want=want, what="painter's order, second run")
        assert_planes(a, b, "two consecutive runs")


# ---------------------------------------------------------------------------------------------- 4. tile geometry
@pytest.mark.parametrize("fmt", [ra.PIX_BGR, ra.PIX_RGBA, ra.PIX_NV12, ra.PIX_I420], ids=["BGR", "RGBA", "NV12", "I420"])
def test_tile_geometry(fmt, comp, mem):
    extra = 1 if fmt <= ra.PIX_RGBA else 2
    iw, ih = 3 * TW + extra, 3 * TH + extra
    src = padded(fmt, iw, ih, 3, 3400 + fmt)
    quads = [square(TW, TH, TW, TH),                               # exactly one tile: its edges lie on the tile boundaries
             square(TW - 1, TH - 1, 2, 2),                         # one pixel of each of four tiles
             square(0, 2 * TH - 1, iw, 2),                         # two rows astride a boundary, the whole width
             square(2 * TW - 1, 0, 2, ih),                         # two columns astride a boundary, the whole height
             np.array([(TW - 0.5, 3.0), (TW + 20.0, 3.5), (TW + 19.0, 9.0), (TW - 0.5, 8.0)]),      # an edge ON a tile boundary between pixel centres
             np.array([(float(TW), 20.0), (TW + 9.0, 21.0), (TW + 8.0, 27.0), (float(TW), 26.0)]),  # an edge through the first column of centres of a tile
             square(iw - 1, ih - 1, 1), square(0, 0, 1), square(iw - 1, 0, 1), square(0, ih - 1, 1),      # the frame's corners: tiles of one or two pixels
             square(3 * TW, 0, extra, ih), square(0, 3 * TH, iw, extra)]                             # the last columns and rows
    for k, q in enumerate(quads):
        run(comp, mem, fmt, src, iw, ih, composite.items([(q, -1, colour(k))]), mode="inplace" if k % 2 else "dev2dev", what="%s quad %d" % (ra.PIX_NAMES[fmt], k))
        mem.close()
    run(comp, mem, fmt, src, iw, ih, composite.items([(q, -1, colour(k)) for k, q in enumerate(quads)]))
    one = composite.items([(square(45, 20, 1), -1, (9, 99, 199))])      # a one-pixel quad
    run(comp, mem, fmt, src, iw, ih, one)
    assert composite.colours(one, None, iw, ih)[0].sum() == 1
    tiny = composite.items([(np.array([(45.2, 20.2), (45.8, 20.25), (45.75, 20.8), (45.15, 20.7)]), -1, (9, 99, 199))])      # smaller than a pixel, no centre inside
    assert composite.colours(tiny, None, iw, ih)[0].sum() == 0 and len(ra.composite_tiles(tiny, iw, ih)) > 0
    assert_planes(run(comp, mem, fmt, src, iw, ih, tiny), src, "a quad that contains no pixel centre wrote something")


# ---------------------------------------------------------------------------------------------- 5. more items over a tile than two ballots hold
@pytest.mark.parametrize("fmt", [ra.PIX_BGR, ra.PIX_NV12], ids=["BGR", "NV12"])
def test_130_small_fills_stacked_over_one_tile(fmt, comp, mem):
    iw, ih = size_for(fmt)
    src = padded(fmt, iw, ih, 1, 3500 + fmt)
    n = 2 * CHUNK + 2
    assert n == 130
    rng = np.random.default_rng(35)
    rows = []
    for k in range(n):      # all inside the tile (1, 1); each later one leaves pixels of the earlier ones visible
        x0, y0 = TW + int(rng.integers(0, TW - 6)), TH + int(rng.integers(0, TH - 4))
        rows.append((square(x0, y0, int(rng.integers(2, 7)), int(rng.integers(1, 5))), -1, colour(k)))
    items = composite.items(rows)
    hit, col, _ = composite.colours(items, None, iw, ih)
    visible = {tuple(int(v) for v in c) for c in col[hit]}
    shown = [k for k in range(n) if colour(k) in visible]      # (colour(k) is different for every k below 256)
    assert shown[0] < CHUNK and any(CHUNK <= k < 2 * CHUNK for k in shown) and shown[-1] == n - 1      # items of all three chunks show
    run(comp, mem, fmt, src, iw, ih, items, what="130 stacked fills")
    for count in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        run(comp, mem, fmt, src, iw, ih, items[:count], mode="dev2dev", what="%d stacked fills" % count)
        mem.close()


# ---------------------------------------------------------------------------------------------- 6. the chroma rule
@pytest.mark.parametrize("fmt", [ra.PIX_NV12, ra.PIX_I420], ids=["NV12", "I420"])
def test_the_chroma_rule(fmt, comp, mem):
    iw, ih = 98, 62
    src = padded(fmt, iw, ih, 0, 3600 + fmt)
    a, b, c = (255, 0, 0), (0, 255, 10), (7, 0, 255)
    rows = [(square(20, 20, 1), -1, a),                                  # 1 of the four luma pixels of sample (10, 10)
            (square(30, 20, 2, 1), -1, a),                               # 2 of sample (15, 10)
            (square(40, 20, 2, 1), -1, a), (square(40, 21, 1), -1, b),   # 3 of sample (20, 10), two colours
            (square(50, 20, 2), -1, a), (square(51, 21, 1), -1, c),      # 4 of sample (25, 10), the last of another colour
            (square(61, 21, 2), -1, b)]                                  # one pixel each of samples (30, 10), (31, 10), (30, 11), (31, 11)
    items = composite.items(rows)
    got = run(comp, mem, fmt, src, iw, ih, items)

    def sample(planes, cx, cy):
        return (int(planes[1][cy, 2 * cx]), int(planes[1][cy, 2 * cx + 1])) if fmt == ra.PIX_NV12 else (int(planes[1][cy, cx]), int(planes[2][cy, cx]))

    def uv(*cols):      # the header's rule, by hand
        n = len(cols)
        m = [(sum(col[ch] for col in cols) + n // 2) // n for ch in range(3)]
        return tuple(int(v) for v in annotate.yuv(*m)[1:])

    assert sample(got, 10, 10) == uv(a) and sample(got, 15, 10) == uv(a, a) and sample(got, 20, 10) == uv(a, a, b) and sample(got, 25, 10) == uv(a, a, a, c)
    assert uv(a, a, b) != uv(a) and uv(a, a, a, c) != uv(a)
    for cx, cy in ((30, 10), (31, 10), (30, 11), (31, 11)):
        assert sample(got, cx, cy) == uv(b)
    for cx, cy in ((11, 10), (10, 11), (16, 10), (26, 10), (29, 10), (32, 11)):      # samples none of whose pixels is covered stay
        assert sample(got, cx, cy) == sample(src, cx, cy)
    assert got[0][20, 20] == int(annotate.yuv(*a)[0]) and got[0][21, 20] == src[0][21, 20]


# ---------------------------------------------------------------------------------------------- 7. invalid items, empty and full jobs
def test_invalid_items_among_valid_ones_and_empty_and_full_jobs(comp, mem):
    iw, ih = 97, 61
    src = padded(ra.PIX_BGR, iw, ih, 2, 3700)
    patches = random_patches(37)
    bow = np.array([(10.0, 10.0), (50.0, 10.0), (10.0, 50.0), (50.0, 50.0)])
    concave = np.array([(10.0, 10.0), (50.0, 10.0), (20.0, 20.0), (10.0, 50.0)])
    nan = np.array([(np.nan, 10.0), (50.0, 10.0), (50.0, 50.0), (10.0, 50.0)])
    inf = np.array([(10.0, 10.0), (np.inf, 10.0), (50.0, 50.0), (10.0, 50.0)])
    huge = np.array([(0.0, 0.0), (1e300, 0.0), (1e300, 1e300), (0.0, 1e300)])
    good = mixed_items(iw, ih, 38, n=4)
    rows = [(bow, -1, (1, 1, 1)), (good[0]["quad"], -1, colour(0)), (concave, 1, (2, 2, 2)), (good[1]["quad"], 2, colour(1)), (nan, -1, (3, 3, 3)), (inf, 0, (4, 4, 4)),
            (good[2]["quad"], -1, colour(2)), (huge, -1, (5, 5, 5)), (square(-300, 10, 40), -1, (6, 6, 6))]
    items = composite.items(rows)
    want = composite.draw(ra.PIX_BGR, src, iw, ih, items, patches)
    assert want[1].tolist() == [0, 1, 0, 1, 0, 0, 1, 0, 1]
    run(comp, mem, ra.PIX_BGR, src, iw, ih, items, patches, want=want)
    only_bad = composite.items([rows[0], rows[2], rows[4], rows[5], rows[7]])
    assert_planes(run(comp, mem, ra.PIX_BGR, src, iw, ih, only_bad, patches), src, "items of status 0 wrote something")
    run(comp, mem, ra.PIX_BGR, src, iw, ih, only_bad, patches, mode="dev2pinned")
    mem.close()
    for fmt in pixfmt.FORMATS:      # n = 0
        w, h = size_for(fmt)
        s = padded(fmt, w, h, 6, 3710 + fmt)
        for mode in ("inplace", "dev2dev", "host2pinned"):
            got = run(comp, mem, fmt, s, w, h, composite.items([]), mode=mode, what="%s n = 0 %s" % (ra.PIX_NAMES[fmt], mode))
            if mode == "inplace":
                assert_planes(got, s, "an empty job in place")
        mem.close()
    assert comp.max_items == 512      # a full job
    rng = np.random.default_rng(39)
    full = composite.items([(composite.random_quad(rng, rng.uniform(-5, iw + 5), rng.uniform(-5, ih + 5), rng.uniform(2, 9), flip=bool(k & 1)), k % 3 if k % 5 == 0 else -1, colour(k)) for k in range(512)])
    run(comp, mem, ra.PIX_BGR, src, iw, ih, full, patches, what="max_items items")
    with pytest.raises(ValueError):
        Pending(mem, ra.PIX_BGR, src, iw, ih, "inplace").enqueue(comp, np.concatenate([full, full[:1]]), patches)      # one more


# ---------------------------------------------------------------------------------------------- 8. jobs in flight
def test_three_jobs_in_flight(mem):
    iw, ih = 98, 62
    c3 = ra.Compositor(PW, PH, max_items=32, njobs=3)
    try:
        with pytest.raises(RuntimeError):
            c3.wait()
        jobs = []
        for k, (fmt, mode, pkind) in enumerate([(ra.PIX_BGR, "inplace", "pinned"), (ra.PIX_NV12, "host2pinned", "host"), (ra.PIX_RGBA, "dev2dev", "device")]):
            src = padded(fmt, iw, ih, 2 + k, 3800 + k)
            items = mixed_items(iw, ih, 80 + k, n=6 + k)
            patches = random_patches(90 + k)
            job = Pending(mem, fmt, src, iw, ih, mode, 4)
            assert job.enqueue(c3, items, patches, pkind) == k
            jobs.append((job, fmt, src, items, patches))
        for k, (job, fmt, src, items, patches) in enumerate(jobs):
            want, wstatus = composite.draw(fmt, src, iw, ih, items, patches)
            assert c3.wait().tolist() == wstatus.tolist()
            assert_planes(job.result(), into(job.out_init, want, fmt, iw, ih), "job %d of three in flight" % k)
        with pytest.raises(RuntimeError):
            c3.wait()
    finally:
        c3.close()


def test_one_job_too_many_is_fatal():
    """in a child process: the fourth enqueue with njobs = 3 and nothing waited for ends the process with a message, as the annotator's does"""
    jobframes.assert_one_job_too_many_is_fatal("s = ra.Compositor(8, 8, max_items=1, njobs=3)\nit = ra.comp_items([[(4, 4), (40, 4), (40, 40), (4, 40)]])",
                                               "s.enqueue(ra.PIX_BGR, (d,), (64 * 3,), 64, 64, it, on_device=True)", "rd_compositor_enqueue")


def test_staging_buffers_grow_with_jobs_in_flight(mem):
    """host frames into pinned destinations: the second job's frame is larger than the first's and takes three host patches where that took one, enqueued while
    it is in flight; the third is the small one again"""
    c2 = ra.Compositor(PW, PH, max_items=16, njobs=2)
    try:
        jobs = []
        for k, (fmt, iw, ih, npatches) in enumerate([(ra.PIX_BGR, 34, 18, 1), (ra.PIX_NV12, 98, 62, 3), (ra.PIX_BGR, 34, 18, 1)]):
            src = padded(fmt, iw, ih, 1 + k, 3850 + k)
            items = mixed_items(iw, ih, 85 + k, n=4 + 2 * npatches, npatches=npatches)
            assert sorted(set(items["patch"].tolist())) == list(range(-1, npatches))
            jobs.append((Pending(mem, fmt, src, iw, ih, "host2pinned", 5 - k), fmt, src, iw, ih, items, random_patches(95 + k, n=npatches)))

        def check(job, status):
            pend, fmt, src, iw, ih, items, patches = job
            want, wstatus = composite.draw(fmt, src, iw, ih, items, patches)
            assert status.tolist() == wstatus.tolist() and wstatus.any()
            assert_planes(pend.result(), into(pend.out_init, want, fmt, iw, ih), "%s %dx%d" % (ra.PIX_NAMES[fmt], iw, ih))

        jobframes.growing_jobs(c2, jobs, lambda job: job[0].enqueue(c2, job[5], job[6]), check)
    finally:
        c2.close()


# ---------------------------------------------------------------------------------------------- 9. argument errors
def test_argument_errors_return_minus_one_and_the_next_job_is_correct(mem):
    iw, ih = 97, 61
    yw, yh = 98, 62
    src = padded(ra.PIX_BGR, iw, ih, 3, 3900)
    ysrc = padded(ra.PIX_NV12, yw, yh, 0, 3901)
    c1 = ra.Compositor(PW, PH, max_items=8, njobs=1)
    dframe, pitch = mem.put("device", src[0]), src[0].shape[1]
    dy, duv = mem.put("device", ysrc[0]), mem.put("device", ysrc[1])
    out_init = padded(ra.PIX_BGR, iw, ih, 1, FILL)
    out, opitch = mem.put("device", out_init[0]), out_init[0].shape[1]
    pout = mem.put("pinned", out_init[0])
    pageable = np.zeros(out_init[0].size, np.uint8)
    patches = random_patches(391)
    dpatches = mem.put("device", patches)
    items = mixed_items(iw, ih, 392, n=8)
    assert (items["patch"] >= 0).any() and items["patch"].max() == 2
    fills = items.copy()
    fills["patch"] = -1
    low, high = items.copy(), items.copy()
    low[3]["patch"] = -2
    high[5]["patch"] = 3
    P, I = ctypes.c_void_p * 3, ctypes.c_int * 3

    def call(fmt=ra.PIX_BGR, pl=(dframe, None, None), pi=(pitch, 0, 0), w=iw, h=ih, kind=1, items_p=items.ctypes.data, n=len(items), pp=dpatches, np_=3, pkind=1,
             opl=(out, None, None), opi=(opitch, 0, 0), out_kind=1):
        return L().rd_compositor_enqueue(c1.h, fmt, P(*pl), I(*pi), w, h, kind, items_p, n, pp, np_, pkind, P(*opl) if opl is not None else None, I(*opi) if opi is not None else None, out_kind)

    hostframe = np.ascontiguousarray(src[0])
    errors = {
        "unknown format": dict(fmt=6), "negative format": dict(fmt=-1),
        "unknown on_device": dict(kind=3), "unknown out_kind": dict(out_kind=0), "out_kind host": dict(out_kind=3),
        "no width": dict(w=0), "no height": dict(h=0), "too wide": dict(w=65537), "too high": dict(h=65537),
        "NULL plane": dict(pl=(None, None, None)),
        "NULL chroma plane": dict(fmt=ra.PIX_NV12, pl=(dy, None, None), pi=(yw, yw, 0), w=yw, h=yh, opl=None),
        "NULL third plane": dict(fmt=ra.PIX_I420, pl=(dy, duv, None), pi=(yw, yw // 2, yw // 2), w=yw, h=yh, opl=None),
        "short pitch": dict(pi=(iw * 3 - 1, 0, 0)),
        "short chroma pitch": dict(fmt=ra.PIX_NV12, pl=(dy, duv, None), pi=(yw, yw - 1, 0), w=yw, h=yh, opl=None),
        "odd width with 4:2:0": dict(fmt=ra.PIX_NV12, pl=(dy, duv, None), pi=(yw, yw, 0), w=yw - 1, h=yh, opl=None),
        "odd height with 4:2:0": dict(fmt=ra.PIX_I420, pl=(dy, duv, duv), pi=(yw, yw, yw), w=yw, h=yh - 1, opl=None),
        "n < 0": dict(n=-1), "n > max_items": dict(n=len(items) + 1), "NULL items": dict(items_p=None),
        "patch below -1": dict(items_p=low.ctypes.data), "patch not below npatches": dict(items_p=high.ctypes.data), "a paste with no patches at all": dict(np_=0),
        "npatches < 0": dict(items_p=fills.ctypes.data, np_=-1),
        "NULL patches while an item pastes": dict(pp=None), "unknown patches_kind": dict(pkind=3), "pageable patches as device memory": dict(pp=patches.ctypes.data),
        "in place on a host frame": dict(pl=(hostframe.ctypes.data, None, None), kind=0, opl=None),
        "in place on a pinned frame": dict(pl=(pout, None, None), pi=(opitch, 0, 0), kind=2, opl=None),
        "NULL out plane": dict(opl=(None, None, None)), "NULL out pitches": dict(opi=None), "short out pitch": dict(opi=(iw * 3 - 1, 0, 0)),
        "pageable out as pinned": dict(opl=(pageable.ctypes.data, None, None), out_kind=2),
        "pageable out as device memory": dict(opl=(pageable.ctypes.data, None, None)),
        "pinned out as device memory": dict(opl=(pout, None, None)), "device out as pinned": dict(out_kind=2),
    }
    try:
        for name, kw in errors.items():
            assert call(**kw) == -1, name
            assert L().rd_compositor_wait(c1.h, None) == -1, name + ": nothing may have been enqueued"
        assert np.array_equal(mem.get("device", dframe, src[0].shape), src[0]) and np.array_equal(mem.get("device", out, out_init[0].shape), out_init[0])
        want, wstatus = composite.draw(ra.PIX_BGR, src, iw, ih, items, patches)
        assert call() == 0      # the first job after all of them: sequence number 0, the right bytes
        assert c1.wait().tolist() == wstatus.tolist()
        assert_planes([mem.get("device", out, out_init[0].shape)], into(out_init, want, ra.PIX_BGR, iw, ih), "the job after the refused ones")
        assert call(opl=None) == 1 and len(c1.wait()) == len(items)      # in place
        assert_planes([mem.get("device", dframe, src[0].shape)], want, "in place after the refused ones")
        assert call(items_p=fills.ctypes.data, pp=None, np_=0, pkind=7) == 2 and len(c1.wait()) == len(items)      # fills alone need no patches
        for bad in ((-1, 8, 8, 1, 1), (0, 0, 8, 1, 1), (0, 8, 0, 1, 1), (0, 16385, 8, 1, 1), (0, 8, 16385, 1, 1), (0, 8, 8, 0, 1), (0, 8, 8, (1 << 20) + 1, 1), (0, 8, 8, 1, 0),
                    (0, 8, 8, 1, 1025), (L().rd_device_count(), 8, 8, 1, 1)):      # (device, pw, ph, max_items, njobs)
            assert not L().rd_compositor_create(*bad), bad
        with pytest.raises(ValueError):
            ra.Compositor(max_items=0)
        with pytest.raises(ValueError):
            c1.enqueue(ra.PIX_BGR, (dframe,), (pitch,), iw, ih, items, random_patches(1, pw=PW + 1), on_device=True)      # host patches of another size
    finally:
        c1.close()


# ---------------------------------------------------------------------------------------------- 10. behind the poll
SIW, SIH = 320, 240
TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
SEED = 0x5EED0000


def rect_items(rects, patch_every=2):
    """fills and pastes of the frame's own rectangles"""
    quads = ra.rect_quads(rects)
    assert np.array_equal(quads, rectify.rect_quads(rects))
    return ra.comp_items(quads, patch=[k % 3 if k % patch_every == 0 else -1 for k in range(len(quads))], colour=[colour(k) for k in range(len(quads))])


@pytest.mark.parametrize("kind", ["rectangles", "polyline"])
def test_composite_polled_behind_a_real_poll(kind, mem):
    frame = cframe(SEED, SIW, SIH, 0)
    src = [frame.reshape(SIH, SIW * 3)]
    patches = random_patches(101)
    rdet = ra.Detector(SIW, SIH, nslots=1, aperture=TAN36)      # the rectangles of the frame, for both kinds
    c2 = ra.Compositor(PW, PH, max_items=256, njobs=2)
    det = rdet if kind == "rectangles" else ra.PolylineDetector(SIW, SIH, nslots=2)
    try:
        out_init = padded(ra.PIX_BGR, SIW, SIH, 8, FILL)
        pout = mem.put("pinned", out_init[0])
        with pytest.raises(ValueError):      # nothing polled yet
            det.composite_polled(c2, ra.comp_items([square(5, 5, 9)]), out_planes=(pout,), out_pitches=(SIW * 3 + 8,), out_pinned=True)
        rdet.enqueue(frame)
        rects = rdet.poll(TAN36)
        assert len(rects) > 0, "the synthetic frame has no rectangle at this size"
        items = rect_items(rects)
        want, wstatus = composite.draw(ra.PIX_BGR, src, SIW, SIH, items, patches)
        assert wstatus.any() and (want[0] != src[0]).sum() > 100
        # a host frame: the detector's uploaded copy is the source, pinned memory the destination
        if kind == "polyline":
            det.enqueue(frame)
            det.poll()
        with pytest.raises(ValueError):      # a host frame without a destination
            det.composite_polled(c2, items, patches)
        det.composite_polled(c2, items, patches, out_planes=(pout,), out_pitches=(SIW * 3 + 8,), out_pinned=True)
        assert c2.wait().tolist() == wstatus.tolist()
        assert_planes([mem.get("pinned", pout, out_init[0].shape)], into(out_init, want, ra.PIX_BGR, SIW, SIH), "host frame, pinned destination")
        # a device frame, in place
        padded_frame = padded(ra.PIX_BGR, SIW, SIH, 4, [src[0]])
        dframe = mem.put("device", padded_frame[0])
        det.enqueue(dframe, ws=SIW * 3 + 4, on_device=True)
        if kind == "rectangles":
            assert helpers.rects_equal(det.poll(TAN36), rects)
        else:
            det.poll()
        dpatches = mem.put("device", patches)
        det.composite_polled(c2, items, (dpatches, len(patches)), patches_on_device=True)
        assert c2.wait().tolist() == wstatus.tolist()
        assert_planes([mem.get("device", dframe, padded_frame[0].shape)], into(padded_frame, want, ra.PIX_BGR, SIW, SIH), "device frame, in place")
    finally:
        if det is not rdet:
            det.close()
        rdet.close()
        c2.close()


@pytest.mark.parametrize("kind", ["rectangles", "polyline"])
def test_composite_polled_at_scale_2(kind, mem):
    """a 640 x 480 source detected at 320 x 240: quads in detector coordinates, the job on the full-size source - what Compositor.enqueue gives there for the mapped quads"""
    sw, sh = 2 * SIW, 2 * SIH
    frame = cframe(SEED, sw, sh, 0)
    src = [frame.reshape(sh, sw * 3)]
    patches = random_patches(102)
    c2 = ra.Compositor(PW, PH, max_items=256, njobs=1)
    rdet = ra.Detector(SIW, SIH, nslots=1, aperture=TAN36)
    det = rdet if kind == "rectangles" else ra.PolylineDetector(SIW, SIH, nslots=2)
    try:
        dsrc = mem.put("device", src[0])
        rdet.enqueue_scaled(ra.PIX_BGR, (dsrc,), (sw * 3,), on_device=True, scale=2)
        rects = rdet.poll(TAN36)
        assert len(rects) > 0, "the synthetic frame has no rectangle at this size"
        if kind == "polyline":
            det.enqueue_scaled(ra.PIX_BGR, (dsrc,), (sw * 3,), on_device=True, scale=2)
            det.poll()
        items = rect_items(rects)
        mapped = items.copy()
        mapped["quad"] = items["quad"] * 2.0 + 0.5
        # the reference: a job of the compositor itself on the full-size source, into another frame
        ref_init = padded(ra.PIX_BGR, sw, sh, 0, FILL)
        ref = mem.put("device", ref_init[0])
        c2.enqueue(ra.PIX_BGR, (dsrc,), (sw * 3,), sw, sh, mapped, patches, out_planes=(ref,), out_pitches=(sw * 3,), on_device=True)
        status = c2.wait()
        want = mem.get("device", ref, ref_init[0].shape)
        wplanes, wstatus = composite.draw(ra.PIX_BGR, src, sw, sh, mapped, patches)
        assert status.tolist() == wstatus.tolist() and wstatus.any()
        assert_planes([want], wplanes, "Compositor.enqueue on the full-size source")
        assert (want != src[0]).sum() > 400
        det.composite_polled(c2, items, patches)      # in place, quads in detector coordinates
        assert c2.wait().tolist() == wstatus.tolist()
        assert_planes([mem.get("device", dsrc, src[0].shape)], [want], "scale 2, device frame in place")
        # the same frame from the host: into a destination of source size, refused without one
        det.enqueue_scaled(ra.PIX_BGR, frame, scale=2)
        det.poll(TAN36) if kind == "rectangles" else det.poll()
        with pytest.raises(ValueError):
            det.composite_polled(c2, items, patches)
        out_init = padded(ra.PIX_BGR, sw, sh, 0, FILL)
        out = mem.put("device", out_init[0])
        det.composite_polled(c2, items, patches, out_planes=(out,), out_pitches=(sw * 3,))
        assert c2.wait().tolist() == wstatus.tolist()
        assert_planes([mem.get("device", out, out_init[0].shape)], [want], "scale 2, host frame")
    finally:
        if det is not rdet:
            det.close()
        rdet.close()
        c2.close()


# ---------------------------------------------------------------------------------------------- the convenience call
def test_composite_convenience_call():
    frame = cframe(7, 200, 120, 0)
    items = mixed_items(200, 120, 111)
    patches = random_patches(112, pw=8, ph=8)
    c = ra.Compositor(8, 8, max_items=64, njobs=1)
    try:
        got = c.composite(frame, items, patches)
        assert got.shape == frame.shape
        assert np.array_equal(got.reshape(120, 600), composite.draw(ra.PIX_BGR, [frame.reshape(120, 600)], 200, 120, items, patches)[0][0])
        assert np.array_equal(c.composite(frame, items[:0]), frame)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------- the example program
@pytest.mark.parametrize("mosaic", [False, True], ids=["fill", "mosaic"])
def test_rdredact_writes_the_frames_the_binding_gives(mosaic, tmp_path):
    """examples/rdredact on a YUV4MPEG2 stream of two frames: the stream that comes out holds, frame by frame, what the binding's detector, rectifier and compositor
    give for the I420 frame - and that is what the restatements give"""
    iw, ih, nframes = 640, 480, 2
    frames = [pixfmt.convert(cframe(SEED, iw, ih, t), ra.PIX_I420)[0] for t in range(nframes)]
    header = b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (iw, ih)
    with open(tmp_path / "in.y4m", "wb") as f:
        f.write(header)
        for planes in frames:
            f.write(b"FRAME\n" + b"".join(np.ascontiguousarray(p).tobytes() for p in planes))
    res = subprocess.run([os.path.join(helpers.ROOT, "examples", "rdredact"), str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), "0"] + (["mosaic"] if mosaic else []),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path, timeout=120)
    assert res.returncode == 0, res.stderr.decode()
    data = open(tmp_path / "out.y4m", "rb").read()
    assert data.startswith(header)
    ny, nc = iw * ih, iw * ih // 4
    assert len(data) == len(header) + nframes * (6 + ny + 2 * nc)
    det = ra.Detector(iw, ih, nslots=1)
    redacted = 0
    try:
        for t, planes in enumerate(frames):
            det.enqueue_planes(ra.PIX_I420, planes)
            rects = det.poll(np.tan(72.0 / 2 / 180.0 * np.pi))
            quads = ra.rect_quads(rects)
            redacted += len(quads)
            src = [np.ascontiguousarray(p).reshape(rows, row) for p, (rows, row) in zip(planes, shapes(ra.PIX_I420, iw, ih))]
            if mosaic:
                patches, _ = rectify.patches(rectify.contract_bgr(ra.PIX_I420, planes), quads, 8, 8)
                items = ra.comp_items(quads, patch=np.arange(len(quads)))
            else:
                patches, items = None, ra.comp_items(quads)
            want, _ = composite.draw(ra.PIX_I420, src, iw, ih, items, patches)
            at = len(header) + t * (6 + ny + 2 * nc)
            assert data[at:at + 6] == b"FRAME\n"
            got = np.frombuffer(data, np.uint8, ny + 2 * nc, at + 6)
            assert_planes([got[:ny].reshape(ih, iw), got[ny:ny + nc].reshape(ih // 2, iw // 2), got[ny + nc:].reshape(ih // 2, iw // 2)], want, "frame %d" % t)
            assert (want[0] != src[0]).sum() > 100
    finally:
        det.close()
    assert redacted > 0 and ("%d rectangle(s)" % redacted) in res.stderr.decode()
