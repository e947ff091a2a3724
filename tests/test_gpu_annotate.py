"""Annotated frames on the GPU (rd_annotator, rd_detector_annotate_polled): every frame equals, in every byte - pitch padding and a guard behind each plane
included - what the restatement of the header's contract draws (tests/annotate.py: the definition's loop with floor division, painter's order, the chroma rule,
RD_ANNOT_CLEAR).  Directions, thickness, lines leaving the frame, painter's order, tile edges, crowded tiles, all six pixel formats and the four ways a frame can
travel, jobs in flight, behind the poll of both detector kinds, argument errors.  No tolerance anywhere."""
import ctypes
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import annotate
from tests import helpers
from tests import jobframes
from tests import pixfmt
from tests.jobframes import FILL, L, assert_planes, cframe, into, padded, shapes

pytestmark = pytest.mark.gpu
MODES = ("inplace", "dev2dev", "host2pinned", "pinned2dev")
LIM = ra.annot_limits()
TW, TH, CHUNK = LIM["tile_w"], LIM["tile_h"], LIM["chunk"]


def golden(name):
    return np.load(os.path.join(helpers.GOLDEN, name + ".npz"), allow_pickle=False)


@pytest.fixture
def mem():
    m = jobframes.Mem()
    yield m
    m.close()


@pytest.fixture(scope="module")
def an():
    a = ra.Annotator(max_prims=4096, njobs=1)
    yield a
    a.close()


class Pending(jobframes.Pending):
    def enqueue(self, an, prims, flags):
        return an.enqueue(self.fmt, self.args, self.pitches, self.iw, self.ih, prims, flags, **self.kw)


def expected(fmt, src, iw, ih, prims, flags, out_init=None):
    return into(out_init, annotate.draw(fmt, src, iw, ih, prims, clear=bool(flags & ra.ANNOT_CLEAR)), fmt, iw, ih)


def run(an, mem, fmt, src, iw, ih, prims, flags=0, mode="inplace", out_pad=3, want=None, what=""):
    """one job, waited for and compared with the restatement (or with `want`, the drawn source, when the caller has it already); returns the frame's planes"""
    job = Pending(mem, fmt, src, iw, ih, mode, out_pad)
    job.enqueue(an, prims, flags)
    assert an.wait() == len(prims)
    got = job.result()
    exp = expected(fmt, src, iw, ih, prims, flags, job.out_init) if want is None else into(job.out_init, want, fmt, iw, ih)
    assert_planes(got, exp, what or "%s %dx%d %s" % (ra.PIX_NAMES[fmt], iw, ih, mode))
    return got


def size_for(fmt, small=True):
    """97 x 61 for the packed formats, 98 x 62 for 4:2:0 - two tiles each way, odd sizes, a tail in both directions"""
    return (97, 61) if fmt <= ra.PIX_RGBA else (98, 62)


COLOURS = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (250, 128, 7), (33, 66, 199), (255, 255, 255), (1, 2, 3)]


def coloured(lines, t=1):
    """(x0, y0, x1, y1[, t]) rows -> primitives with distinct colours"""
    return annotate.prims([tuple(l[:4]) + COLOURS[k % len(COLOURS)][:2] + ((COLOURS[k % len(COLOURS)][2] + 16 * (k // len(COLOURS))) % 256,) + ((l[4],) if len(l) > 4 else (t,)) for k, l in enumerate(lines)])


# ---------------------------------------------------------------------------------------------- 1. directions
OFFSETS = [(20, 0), (-20, 0), (0, 15), (0, -15), (12, 12), (-12, 12), (12, -12), (-12, -12), (0, 0), (20, 7), (20, -7), (-20, 7), (-20, -7), (7, 20), (7, -20), (-7, 20),
           (-7, -20), (1, 0), (0, 1), (1, 1), (13, 12), (12, 13), (-13, 12), (25, 1)]


def test_directions_one_line_per_job_both_endpoint_orders(an, mem):
    iw, ih = 97, 61
    src = padded(ra.PIX_BGR, iw, ih, 5, 1001)
    assert len(OFFSETS) == 24
    for dx, dy in OFFSETS:
        fwd = coloured([(40, 30, 40 + dx, 30 + dy)])
        rev = coloured([(40 + dx, 30 + dy, 40, 30)])
        a = run(an, mem, ra.PIX_BGR, src, iw, ih, fwd, what="line to (%d, %d)" % (dx, dy))
        b = run(an, mem, ra.PIX_BGR, src, iw, ih, rev, what="line from (%d, %d)" % (dx, dy))
        assert np.array_equal(a[0], b[0]), "the order of the endpoints changed the line to (%d, %d)" % (dx, dy)
        assert (a[0] != src[0]).sum() > 0
        mem.close()


@pytest.mark.parametrize("fmt", [ra.PIX_BGR, ra.PIX_NV12], ids=["BGR", "NV12"])
def test_directions_all_in_one_job(fmt, an, mem):
    iw, ih = size_for(fmt)
    src = padded(fmt, iw, ih, 5, 1002)
    lines = [(40, 30, 40 + dx, 30 + dy) if k % 2 == 0 else (40 + dx, 30 + dy, 40, 30) for k, (dx, dy) in enumerate(OFFSETS)]
    run(an, mem, fmt, src, iw, ih, coloured(lines))


# ---------------------------------------------------------------------------------------------- 2. thickness
@pytest.mark.parametrize("fmt", [ra.PIX_BGR, ra.PIX_I420], ids=["BGR", "I420"])
def test_thickness(fmt, an, mem):
    iw, ih = size_for(fmt)
    src = padded(fmt, iw, ih, 2, 1003)
    for t in (1, 2, 3, 4, 7, 255):      # (at 255 the brush is taller than the frame)
        got = run(an, mem, fmt, src, iw, ih, coloured([(30, 5, 45, 55), (5, 20, 90, 35)], t), what="thickness %d" % t)
        if t == 255:
            assert (got[0][:, :iw * (3 if fmt == ra.PIX_BGR else 1)] != src[0][:, :iw * (3 if fmt == ra.PIX_BGR else 1)]).mean() > 0.9
        mem.close()


# ---------------------------------------------------------------------------------------------- 3. outside the frame
def test_lines_that_leave_the_frame(an, mem):
    iw, ih = 97, 61
    src = padded(ra.PIX_RGB, iw, ih, 7, 1004)
    lo, hi = annotate.COORD_MIN, annotate.COORD_MAX
    lines = [(-30, 20, 50, 30, 2), (50, 30, 130, 40, 3), (40, -25, 50, 30, 2), (50, 30, 60, 100, 1), (-40, -30, 140, 90, 4), (96, 0, 96, 60, 1), (0, 60, 96, 60, 5), (-1, 0, -1, 60, 1),
             (97, 0, 97, 60, 1), (0, -1, 96, -1, 2), (0, 61, 96, 61, 1)]
    for l in lines:
        run(an, mem, ra.PIX_RGB, src, iw, ih, coloured([l]), what="line %r" % (l,))
    run(an, mem, ra.PIX_RGB, src, iw, ih, coloured(lines), what="all of them")
    mem.close()
    for l in [(-50, -10, -5, -40, 3), (200, 10, 300, 70, 2), (10, 200, 90, 300, 255), (lo, 10, -100, 20, 9)]:      # wholly outside: not a byte changes
        got = run(an, mem, ra.PIX_RGB, src, iw, ih, coloured([l]), what="outside %r" % (l,))
        assert np.array_equal(got[0], src[0])
    through = coloured([(lo, lo, hi, hi, 3), (lo, 700000, hi, -699930, 2), (hi, 30, lo, 31, 1)])
    got = run(an, mem, ra.PIX_RGB, src, iw, ih, through, what="across the whole legal range")
    assert (got[0] != src[0]).sum() > 300
    got = run(an, mem, ra.PIX_RGB, src, iw, ih, through, mode="dev2dev", what="across the whole legal range, out of place")


def test_illegal_primitives_are_refused_and_the_frame_stays(an, mem):
    iw, ih = 97, 61
    src = padded(ra.PIX_BGR, iw, ih, 0, 1005)
    job = Pending(mem, ra.PIX_BGR, src, iw, ih, "inplace", 0)
    good = (10, 10, 50, 40, 9, 9, 9, 1)
    for bad in [(1048576, 0, 5, 5, 1, 1, 1, 1), (0, -1048577, 5, 5, 1, 1, 1, 1), (0, 0, 1048576, 5, 1, 1, 1, 1), (0, 0, 5, -1048577, 1, 1, 1, 1), (10, 10, 50, 40, 1, 1, 1, 0)]:
        for rows in ([bad], [good, bad], [bad, good]):
            with pytest.raises(ValueError):
                job.enqueue(an, annotate.prims(rows), 0)
            with pytest.raises(RuntimeError):
                an.wait()      # nothing was enqueued
    assert np.array_equal(job.result()[0], src[0])
    job.enqueue(an, annotate.prims([good, (annotate.COORD_MAX, annotate.COORD_MIN, 0, 0, 1, 1, 1, 255)]), 0)      # the legal extremes are taken
    assert an.wait() == 2


# ---------------------------------------------------------------------------------------------- 4. painter's order
def test_painters_order_is_the_jobs_and_not_the_schedules(an, mem):
    iw, ih = 97, 61
    src = padded(ra.PIX_BGRA, iw, ih, 4, 1006)
    ends = [(0, 30), (8, 0), (48, 0), (90, 2), (96, 14), (0, 50), (20, 60), (48, 60)]
    lines = [(x, y, 2 * 48 - x, 2 * 30 - y, 1 + k % 3) for k, (x, y) in enumerate(ends)]      # eight lines through (48, 30)
    fwd, rev = coloured(lines), coloured(lines)[::-1].copy()
    want_f, want_r = (annotate.draw(ra.PIX_BGRA, src, iw, ih, p) for p in (fwd, rev))
    assert tuple(want_f[0][30, 48 * 4:48 * 4 + 3]) == (fwd[7]["b"], fwd[7]["g"], fwd[7]["r"]) and tuple(want_r[0][30, 48 * 4:48 * 4 + 3]) == (fwd[0]["b"], fwd[0]["g"], fwd[0]["r"])
    for prims, want in ((fwd, want_f), (rev, want_r)):
        for _ in range(3):
            run(an, mem, ra.PIX_BGRA, src, iw, ih, prims, want=want, what="painter's order")
    assert not np.array_equal(want_f[0], want_r[0])


# ---------------------------------------------------------------------------------------------- 5. tile edges
@pytest.mark.parametrize("fmt", [ra.PIX_BGR, ra.PIX_RGBA, ra.PIX_NV12, ra.PIX_I420], ids=["BGR", "RGBA", "NV12", "I420"])
@pytest.mark.parametrize("mode", ["inplace", "dev2dev"])
def test_tile_edges(fmt, mode, an, mem):
    extra = 1 if fmt <= ra.PIX_RGBA else 2
    iw, ih = 3 * TW + extra, 2 * TH + extra
    src = padded(fmt, iw, ih, 3, 1007)
    lines = [(0, TH - 1, iw - 1, TH - 1, 1), (0, TH, iw - 1, TH, 1), (TW - 1, 0, TW - 1, ih - 1, 1), (TW, 0, TW, ih - 1, 1), (2 * TW - 1, 3, 2 * TW, 3, 1),
             (5, 2 * TH - 3, iw - 5, 2 * TH - 3, 6),      # a thick line astride the boundary between the second tile row and the last rows
             (TW - 3, 0, TW + 2, ih - 1, 5),               # a thick steep one along a tile column's edge
             (0, 10, 3 * TW, TH + 8, 1),                   # a shallow diagonal across all tiles of the width
             (iw - 1, 0, iw - 1, ih - 1, 1), (0, ih - 1, iw - 1, ih - 1, 1)]      # the frame's last column and row (tiles of one or two pixels)
    for l in lines:
        run(an, mem, fmt, src, iw, ih, coloured([l]), mode=mode, what="%s %s line %r" % (ra.PIX_NAMES[fmt], mode, l))
        mem.close()
    run(an, mem, fmt, src, iw, ih, coloured(lines), mode=mode)
    run(an, mem, fmt, src, iw, ih, coloured(lines), ra.ANNOT_CLEAR, mode=mode)


# ---------------------------------------------------------------------------------------------- 6. crowds
def random_segments(rng, n, x0, y0, x1, y1, reach, tmax):
    a = np.zeros(n, ra.PRIM_DTYPE)
    a["x0"], a["y0"] = rng.integers(x0, x1, n), rng.integers(y0, y1, n)
    a["x1"], a["y1"] = a["x0"] + rng.integers(-reach, reach + 1, n), a["y0"] + rng.integers(-reach, reach + 1, n)
    for c in ("b", "g", "r"):
        a[c] = rng.integers(0, 256, n)
    a["thickness"] = rng.integers(1, tmax + 1, n)
    return a


@pytest.mark.parametrize("fmt", [ra.PIX_BGR, ra.PIX_NV12], ids=["BGR", "NV12"])
def test_more_primitives_through_one_tile_than_a_chunk_holds(fmt, an, mem):
    iw, ih = size_for(fmt)
    src = padded(fmt, iw, ih, 1, 1008)
    n = 3 * CHUNK + 1
    prims = random_segments(np.random.default_rng(61), n, 2, 2, TW - 2, TH - 2, 12, 2)
    prims[n - 1] = (1, 1, TW - 2, TH - 2, 7, 77, 177, 1)      # the last one, alone in the fourth chunk, on top of all the others
    got = run(an, mem, fmt, src, iw, ih, prims)
    assert (annotate.owners(prims, iw, ih) == n - 1).sum() >= TH - 2
    for count in (CHUNK - 1, CHUNK, CHUNK + 1):
        run(an, mem, fmt, src, iw, ih, prims[:count], mode="dev2dev", what="%d primitives" % count)
        mem.close()


def test_a_full_job_and_empty_jobs(an, mem):
    iw, ih = 256, 128
    assert an.max_prims == 4096
    for fmt in (ra.PIX_RGB, ra.PIX_I420):
        src = padded(fmt, iw, ih, 0, 1009)
        prims = random_segments(np.random.default_rng(62), 4096, -10, -10, iw + 10, ih + 10, 14, 3)
        run(an, mem, fmt, src, iw, ih, prims, what="max_prims primitives")
        with pytest.raises(ValueError):
            Pending(mem, fmt, src, iw, ih, "inplace", 0).enqueue(an, np.concatenate([prims, prims[:1]]), 0)      # one more
        mem.close()
    for fmt in pixfmt.FORMATS:
        iw, ih = size_for(fmt)
        src = padded(fmt, iw, ih, 6, 1010 + fmt)
        for mode in ("inplace", "dev2dev", "host2pinned"):
            for flags in (0, ra.ANNOT_CLEAR):
                got = run(an, mem, fmt, src, iw, ih, annotate.prims([]), flags, mode=mode, what="%s n = 0, flags %d, %s" % (ra.PIX_NAMES[fmt], flags, mode))
                if mode == "inplace" and not flags:
                    assert_planes(got, src, "an empty job in place")
        mem.close()


# ---------------------------------------------------------------------------------------------- 7. formats and memory kinds
def mixed_prims(iw, ih):
    lines = [(3, 3, iw - 4, ih - 4, 1), (iw - 4, 3, 3, ih - 4, 2), (10, 40, 80, 44, 3), (50, 2, 54, 58, 4), (-20, 10, 40, 70, 1), (70, 50, 70, 50, 5), (0, 0, iw - 1, 0, 1),
             (0, ih - 1, iw - 1, ih - 1, 2), (20, 20, 20, 20, 1), (21, 21, 21, 21, 1),      # two points of different colours inside one 2 x 2 block: the later one gives the chroma
             (31, 20, 31, 20, 1), (30, 21, 30, 21, 1), (60, 10, 75, 25, 7), (62, 12, 90, 12, 1)]
    return coloured(lines)


@lru_cache(maxsize=None)
def format_case(fmt, iw, ih, flags):
    src = padded(fmt, iw, ih, 13, 2000 + fmt)
    prims = mixed_prims(iw, ih)
    return src, prims, annotate.draw(fmt, src, iw, ih, prims, clear=bool(flags))


@pytest.mark.parametrize("flags", [0, ra.ANNOT_CLEAR], ids=["draw", "clear"])
@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_every_format_and_every_way_a_frame_travels(fmt, flags, an, mem):
    sizes = [(98, 62)] + ([(97, 61)] if fmt <= ra.PIX_RGBA else [])
    for iw, ih in sizes:
        src, prims, want = format_case(fmt, iw, ih, flags)
        for mode in MODES:
            for out_pad in (0, 9):
                if mode == "inplace" and out_pad:
                    continue
                got = run(an, mem, fmt, src, iw, ih, prims, flags, mode=mode, out_pad=out_pad, want=want, what="%s %dx%d %s, flags %d, output padded by %d" % (ra.PIX_NAMES[fmt], iw, ih, mode, flags, out_pad))
                if fmt in (ra.PIX_BGRA, ra.PIX_RGBA):      # A is never written: in place it is the frame's own, out of place it came with the source's pixel
                    assert np.array_equal(got[0][:, 3:iw * 4:4], src[0][:, 3:iw * 4:4])
                if flags and fmt >= ra.PIX_NV12:
                    assert (got[0][:, :iw] == 16).sum() > iw * ih // 2 and (got[1][:, :iw // (1 if fmt == ra.PIX_NV12 else 2)] == 128).sum() > iw * ih // 8
            mem.close()


def test_the_chroma_rule(an, mem):
    """two primitives of different colours inside one 2 x 2 block: both luma pixels are drawn, the block's chroma is the later one's"""
    iw, ih = 98, 62
    for fmt in (ra.PIX_NV12, ra.PIX_I420):
        src = padded(fmt, iw, ih, 0, 1011)
        first, second = (20, 20, 20, 20, 255, 0, 0, 1), (21, 21, 21, 21, 0, 0, 255, 1)
        for rows in ([first, second], [second, first]):
            got = run(an, mem, fmt, src, iw, ih, annotate.prims(rows))
            ya, ua, va = (int(v) for v in annotate.yuv(*rows[0][4:7]))
            yb, ub, vb = (int(v) for v in annotate.yuv(*rows[1][4:7]))
            assert got[0][rows[0][1], rows[0][0]] == ya and got[0][rows[1][1], rows[1][0]] == yb
            uv = (got[1][10, 20], got[1][10, 21]) if fmt == ra.PIX_NV12 else (got[1][10, 10], got[2][10, 10])
            assert uv == (ub, vb) and (ua, va) != (ub, vb)


# ---------------------------------------------------------------------------------------------- 8. jobs in flight
def test_three_jobs_in_flight(mem):
    iw, ih = 98, 62
    a3 = ra.Annotator(max_prims=64, njobs=3)
    try:
        with pytest.raises(RuntimeError):
            a3.wait()
        jobs = []
        for k, (fmt, mode, flags) in enumerate([(ra.PIX_BGR, "inplace", 0), (ra.PIX_NV12, "host2pinned", ra.ANNOT_CLEAR), (ra.PIX_RGBA, "dev2dev", 0)]):
            src = padded(fmt, iw, ih, 2 + k, 1020 + k)
            prims = mixed_prims(iw, ih)[k:k + 5 + k]
            job = Pending(mem, fmt, src, iw, ih, mode, 4)
            assert job.enqueue(a3, prims, flags) == k
            jobs.append((job, fmt, src, prims, flags))
        for k, (job, fmt, src, prims, flags) in enumerate(jobs):
            assert a3.wait() == len(prims)
            assert_planes(job.result(), expected(fmt, src, iw, ih, prims, flags, job.out_init), "job %d of three in flight" % k)
        with pytest.raises(RuntimeError):
            a3.wait()
    finally:
        a3.close()


def test_one_job_too_many_is_fatal():
    """in a child process: the fourth enqueue with njobs = 3 and nothing waited for ends the process with a message, as the rectifier's does"""
    jobframes.assert_one_job_too_many_is_fatal("s = ra.Annotator(max_prims=4, njobs=3)\np = np.zeros(1, ra.PRIM_DTYPE); p['x1'] = 9; p['thickness'] = 1",
                                               "s.enqueue(ra.PIX_BGR, (d,), (64 * 3,), 64, 64, p, on_device=True)", "rd_annotator_enqueue")


def test_staging_buffers_grow_with_jobs_in_flight(mem):
    """host frames into pinned destinations: the second job's frame is larger than the first's and enqueued while that is in flight, the third is the small one again"""
    a2 = ra.Annotator(max_prims=64, njobs=2)
    try:
        jobs = []
        for k, (fmt, iw, ih) in enumerate([(ra.PIX_BGR, 34, 18), (ra.PIX_NV12, 98, 62), (ra.PIX_BGR, 34, 18)]):
            src = padded(fmt, iw, ih, 1 + k, 1040 + k)
            prims = coloured([(1, 1, iw - 2, ih - 2, 1), (iw - 3, 0, 2, ih - 1, 2), (-5, ih // 2, iw + 5, ih // 2 + 1, 3), (iw - 1, 0, iw - 1, ih - 1, 1)][k % 2:])
            jobs.append((Pending(mem, fmt, src, iw, ih, "host2pinned", 5 - k), fmt, src, iw, ih, prims))

        def check(job, n):
            pend, fmt, src, iw, ih, prims = job
            assert n == len(prims)
            assert_planes(pend.result(), expected(fmt, src, iw, ih, prims, 0, pend.out_init), "%s %dx%d" % (ra.PIX_NAMES[fmt], iw, ih))

        jobframes.growing_jobs(a2, jobs, lambda job: job[0].enqueue(a2, job[5], 0), check)
    finally:
        a2.close()


# ---------------------------------------------------------------------------------------------- 9. behind the poll
SIW, SIH = 640, 480
TAN36 = float(np.tan(36.0 / 180.0 * np.pi))


def test_annotate_polled_rectangles(mem):
    g = golden("rect_640x480_s0")
    frame = cframe(g["seed"], SIW, SIH, 0)
    src = [frame.reshape(SIH, SIW * 3)]
    want_prims = annotate.rects_prims(g["f0_rects"])
    assert len(want_prims) == 6 * len(g["f0_rects"]) > 0
    want = annotate.draw(ra.PIX_BGR, src, SIW, SIH, want_prims)
    an2 = ra.Annotator(max_prims=256, njobs=2)
    det = ra.Detector(SIW, SIH, nslots=1, aperture=float(g["tan_aov"]))
    try:
        out_init = padded(ra.PIX_BGR, SIW, SIH, 8, FILL)
        out = mem.put("pinned", out_init[0])
        with pytest.raises(ValueError):      # nothing polled yet
            det.annotate_polled(an2, want_prims, out_planes=(out,), out_pitches=(SIW * 3 + 8,), out_pinned=True)
        # a host frame: the detector's uploaded copy is the source, pinned memory the destination
        det.enqueue(frame)
        rects = det.poll(float(g["tan_aov"]))
        prims = ra.annot_rects(rects)
        assert prims.tobytes() == want_prims.tobytes(), "the polled rectangles give other primitives than the golden list"
        with pytest.raises(ValueError):      # a host frame without a destination
            det.annotate_polled(an2, prims)
        det.annotate_polled(an2, prims, out_planes=(out,), out_pitches=(SIW * 3 + 8,), out_pinned=True)
        assert an2.wait() == len(prims)
        exp = out_init[0].copy()
        exp[:, :SIW * 3] = want[0]
        assert_planes([mem.get("pinned", out, out_init[0].shape)], [exp], "host frame, pinned destination")
        # ... and the copy is still what the rectifier reads
        rect = ra.Rectifier(32, 32, max_quads=1, njobs=1)
        try:
            pd = mem.put("device", np.zeros(32 * 32 * 3, np.uint8))
            q = [(99.5, 99.5), (131.5, 99.5), (131.5, 131.5), (99.5, 131.5)]      # an axis-aligned quad at pixel pitch: the crop
            det.rectify_polled(rect, [q], pd)
            rect.wait()
            assert np.array_equal(mem.get("device", pd, (32, 32, 3)), frame[100:132, 100:132]), "the detector's copy of the host frame was drawn into"
        finally:
            rect.close()
        # a device frame, in place
        padded_frame = padded(ra.PIX_BGR, SIW, SIH, 4, [src[0]])
        dframe = mem.put("device", padded_frame[0])
        det.enqueue(dframe, ws=SIW * 3 + 4, on_device=True)
        rects = det.poll(float(g["tan_aov"]))
        prims = ra.annot_rects(rects)
        assert prims.tobytes() == want_prims.tobytes()
        det.annotate_polled(an2, prims)
        assert an2.wait() == len(prims)
        exp = padded_frame[0].copy()
        exp[:, :SIW * 3] = want[0]
        assert_planes([mem.get("device", dframe, exp.shape)], [exp], "device frame, in place")
        if L().rd_device_count() > 1:      # an annotator on another device
            other = ra.Annotator(max_prims=256, njobs=1, device=1)
            try:
                with pytest.raises(ValueError):
                    det.annotate_polled(other, prims)
            finally:
                other.close()
    finally:
        det.close()
        an2.close()


def test_annotate_polled_segments_both_modes_with_clear(mem):
    g = golden("rect_640x480_s0")
    frame = cframe(g["seed"], SIW, SIH, 0)
    src = [frame.reshape(SIH, SIW * 3)]
    an2 = ra.Annotator(max_prims=4096, njobs=1)
    det = ra.PolylineDetector(SIW, SIH, nslots=2)
    try:
        dsrc = mem.put("device", src[0])
        for mode in (ra.ANNOT_SEG_ALL, ra.ANNOT_SEG_CHAINS):
            det.enqueue(dsrc, ws=SIW * 3, on_device=True)
            segs, _ = det.poll()
            prims = ra.annot_segments(segs, mode)
            assert prims.tobytes() == annotate.segments_prims(segs, mode).tobytes() and len(prims) > 0
            out_init = padded(ra.PIX_BGR, SIW, SIH, 0, FILL)
            out = mem.put("device", out_init[0])
            det.annotate_polled(an2, prims, ra.ANNOT_CLEAR, out_planes=(out,), out_pitches=(SIW * 3,))
            assert an2.wait() == len(prims)
            want = annotate.draw(ra.PIX_BGR, src, SIW, SIH, prims, clear=True)
            got = mem.get("device", out, out_init[0].shape)
            assert_planes([got], want, "segments, mode %d, on black" % mode)
            assert 0 < (got != 0).sum() < got.size // 10
            assert np.array_equal(mem.get("device", dsrc, src[0].shape), src[0])
    finally:
        det.close()
        an2.close()


def test_annotate_polled_at_scale_2(mem):
    """a 1280 x 960 source detected at 640 x 480: the helpers at scale 2 give source coordinates, the frame is annotated at source size"""
    g = golden("rect_640x480_s0")
    sw, sh = 2 * SIW, 2 * SIH
    frame = cframe(g["seed"], sw, sh, 0)
    src = [frame.reshape(sh, sw * 3)]
    an2 = ra.Annotator(max_prims=1024, njobs=1)
    det = ra.Detector(SIW, SIH, nslots=1, aperture=TAN36)
    try:
        dsrc = mem.put("device", src[0])
        det.enqueue_scaled(ra.PIX_BGR, (dsrc,), (sw * 3,), on_device=True, scale=2)
        rects = det.poll(TAN36)
        prims = ra.annot_rects(rects, scale=2)
        assert prims.tobytes() == annotate.rects_prims(rects, 2).tobytes()
        segs = ra.annot_segments(det.last_segments(), ra.ANNOT_SEG_ALL, scale=2)
        assert len(segs) > 0 and (segs["thickness"] == 2).all()
        prims = np.concatenate([segs, prims])
        det.annotate_polled(an2, prims)
        assert an2.wait() == len(prims)
        want = annotate.draw(ra.PIX_BGR, src, sw, sh, prims)
        assert_planes([mem.get("device", dsrc, src[0].shape)], want, "scale 2, device frame in place")
        # the same frame from the host: into a destination of source size
        det.enqueue_scaled(ra.PIX_BGR, frame, scale=2)
        rects2 = det.poll(TAN36)
        assert helpers.rects_equal(rects, rects2)
        out_init = padded(ra.PIX_BGR, sw, sh, 0, FILL)
        out = mem.put("device", out_init[0])
        det.annotate_polled(an2, prims, out_planes=(out,), out_pitches=(sw * 3,))
        assert an2.wait() == len(prims)
        assert_planes([mem.get("device", out, out_init[0].shape)], want, "scale 2, host frame")
    finally:
        det.close()
        an2.close()


# ---------------------------------------------------------------------------------------------- 10. argument errors
def test_argument_errors_return_minus_one_and_the_next_job_is_correct(mem):
    iw, ih = 97, 61
    yw, yh = 98, 62
    src = padded(ra.PIX_BGR, iw, ih, 3, 1030)
    ysrc = padded(ra.PIX_NV12, yw, yh, 0, 1031)
    a1 = ra.Annotator(max_prims=8, njobs=1)
    dframe, pitch = mem.put("device", src[0]), src[0].shape[1]
    dy, duv = mem.put("device", ysrc[0]), mem.put("device", ysrc[1])
    out_init = padded(ra.PIX_BGR, iw, ih, 1, FILL)
    out, opitch = mem.put("device", out_init[0]), out_init[0].shape[1]
    pout = mem.put("pinned", out_init[0])
    pageable = np.zeros(out_init[0].size, np.uint8)
    prims = mixed_prims(iw, ih)[:8]
    bad_prim = prims.copy()
    bad_prim[5]["x1"] = 1048576
    zero_t = prims.copy()
    zero_t[7]["thickness"] = 0
    P, I = ctypes.c_void_p * 3, ctypes.c_int * 3

    def call(fmt=ra.PIX_BGR, pl=(dframe, None, None), pi=(pitch, 0, 0), w=iw, h=ih, kind=1, prims_p=prims.ctypes.data, n=len(prims), flags=0, opl=(out, None, None), opi=(opitch, 0, 0), out_kind=1):
        return L().rd_annotator_enqueue(a1.h, fmt, P(*pl), I(*pi), w, h, kind, prims_p, n, flags, P(*opl) if opl is not None else None, I(*opi) if opi is not None else None, out_kind)

    hostframe = np.ascontiguousarray(src[0])
    errors = {
        "unknown format": dict(fmt=6), "negative format": dict(fmt=-1),
        "unknown on_device": dict(kind=3), "unknown out_kind": dict(out_kind=0), "out_kind host": dict(out_kind=3),
        "unknown flag bits": dict(flags=2), "more unknown flag bits": dict(flags=ra.ANNOT_CLEAR | 4),
        "no width": dict(w=0), "no height": dict(h=0), "too wide": dict(w=65537), "too high": dict(h=65537),
        "NULL plane": dict(pl=(None, None, None)),
        "NULL chroma plane": dict(fmt=ra.PIX_NV12, pl=(dy, None, None), pi=(yw, yw, 0), w=yw, h=yh, opl=None),
        "NULL third plane": dict(fmt=ra.PIX_I420, pl=(dy, duv, None), pi=(yw, yw // 2, yw // 2), w=yw, h=yh, opl=None),
        "short pitch": dict(pi=(iw * 3 - 1, 0, 0)),
        "short chroma pitch": dict(fmt=ra.PIX_NV12, pl=(dy, duv, None), pi=(yw, yw - 1, 0), w=yw, h=yh, opl=None),
        "odd width with 4:2:0": dict(fmt=ra.PIX_NV12, pl=(dy, duv, None), pi=(yw, yw, 0), w=yw - 1, h=yh, opl=None),
        "odd height with 4:2:0": dict(fmt=ra.PIX_I420, pl=(dy, duv, duv), pi=(yw, yw, yw), w=yw, h=yh - 1, opl=None),
        "n < 0": dict(n=-1), "n > max_prims": dict(n=len(prims) + 1), "NULL prims": dict(prims_p=None),
        "a coordinate out of range": dict(prims_p=bad_prim.ctypes.data), "thickness 0": dict(prims_p=zero_t.ctypes.data),
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
            assert L().rd_annotator_wait(a1.h) == -1, name + ": nothing may have been enqueued"
        assert np.array_equal(mem.get("device", dframe, src[0].shape), src[0]) and np.array_equal(mem.get("device", out, out_init[0].shape), out_init[0])
        assert call() == 0      # the first job after all of them: sequence number 0, the right bytes
        assert a1.wait() == len(prims)
        assert_planes([mem.get("device", out, out_init[0].shape)], expected(ra.PIX_BGR, src, iw, ih, prims, 0, out_init), "the job after the refused ones")
        assert call(opl=None) == 1 and a1.wait() == len(prims)      # in place
        assert_planes([mem.get("device", dframe, src[0].shape)], expected(ra.PIX_BGR, src, iw, ih, prims, 0), "in place after the refused ones")
        for bad in ((-1, 1, 1), (0, 0, 1), (0, -5, 1), (0, (1 << 20) + 1, 1), (0, 1, 0), (0, 1, 1025), (L().rd_device_count(), 1, 1)):      # (device, max_prims, njobs)
            assert not L().rd_annotator_create(*bad), bad
        with pytest.raises(ValueError):
            ra.Annotator(max_prims=0)
    finally:
        a1.close()


# ---------------------------------------------------------------------------------------------- the convenience call
def test_annotate_convenience_call():
    frame = cframe(7, 320, 200, 0)
    prims = mixed_prims(320, 200)
    a = ra.Annotator(max_prims=64, njobs=1)
    try:
        got = a.annotate(frame, prims)
        assert got.shape == frame.shape
        assert np.array_equal(got.reshape(200, 960), annotate.draw(ra.PIX_BGR, [frame.reshape(200, 960)], 320, 200, prims)[0])
        black = a.annotate(frame, prims[:0], ra.ANNOT_CLEAR)
        assert not black.any()
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------- the example program
@pytest.mark.parametrize("poly", [False, True], ids=["rectangles", "poly"])
def test_rdannotate_writes_the_frames_the_binding_gives(poly, tmp_path):
    """examples/rdannotate on a YUV4MPEG2 stream of three frames: the stream that comes out holds, frame by frame, what the restatement draws into the I420 frame from
    the lists the binding's detector returns for it"""
    iw, ih, nframes = 640, 480, 3
    frames = [pixfmt.convert(cframe(0x5EED0000, iw, ih, t), ra.PIX_I420)[0] for t in range(nframes)]
    header = b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (iw, ih)
    with open(tmp_path / "in.y4m", "wb") as f:
        f.write(header)
        for planes in frames:
            f.write(b"FRAME\n" + b"".join(np.ascontiguousarray(p).tobytes() for p in planes))
    res = subprocess.run([os.path.join(helpers.ROOT, "examples", "rdannotate"), str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), "0"] + (["poly"] if poly else []),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path, timeout=120)
    assert res.returncode == 0, res.stderr.decode()
    data = open(tmp_path / "out.y4m", "rb").read()
    assert data.startswith(header)
    ny, nc = iw * ih, iw * ih // 4
    assert len(data) == len(header) + nframes * (6 + ny + 2 * nc)
    det = ra.PolylineDetector(iw, ih, nslots=1, strength_thre=2000, minerror=1.0, size_thre=10) if poly else ra.Detector(iw, ih, nslots=1)
    drawn = 0
    try:
        for t, planes in enumerate(frames):
            det.enqueue_planes(ra.PIX_I420, planes)
            prims = ra.annot_segments(det.poll()[0], ra.ANNOT_SEG_ALL) if poly else ra.annot_rects(det.poll(np.tan(72.0 / 2 / 180.0 * np.pi)))
            drawn += len(prims)
            src = [np.ascontiguousarray(p).reshape(rows, row) for p, (rows, row) in zip(planes, shapes(ra.PIX_I420, iw, ih))]
            want = annotate.draw(ra.PIX_I420, src, iw, ih, prims, clear=poly)
            at = len(header) + t * (6 + ny + 2 * nc)
            assert data[at:at + 6] == b"FRAME\n"
            got = np.frombuffer(data, np.uint8, ny + 2 * nc, at + 6)
            assert_planes([got[:ny].reshape(ih, iw), got[ny:ny + nc].reshape(ih // 2, iw // 2), got[ny + nc:].reshape(ih // 2, iw // 2)], want, "frame %d" % t)
    finally:
        det.close()
    assert drawn > 0 and ("%d primitive(s) drawn" % drawn) in res.stderr.decode()
