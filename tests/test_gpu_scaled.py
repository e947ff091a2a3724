"""rd_detector_enqueue_scaled on the GPU: a source frame of 2 iw x 2 ih pixels in any of the six formats gives exactly what the detector gives for the BGR frame
of the contract (include/rectdetect_hip.h): half() below of the conversion contract's full-size BGR frame - the front kernel's plab0 over random bytes, rectangle
and segment lists over streams in every frame kind with 1, 2, 8 and 64 slots, mixed scales in one stream, argument errors, the copy contract of host frames,
the scaled-source staging (counter 33), patches cut from the full-size source, and examples/rdy4m's `half` option.  No tolerance anywhere."""
import ctypes
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers
from tests import pixfmt
from tests import rectify

pytestmark = pytest.mark.gpu
TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
L = ra.lib
SW, SH, IW, IH = 1284, 724, 642, 362      # the streams' source and detector size: iw = 642 is no multiple of 4 (and 1284 none of 8), ih = 362 none of 64


def half(a):
    """the contract: 2x2 box average of a full-size BGR frame, (sum + 2) >> 2 per channel in int32"""
    a = a.astype(np.int32)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- frames
@lru_cache(maxsize=4)
def stream(sw, sh, n, hard=0):
    """n frames of synth.frame's stream at the SOURCE size, then `hard` of synth.hard_frame's stills"""
    kinds = ("tiles", "waves", "bars", "noise")
    return tuple([synth.frame(synth.SEED0 + 11, sw, sh, t) for t in range(n)] + [synth.hard_frame(kinds[k % 4], 50 + k, sw, sh) for k in range(hard)])


@lru_cache(maxsize=8)
def converted(sw, sh, n, hard, fmt):
    """[(source planes in format fmt, the contract's half-size BGR frame, the contract's full-size BGR frame)] of stream(sw, sh, n, hard)"""
    out = []
    for f in stream(sw, sh, n, hard):
        planes, full = pixfmt.convert(f, fmt)
        out.append((planes, half(full), full))
    return tuple(out)


def random_source(fmt, sw, sh, seed):
    """planes of uniformly random bytes (NV12 / I420: independent Y, U and V planes - four different Y under one U, V pair, the clamps of the conversion hit)"""
    rng = np.random.default_rng([seed, fmt, sw, sh])
    if fmt in (ra.PIX_BGR, ra.PIX_RGB):
        return (rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8),)
    if fmt in (ra.PIX_BGRA, ra.PIX_RGBA):
        return (rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8),)
    Y = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    U, V = (rng.integers(0, 256, (sh // 2, sw // 2), dtype=np.uint8) for _ in range(2))
    if fmt == ra.PIX_I420:
        return (Y, U, V)
    return (Y, np.ascontiguousarray(np.stack([U, V], -1).reshape(sh // 2, sw)))


# ---------------------------------------------------------------------------------------------------------------- driving
class Placer:
    """where device / pinned planes live: `nbuf` sets of planes, each plane in an allocation of its own, rows `align` bytes apart (None: rows back to back)"""

    def __init__(self, kind, nbuf, align=None):
        self.kind, self.nbuf, self.align, self.bufs = kind, nbuf, align, {}

    def put(self, i, planes):
        ptrs, pitches = [], []
        for k, p in enumerate(planes):
            p = np.ascontiguousarray(p)
            rows, row = p.shape[0], p.size // p.shape[0]
            pitch = row if self.align is None else (row + self.align - 1) // self.align * self.align
            img = np.zeros((rows, pitch), np.uint8)
            img[:, :row] = p.reshape(rows, row)
            key = (i % self.nbuf, k)
            if key not in self.bufs or self.bufs[key][1] < img.nbytes:
                if key in self.bufs:
                    self._free(self.bufs[key][0])
                self.bufs[key] = (L().rd_device_alloc(img.nbytes) if self.kind == "device" else L().rd_host_alloc(img.nbytes), img.nbytes)
            ptr = self.bufs[key][0]
            if self.kind == "device":
                L().rd_upload(ptr, img.ctypes.data, img.nbytes)
            else:
                ctypes.memmove(ptr, img.ctypes.data, img.nbytes)
            ptrs.append(ptr)
            pitches.append(pitch)
        return ptrs, pitches

    def _free(self, p):
        (L().rd_device_free if self.kind == "device" else L().rd_host_free)(p)

    def close(self):
        for p, _ in self.bufs.values():
            self._free(p)
        self.bufs = {}


def drive(nslots, n, enqueue, poll):
    """frames 0..n-1 with the slots kept full (the oldest polled once they are): the results in order"""
    out, inflight = [], 0
    for i in range(n):
        if inflight == nslots:
            out.append(poll())
            inflight -= 1
        enqueue(i)
        inflight += 1
    while inflight:
        out.append(poll())
        inflight -= 1
    return out


def enqueue_fn(det, items, fmts, scales, kind, placer):
    """enqueue of frame i: items[i][0] = planes in format fmts[i] at scale scales[i], as a `kind` frame"""
    def enq(i):
        planes = items[i][0]
        if kind == "host":
            return det.enqueue_scaled(fmts[i], planes, scale=scales[i])
        ptrs, pitches = placer.put(i, planes)
        return det.enqueue_scaled(fmts[i], ptrs, pitches, on_device=kind == "device", pinned=kind == "pinned", scale=scales[i])
    return enq


def groups_of(det):
    return L().rd_detector_counter(det.h, 16) + L().rd_detector_counter(det.h, 17)


def rect_run(iw, ih, nslots, items, fmts, scales, kind, align=None):
    """(rectangle lists, counters 16 + 17) of the stream through a rectangle detector"""
    det = ra.Detector(iw, ih, nslots=nslots, aperture=TAN36)
    placer = Placer(kind, nslots, align)
    try:
        res = drive(nslots, len(items), enqueue_fn(det, items, fmts, scales, kind, placer), lambda: det.poll(TAN36))
        return res, groups_of(det)
    finally:
        det.close()
        placer.close()


def bgr_run(iw, ih, nslots, frames):
    """(rectangle lists, counters 16 + 17) of BGR frames through rd_detector_enqueue, driven in the same pattern"""
    det = ra.Detector(iw, ih, nslots=nslots, aperture=TAN36)
    try:
        res = drive(nslots, len(frames), lambda i: det.enqueue(frames[i]), lambda: det.poll(TAN36))
        return res, groups_of(det)
    finally:
        det.close()


@lru_cache(maxsize=None)
def rect_reference(n, hard, yuv, nslots):
    """bgr_run of half() of the contract's frames of stream(SW, SH, n, hard): of the stream itself for the packed formats, of its 4:2:0 round trip for NV12 / I420"""
    return bgr_run(IW, IH, nslots, [h for _, h, _ in converted(SW, SH, n, hard, ra.PIX_NV12 if yuv else ra.PIX_BGR)])


def assert_rect_lists(got, want):
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not helpers.rects_equal(a, b)]
    assert not bad, "frames whose rectangle list differs: %r" % bad[:10]
    assert sum(len(a) for a in got) > 0


# ---------------------------------------------------------------------------------------------------------------- 1. the arithmetic alone
@pytest.mark.parametrize("iw,ih", [(321, 181), (64, 64)])
@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_plab0_equals_the_box_average(fmt, iw, ih):
    """plab0 through a one-slot polyline detector: 321x181 from 642x362 - groups of fewer than 4 at the row end, a partial tile in both directions, RGB rows of 1926
    bytes (the byte path) - and exactly one tile; host, device and pinned frames, rows back to back and 256 bytes apart"""
    planes = random_source(fmt, 2 * iw, 2 * ih, 3)
    full = rectify.contract_bgr(fmt, planes)
    det = ra.PolylineDetector(iw, ih, nslots=1)
    try:
        def plab0_bgr(bgr):
            det.enqueue(np.ascontiguousarray(bgr))
            det.poll()
            return det.plane("plab0", np.uint32)
        want = plab0_bgr(half(full))
        one_tap = plab0_bgr(full[0::2, 0::2])
        assert not np.array_equal(want, one_tap)      # a kernel that takes one tap must not pass
        for kind, align in (("host", None), ("device", None), ("device", 256), ("pinned", None), ("pinned", 256)):
            placer = Placer(kind, 1, align)
            try:
                enqueue_fn(det, [(planes,)], [fmt], [2], kind, placer)(0)
                det.poll()
                got = det.plane("plab0", np.uint32)
            finally:
                placer.close()
            assert np.array_equal(got, want), "%s, %s frame, align %r: %d pixels differ" % (ra.PIX_NAMES[fmt], kind, align, int((got != want).sum()))
            assert not np.array_equal(got, one_tap)
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------------------------- 2. rectangle kind, end to end
@pytest.mark.parametrize("nslots,kind", [(2, "device"), (2, "pinned"), (64, "device"), (64, "host")])
def test_rect_streams(nslots, kind):
    for fmt in (ra.PIX_BGR, ra.PIX_BGRA, ra.PIX_NV12):
        items = converted(SW, SH, 12, 1, fmt)
        got, groups = rect_run(IW, IH, nslots, items, [fmt] * len(items), [2] * len(items), kind)
        want, want_groups = rect_reference(12, 1, fmt >= ra.PIX_NV12, nslots)
        assert_rect_lists(got, want)
        if nslots == 64 and kind == "device":      # the group path was taken: as many group launches as the BGR stream driven in the same pattern
            assert groups == want_groups and groups > 0, (ra.PIX_NAMES[fmt], groups, want_groups)


# ---------------------------------------------------------------------------------------------------------------- 3. mixed scales in one stream
@pytest.mark.parametrize("kind", ["host", "device"])
def test_mixed_scales_equal_bgr_stream(kind):
    """frames alternate between scale 1 (640x360 planes) and scale 2 (1280x720 planes) and cycle through the formats - host frames from frame to frame (every group
    mixes: frame by frame), device frames from group to group (group launches of each layout, one after the other); the result is that of the all-BGR stream"""
    iw, ih, n = 640, 360, 64
    items, fmts, scales = [], [], []
    for i, f in enumerate(stream(2 * iw, 2 * ih, n)):
        g = i // 8
        scale, fmt = (1 + i % 2, pixfmt.FORMATS[(i // 2) % 6]) if kind == "host" else (1 + (g + g // 6) % 2, pixfmt.FORMATS[g % 6])
        if scale == 2:
            planes, full = pixfmt.convert(f, fmt)
            items.append((planes, half(full)))
        else:
            items.append(pixfmt.convert(half(f), fmt))
        fmts.append(fmt)
        scales.append(scale)
    got, groups = rect_run(iw, ih, 64, items, fmts, scales, kind)
    want, want_groups = bgr_run(iw, ih, 64, [r for _, r in items])
    assert_rect_lists(got, want)
    assert groups == (0 if kind == "host" else want_groups) and want_groups > 0


# ---------------------------------------------------------------------------------------------------------------- 4. polyline kind
@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("fmt", [ra.PIX_NV12, ra.PIX_RGB], ids=["NV12", "RGB"])
def test_polyline_streams(fmt, kind):
    items = converted(SW, SH, 12, 1, fmt)
    det = ra.PolylineDetector(IW, IH, nslots=8)
    ref = ra.PolylineDetector(IW, IH, nslots=8)
    placer = Placer(kind, 8)
    try:
        ids = lambda d: (lambda: d.poll(ids=True))
        got = drive(8, len(items), enqueue_fn(det, items, [fmt] * len(items), [2] * len(items), kind, placer), ids(det))
        want = drive(8, len(items), lambda i: ref.enqueue(items[i][1]), ids(ref))
    finally:
        det.close()
        ref.close()
        placer.close()
    for i, ((sa, ia), (sb, ib)) in enumerate(zip(got, want)):
        assert helpers.segments_equal(sa, sb), i
        assert np.array_equal(ia, ib), i
    assert sum(int(s.view("i4")[0]) for s, _ in got) > 0


# ---------------------------------------------------------------------------------------------------------------- 5. argument errors
def test_argument_errors_enqueue_nothing():
    iw, ih = 322, 182      # from 644 x 364 frames
    items = converted(2 * iw, 2 * ih, 3, 0, ra.PIX_I420)
    bgr = [np.ascontiguousarray(f) for f in stream(2 * iw, 2 * ih, 3)]
    (y, u, v) = (np.ascontiguousarray(p) for p in items[1][0])
    sw = 2 * iw
    det = ra.Detector(iw, ih, nslots=2, aperture=TAN36)
    ref = ra.Detector(iw, ih, nslots=2, aperture=TAN36)
    P = lambda *ps: (ctypes.c_void_p * 3)(*(list(ps) + [None] * (3 - len(ps))))
    I = lambda *ps: (ctypes.c_int * 3)(*(list(ps) + [0] * (3 - len(ps))))
    call = lambda fmt, planes, pitches, scale, kind=0: L().rd_detector_enqueue_scaled(det.h, fmt, planes, pitches, scale, kind)
    try:
        assert det.enqueue_scaled(ra.PIX_BGR, bgr[0]) == 0
        b1 = bgr[1].ctypes.data
        bad = [(ra.PIX_BGR, P(b1), I(sw * 3), s, 0) for s in (0, 3, 4, -1)]                                                   # unknown scale
        bad += [(ra.PIX_BGR, P(None), I(sw * 3), 2, 0), (ra.PIX_NV12, P(y.ctypes.data, None), I(sw, sw), 2, 0),                # a NULL plane the format uses
                (ra.PIX_I420, P(y.ctypes.data, u.ctypes.data, None), I(sw, sw // 2, sw // 2), 2, 0)]
        bad += [(ra.PIX_BGR, P(b1), I(iw * 3), 2, 0), (ra.PIX_BGRA, P(b1), I(iw * 4), 2, 0), (ra.PIX_NV12, P(y.ctypes.data, u.ctypes.data), I(iw, iw), 2, 0),   # pitches[0] = iw * bpp: enough for scale 1, too small for scale 2
                (ra.PIX_BGR, P(b1), I(sw * 3 - 1), 2, 0), (ra.PIX_I420, P(y.ctypes.data, u.ctypes.data, v.ctypes.data), I(sw, sw // 2 - 1, sw // 2), 2, 0)]
        bad += [(6, P(b1), I(sw * 3), 2, 0), (-1, P(b1), I(sw * 3), 2, 0)]                                                     # unknown format
        bad += [(ra.PIX_BGR, P(b1), I(sw * 3), 2, 3), (ra.PIX_BGR, P(b1), I(sw * 3), 2, -1)]                                   # unknown on_device
        for fmt, planes, pitches, scale, kind in bad:
            assert call(fmt, planes, pitches, scale, kind) == -1, (fmt, scale, kind)
        with pytest.raises(ValueError):
            det.enqueue_scaled(ra.PIX_BGR, bgr[1], scale=3)
        with pytest.raises(ValueError):      # the binding checks host planes against the source size
            det.enqueue_scaled(ra.PIX_BGR, bgr[1][:ih, :iw])
        assert det.enqueue_scaled(ra.PIX_I420, (y, u, v)) == 1      # the next valid frame: the sequence number that was due
        got = [det.poll(TAN36), det.poll(TAN36)]
        assert det.enqueue_scaled(ra.PIX_BGR, bgr[2]) == 2
        got.append(det.poll(TAN36))
        frames = [half(bgr[0]), items[1][1], half(bgr[2])]
        want = drive(2, 3, lambda i: ref.enqueue(frames[i]), lambda: ref.poll(TAN36))
        assert all(helpers.rects_equal(a, b) for a, b in zip(got, want))
        # scale 1 is enqueue_planes on the same planes, list for list
        small = [pixfmt.convert(half(f), fmt) for f, fmt in zip(bgr, (ra.PIX_NV12, ra.PIX_RGBA, ra.PIX_BGR))]
        fm = [ra.PIX_NV12, ra.PIX_RGBA, ra.PIX_BGR]
        a = drive(2, 3, lambda i: det.enqueue_scaled(fm[i], small[i][0], scale=1), lambda: det.poll(TAN36))
        b = drive(2, 3, lambda i: ref.enqueue_planes(fm[i], small[i][0]), lambda: ref.poll(TAN36))
        assert all(helpers.rects_equal(p, q) for p, q in zip(a, b))
    finally:
        det.close()
        ref.close()


# ---------------------------------------------------------------------------------------------------------------- 6. copy contract
@pytest.mark.parametrize("nslots", [1, 64])
def test_host_planes_may_be_overwritten_at_once(nslots):
    items = converted(SW, SH, 12, 1, ra.PIX_NV12)
    det = ra.Detector(IW, IH, nslots=nslots, aperture=TAN36)
    try:
        def enq(i):
            y, uv = (p.copy() for p in items[i][0])
            det.enqueue_scaled(ra.PIX_NV12, (y, uv))
            y[:] = 255 - y      # the call has returned: the detector owns a copy
            uv[:] = 0
        got = drive(nslots, len(items), enq, lambda: det.poll(TAN36))
    finally:
        det.close()
    assert_rect_lists(got, rect_reference(12, 1, True, nslots)[0])


# ---------------------------------------------------------------------------------------------------------------- 7. staging
def test_scaled_staging_is_allocated_on_first_host_frame_only():
    items = converted(SW, SH, 12, 1, ra.PIX_NV12)
    fresh = ra.Detector(IW, IH, nslots=2, aperture=TAN36)
    det = ra.Detector(IW, IH, nslots=2, aperture=TAN36)
    placer = Placer("device", 2)
    ctr = lambda d, k: L().rd_detector_counter(d.h, k)
    try:
        slot_bytes = ctr(fresh, 31)
        assert ctr(fresh, 33) == 0
        for i in range(3):
            enqueue_fn(det, items, [ra.PIX_NV12] * 3, [2] * 3, "device", placer)(i)
            det.poll(TAN36)
        assert ctr(det, 33) == 0 and ctr(det, 31) == slot_bytes      # device frames are read in place: nothing allocated
        det.enqueue_scaled(ra.PIX_NV12, items[3][0])
        got = det.poll(TAN36)
        assert ctr(det, 33) > 0 and ctr(det, 31) == slot_bytes
        # (a frame's result depends on the frame before it - the strong mask it starts from - so the reference takes the same four frames the same way)
        want = drive(1, 4, lambda i: fresh.enqueue(items[i][1]), lambda: fresh.poll(TAN36))
        assert helpers.rects_equal(got, want[3]) and ctr(fresh, 33) == 0
    finally:
        det.close()
        fresh.close()
        placer.close()


# ---------------------------------------------------------------------------------------------------------------- 8. patches from the full-size source
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("fmt", [ra.PIX_BGR, ra.PIX_NV12], ids=["BGR", "NV12"])
def test_rectify_polled_reads_the_full_size_source(fmt, kind):
    PW, PH = 64, 48
    items = converted(SW, SH, 3, 0, fmt)
    det = ra.Detector(IW, IH, nslots=1, aperture=TAN36)
    rectifier = ra.Rectifier(PW, PH, max_quads=64, njobs=1)
    placer = Placer(kind, 1)
    out = L().rd_device_alloc(64 * PW * PH * 3)

    def job(quads):
        det.rectify_polled(rectifier, quads, out)
        status = rectifier.wait()
        a = np.zeros(len(quads) * PW * PH * 3, np.uint8)
        L().rd_download(a.ctypes.data, out, a.nbytes)
        return a.reshape(len(quads), PH, PW, 3), status

    total = 0
    try:
        for i, (planes, small, full) in enumerate(items):
            enqueue_fn(det, items, [fmt] * len(items), [2] * len(items), kind, placer)(i)
            rects = det.poll(TAN36)
            quads = ra.rect_quads(rects).reshape(-1, 8)
            assert 0 < len(quads) <= 64
            assert np.array_equal(quads.reshape(-1, 4, 2), rectify.rect_quads(rects))
            got, status = job(quads)
            want, wstatus = rectify.patches(full, quads * 2.0 + 0.5, PW, PH)
            assert np.array_equal(status, wstatus) and (status == 1).all()
            assert np.array_equal(got, want), "frame %d: %d patches differ" % (i, sum(not np.array_equal(a, b) for a, b in zip(got, want)))
            assert not np.array_equal(got, rectify.patches(small, quads, PW, PH)[0])      # the source was read, not the half-size frame
            total += len(quads)
            if i == 0:      # a quad that reaches outside the frame: the clamp uses the source's size
                outside = np.array([[IW - 40.0, IH - 30.0, IW + 60.0, IH - 30.0, IW + 60.0, IH + 50.0, IW - 40.0, IH + 50.0], [-20.0, -10.0, 30.0, -10.0, 30.0, 25.0, -20.0, 25.0]])
                got, status = job(outside)
                want, wstatus = rectify.patches(full, outside * 2.0 + 0.5, PW, PH)
                assert np.array_equal(status, wstatus) and np.array_equal(got, want)
                assert not np.array_equal(got, rectify.patches(small, outside, PW, PH)[0])
        assert total > 0
    finally:
        rectifier.close()
        det.close()
        placer.close()
        L().rd_device_free(out)


# ---------------------------------------------------------------------------------------------------------------- 9. the example
def test_rdy4m_half_matches_binding(tmp_path):
    n = 12
    frames = [pixfmt.bgr_to_i420(f) for f in stream(SW, SH, n, 1)]
    path = str(tmp_path / "s.y4m")
    pixfmt.write_y4m(path, frames, SW, SH)
    exe = os.path.join(helpers.ROOT, "examples", "rdy4m")
    r = subprocess.run([exe, path, "0", "72", "4", "half"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    counts = [int(l.split(":")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("frame ")]
    det = ra.Detector(IW, IH, nslots=4)
    tan72 = float(np.tan(72.0 / 2 / 180.0 * np.pi))
    try:
        want = drive(4, len(frames), lambda i: det.enqueue_scaled(ra.PIX_I420, frames[i]), lambda: det.poll(tan72))
    finally:
        det.close()
    assert counts == [len(w) for w in want]
    assert sum(counts) > 0
