"""rd_detector_enqueue_planes on the GPU: frames in RGB, BGRA, RGBA, NV12 and I420 give exactly what the detector gives for the BGR frame of the conversion
contract (include/rectdetect_hip.h; restated in tests/pixfmt.py) - the front kernel's plab0 over every (Y, U, V) triple, and rectangle / segment lists over
streams in every frame kind, with 1, 2 and 64 slots, padded pitches and sizes that are no multiple of 4."""
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

pytestmark = pytest.mark.gpu
TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
L = ra.lib
NEW = (ra.PIX_RGB, ra.PIX_BGRA, ra.PIX_RGBA, ra.PIX_NV12, ra.PIX_I420)


@lru_cache(maxsize=4)
def stream(iw, ih, n, hard=0):
    """n frames of the synthetic stream (the C generator of synth.frame's stream, rd_synth.c), then `hard` of synth.hard_frame's stills"""
    out = []
    for t in range(n):
        a = np.empty((ih, iw, 3), np.uint8)
        L().rd_synth_frame(a.ctypes.data, iw, ih, iw * 3, synth.SEED0 + 11, t, 1)
        out.append(a)
    kinds = ("tiles", "waves", "bars", "noise")
    return tuple(out + [synth.hard_frame(kinds[k % 4], 50 + k, iw, ih) for k in range(hard)])


@lru_cache(maxsize=2)
def converted(iw, ih, n, hard, fmt):
    """[(planes, contract BGR frame)] of a stream in format fmt"""
    return tuple(pixfmt.convert(f, fmt) for f in stream(iw, ih, n, hard))


class Placer:
    """where device / pinned planes live: `nbuf` sets of planes, each plane in an allocation of its own (a UV plane apart from its Y plane), rows `align` bytes
    apart (None: rows back to back)"""

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


def enqueue_fn(det, items, fmts, kind, placer):
    """enqueue of frame i: items[i] = (planes, _) in format fmts[i] as a `kind` frame"""
    def enq(i):
        planes, _ = items[i]
        if kind == "host":
            return det.enqueue_planes(fmts[i], planes)
        ptrs, pitches = placer.put(i, planes)
        return det.enqueue_planes(fmts[i], ptrs, pitches, on_device=kind == "device", pinned=kind == "pinned")
    return enq


def rect_run(iw, ih, nslots, items, fmts, kind, align=None):
    """(rectangle lists, counters 16 + 17) of the stream through a rectangle detector"""
    det = ra.Detector(iw, ih, nslots=nslots, aperture=TAN36)
    placer = Placer(kind, nslots, align)
    try:
        res = drive(nslots, len(items), enqueue_fn(det, items, fmts, kind, placer), lambda: det.poll(TAN36))
        return res, L().rd_detector_counter(det.h, 16) + L().rd_detector_counter(det.h, 17)
    finally:
        det.close()
        placer.close()


def bgr_run(iw, ih, nslots, frames):
    """(rectangle lists, counters 16 + 17) of BGR frames through rd_detector_enqueue, driven in the same pattern"""
    det = ra.Detector(iw, ih, nslots=nslots, aperture=TAN36)
    try:
        res = drive(nslots, len(frames), lambda i: det.enqueue(frames[i]), lambda: det.poll(TAN36))
        return res, L().rd_detector_counter(det.h, 16) + L().rd_detector_counter(det.h, 17)
    finally:
        det.close()


@lru_cache(maxsize=None)
def rect_reference(iw, ih, n, hard, yuv, nslots):
    """bgr_run of the contract's BGR frames of stream(iw, ih, n, hard): the stream itself for the packed formats, its YUV 4:2:0 round trip for NV12 / I420"""
    return bgr_run(iw, ih, nslots, [r for _, r in converted(iw, ih, n, hard, ra.PIX_NV12 if yuv else ra.PIX_BGR)])


def assert_rect_lists(got, want):
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not helpers.rects_equal(a, b)]
    assert not bad, "frames whose rectangle list differs: %r" % bad[:10]
    assert sum(len(a) for a in got) > 0


def plab0_of(iw, ih, fmt, planes, kind="host", align=None):
    """plab0 of one frame through a one-slot polyline detector"""
    det = ra.PolylineDetector(iw, ih, nslots=1)
    placer = Placer(kind, 1, align)
    try:
        enqueue_fn(det, [(planes, None)], [fmt], kind, placer)(0)
        det.poll()
        return det.plane("plab0", np.uint32)
    finally:
        det.close()
        placer.close()


def plab0_bgr(iw, ih, bgr):
    det = ra.PolylineDetector(iw, ih, nslots=1)
    try:
        det.enqueue(bgr)
        det.poll()
        return det.plane("plab0", np.uint32)
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------------------------- 1. the conversion itself
@pytest.mark.parametrize("fmt", [ra.PIX_NV12, ra.PIX_I420])
def test_every_yuv_triple(fmt):
    """all 2^24 (Y, U, V) triples: four 2048x2048 frames, each (U, V) pair in 16 of the 2x2 blocks of a frame, its 4 x 16 x 4 Y values all 256"""
    S = 2048
    b = np.arange((S // 2) ** 2, dtype=np.int64).reshape(S // 2, S // 2)      # block index: (U, V) pair = b & 0xFFFF, repetition = b >> 16
    U, V = (b & 255).astype(np.uint8), ((b >> 8) & 255).astype(np.uint8)
    pair, rep = b & 0xFFFF, b >> 16
    for f in range(4):
        Y = np.empty((S, S), np.uint8)
        for j, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            Y[dy::2, dx::2] = ((f * 64 + rep * 4 + j + pair * 37) & 255).astype(np.uint8)
        planes = (Y, U, V) if fmt == ra.PIX_I420 else (Y, np.ascontiguousarray(np.stack([U, V], -1).reshape(S // 2, S)))
        want = plab0_bgr(S, S, pixfmt.i420_to_bgr(Y, U, V))
        got = plab0_of(S, S, fmt, planes)
        assert np.array_equal(got, want), "frame %d: %d pixels differ" % (f, int((got != want).sum()))


@pytest.mark.parametrize("iw,ih", [(1920, 1080), (1027, 38)])
@pytest.mark.parametrize("fmt", [ra.PIX_RGB, ra.PIX_BGRA, ra.PIX_RGBA])
def test_packed_formats_random_bytes(fmt, iw, ih):
    bgr = np.random.default_rng([fmt, iw]).integers(0, 256, (ih, iw, 3), dtype=np.uint8)
    (planes, ref) = pixfmt.convert(bgr, fmt)
    want = plab0_bgr(iw, ih, ref)
    assert np.array_equal(plab0_of(iw, ih, fmt, planes), want)
    assert np.array_equal(plab0_of(iw, ih, fmt, planes, "device"), want)


@pytest.mark.parametrize("align", [256, None])
@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_awkward_geometry_plab0(kind, align):
    """1282x722: iw no multiple of 4 (a chroma row of 641), planes in allocations of their own, rows 256-aligned or back to back (byte loads)"""
    iw, ih = 1282, 722
    bgr = synth.hard_frame("noise", 7, iw, ih)
    for fmt in NEW:
        planes, ref = pixfmt.convert(bgr, fmt)
        assert np.array_equal(plab0_of(iw, ih, fmt, planes, kind, align), plab0_bgr(iw, ih, ref)), ra.PIX_NAMES[fmt]


# ---------------------------------------------------------------------------------------------------------------- 2. rectangle kind, end to end
RECT_CASES = [      # (iw, ih, stream frames, hard stills, nslots, kind, formats)
    (1920, 1080, 64, 4, 64, "device", NEW),
    (1920, 1080, 64, 0, 64, "host", (ra.PIX_NV12, ra.PIX_RGBA)),
    (1920, 1080, 64, 0, 64, "pinned", (ra.PIX_NV12, ra.PIX_RGBA)),
    (1280, 720, 64, 2, 1, "host", (ra.PIX_NV12, ra.PIX_I420)),
    (1280, 720, 64, 0, 1, "pinned", (ra.PIX_I420,)),
    (1280, 720, 64, 2, 2, "device", (ra.PIX_NV12, ra.PIX_I420)),
    (1280, 720, 64, 0, 2, "pinned", (ra.PIX_NV12,)),
    (3840, 2160, 16, 0, 8, "device", (ra.PIX_NV12,)),
]


@pytest.mark.parametrize("iw,ih,n,hard,nslots,kind,fmts", RECT_CASES, ids=["%dx%d-%s-%dslots" % (c[0], c[1], c[5], c[4]) for c in RECT_CASES])
def test_rect_streams(iw, ih, n, hard, nslots, kind, fmts):
    for fmt in fmts:
        items = converted(iw, ih, n, hard, fmt)
        got, groups = rect_run(iw, ih, nslots, items, [fmt] * len(items), kind)
        want, want_groups = rect_reference(iw, ih, n, hard, fmt >= ra.PIX_NV12, nslots)
        assert_rect_lists(got, want)
        # the group path: as many group launches (rd_detector_counter 16 + 17) as the BGR stream driven in the same pattern
        assert groups == want_groups and (groups > 0 or nslots < 64), (ra.PIX_NAMES[fmt], groups, want_groups)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_mixed_formats_equal_bgr_stream(kind):
    """a stream that cycles through all six formats (their frames go frame by frame where a group mixes formats) equals the all-BGR stream"""
    iw, ih = 1280, 720
    base = stream(iw, ih, 72)
    # every frame through its YUV 4:2:0 round trip first, so that one BGR stream is the contract of all six formats; host frames change format from frame to
    # frame (every group mixes formats: frame by frame), device frames from group to group (group launches of each format, one after the other)
    items, fmts = [], []
    for i, f in enumerate(base):
        fmt = pixfmt.FORMATS[i % 6 if kind == "host" else (i // 8) % 6]
        yb = pixfmt.convert(f, ra.PIX_I420)[1]
        items.append(pixfmt.convert(f, fmt) if fmt >= ra.PIX_NV12 else pixfmt.convert(yb, fmt))
        fmts.append(fmt)
    got, groups = rect_run(iw, ih, 64, items, fmts, kind)
    want, want_groups = bgr_run(iw, ih, 64, [r for _, r in items])
    assert_rect_lists(got, want)
    assert groups == (0 if kind == "host" else want_groups) and want_groups > 0


@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_awkward_geometry_stream(kind):
    iw, ih = 1282, 722
    for fmt in NEW:
        items = converted(iw, ih, 12, 1, fmt)
        got, _ = rect_run(iw, ih, 2, items, [fmt] * len(items), kind, align=256)
        want, _ = rect_reference(iw, ih, 12, 1, fmt >= ra.PIX_NV12, 2)
        assert_rect_lists(got, want)


@pytest.mark.parametrize("kind", ["host", "device", "pinned"])
def test_bgr_through_planes_equals_enqueue(kind):
    iw, ih = 1920, 1080
    items = converted(iw, ih, 24, 0, ra.PIX_BGR)
    got, groups = rect_run(iw, ih, 8, items, [ra.PIX_BGR] * len(items), kind)
    want, want_groups = rect_reference(iw, ih, 24, 0, False, 8)
    assert_rect_lists(got, want)
    assert groups == want_groups


def test_argument_errors_enqueue_nothing():
    iw, ih = 640, 480
    f = stream(iw, ih, 3)
    det = ra.Detector(iw, ih, nslots=2, aperture=TAN36)
    ref = ra.Detector(iw, ih, nslots=2, aperture=TAN36)
    y, u, v = pixfmt.bgr_to_i420(f[0])
    Y = np.ascontiguousarray(y)
    P = lambda *ps: (ctypes.c_void_p * 3)(*(list(ps) + [None] * (3 - len(ps))))
    I = lambda *ps: (ctypes.c_int * 3)(*(list(ps) + [0] * (3 - len(ps))))
    call = lambda fmt, planes, pitches, kind=0: L().rd_detector_enqueue_planes(det.h, fmt, planes, pitches, kind)
    try:
        assert det.enqueue_planes(ra.PIX_BGR, f[0]) == 0
        bad = [
            (6, P(Y.ctypes.data), I(iw), 0), (-1, P(Y.ctypes.data), I(iw), 0),                                  # unknown format
            (ra.PIX_BGR, P(f[1].ctypes.data), I(iw * 3), 3), (ra.PIX_BGR, P(f[1].ctypes.data), I(iw * 3), -1),  # unknown on_device
            (ra.PIX_BGR, P(None), I(iw * 3), 0), (ra.PIX_NV12, P(Y.ctypes.data, None), I(iw, iw), 0),        # a NULL plane the format uses
            (ra.PIX_I420, P(Y.ctypes.data, u.ctypes.data, None), I(iw, iw // 2, iw // 2), 0),
            (ra.PIX_BGR, P(f[1].ctypes.data), I(iw * 3 - 1), 0), (ra.PIX_RGBA, P(f[1].ctypes.data), I(iw * 3), 0),   # pitch below the row
            (ra.PIX_NV12, P(Y.ctypes.data, u.ctypes.data), I(iw, iw - 2), 0), (ra.PIX_I420, P(Y.ctypes.data, u.ctypes.data, v.ctypes.data), I(iw, iw // 2 - 1, iw // 2), 0),
        ]
        for fmt, planes, pitches, kind in bad:
            assert call(fmt, planes, pitches, kind) == -1, (fmt, kind)
        with pytest.raises(ValueError):
            det.enqueue_planes(ra.PIX_NV12, (Y,), pitches=None)
        assert det.enqueue_planes(ra.PIX_I420, (y, u, v)) == 1      # the next valid frame: the next sequence number
        got = [det.poll(TAN36), det.poll(TAN36)]
        assert det.enqueue_planes(ra.PIX_BGR, f[2]) == 2
        got.append(det.poll(TAN36))
        want = drive(2, 3, lambda i: ref.enqueue([f[0], pixfmt.i420_to_bgr(y, u, v), f[2]][i]), lambda: ref.poll(TAN36))
        assert all(helpers.rects_equal(a, b) for a, b in zip(got, want))
    finally:
        det.close()
        ref.close()
    # odd sizes refuse the YUV formats
    odd = ra.Detector(643, 481, nslots=1)
    try:
        Yo = np.zeros((481, 643), np.uint8)
        assert L().rd_detector_enqueue_planes(odd.h, ra.PIX_NV12, P(Yo.ctypes.data, Yo.ctypes.data), I(643, 644), 0) == -1
        assert L().rd_detector_enqueue_planes(odd.h, ra.PIX_I420, P(Yo.ctypes.data, Yo.ctypes.data, Yo.ctypes.data), I(643, 322, 322), 0) == -1
    finally:
        odd.close()


@pytest.mark.parametrize("nslots", [1, 64])
def test_host_planes_may_be_overwritten_at_once(nslots):
    iw, ih = 1280, 720
    items = converted(iw, ih, 64, 0, ra.PIX_NV12)
    det = ra.Detector(iw, ih, nslots=nslots, aperture=TAN36)
    try:
        def enq(i):
            y, uv = (p.copy() for p in items[i][0])
            det.enqueue_planes(ra.PIX_NV12, (y, uv))
            y[:] = 255 - y      # the call has returned: the detector owns a copy
            uv[:] = 0
        got = drive(nslots, len(items), enq, lambda: det.poll(TAN36))
    finally:
        det.close()
    assert_rect_lists(got, rect_reference(iw, ih, 64, 0, True, nslots)[0])


# ---------------------------------------------------------------------------------------------------------------- 3. polyline kind
POLY_CASES = [(1920, 1080, 64, "device", ra.PIX_NV12), (1280, 720, 8, "host", ra.PIX_RGBA), (1280, 720, 2, "pinned", ra.PIX_I420), (1280, 720, 1, "device", ra.PIX_RGB)]


@pytest.mark.parametrize("iw,ih,nslots,kind,fmt", POLY_CASES)
def test_polyline_streams(iw, ih, nslots, kind, fmt):
    items = converted(iw, ih, 64, 2, fmt)
    det = ra.PolylineDetector(iw, ih, nslots=nslots)
    ref = ra.PolylineDetector(iw, ih, nslots=nslots)
    placer = Placer(kind, nslots)
    try:
        ids = lambda d: (lambda: d.poll(ids=True))
        got = drive(nslots, len(items), enqueue_fn(det, items, [fmt] * len(items), kind, placer), ids(det))
        want = drive(nslots, len(items), lambda i: ref.enqueue(items[i][1]), ids(ref))
    finally:
        det.close()
        ref.close()
        placer.close()
    for i, ((sa, ia), (sb, ib)) in enumerate(zip(got, want)):
        assert helpers.segments_equal(sa, sb), i
        assert np.array_equal(ia, ib), i
    assert sum(int(s.view("i4")[0]) for s, _ in got) > 0


# ---------------------------------------------------------------------------------------------------------------- the example
def test_rdy4m_matches_binding(tmp_path):
    iw, ih, n = 1280, 720, 24
    frames = [pixfmt.bgr_to_i420(f) for f in stream(iw, ih, n, 2)]
    path = str(tmp_path / "s.y4m")
    pixfmt.write_y4m(path, frames, iw, ih)
    exe = os.path.join(helpers.ROOT, "examples", "rdy4m")
    r = subprocess.run([exe, path, "0", "72", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    counts = [int(l.split(":")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("frame ")]
    det = ra.Detector(iw, ih, nslots=4)
    tan72 = float(np.tan(72.0 / 2 / 180.0 * np.pi))
    try:
        want = drive(4, len(frames), lambda i: det.enqueue_planes(ra.PIX_I420, frames[i]), lambda: det.poll(tan72))
    finally:
        det.close()
    assert counts == [len(w) for w in want]
    assert sum(counts) > 0
