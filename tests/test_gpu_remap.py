"""Remapped frames on the GPU (rd_remapper): every output equals, in every byte and with the destination's pitch padding untouched, the numpy restatement of the
header's contract (tests/remap.py) applied to the BGR frame the conversion contract gives for the source (tests/rectify.py: contract_bgr) - all six pixel formats,
host / pinned / device sources, device / pinned output, row tails and misaligned destinations, clamped taps, outside entries, jobs in flight, both creators,
argument errors, and the hand-over to the detector and the rectifier.  No tolerance anywhere."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers
from tests import jobframes
from tests import pixfmt
from tests import rectify
from tests import remap
from tests.jobframes import L

pytestmark = pytest.mark.gpu
FORMATS = [ra.PIX_BGR, ra.PIX_RGB, ra.PIX_BGRA, ra.PIX_RGBA, ra.PIX_NV12, ra.PIX_I420]
OW, OH = 83, 59


@pytest.fixture
def mem():
    m = jobframes.Mem()
    yield m
    m.close()


def source_size(fmt):
    return (97, 61) if fmt <= ra.PIX_RGBA else (98, 62)      # NV12 and I420 need even sizes


@lru_cache(maxsize=None)
def source(fmt, iw, ih, seed=77):
    """(planes of a random frame in format fmt, the BGR frame the conversion contract gives for them)"""
    bgr = np.random.default_rng(seed + iw).integers(0, 256, (ih, iw, 3), dtype=np.uint8)
    planes, _ = pixfmt.convert(bgr, fmt)
    return planes, rectify.contract_bgr(fmt, planes)


def barrel(iw, ih):
    """a barrel lens on an iw x ih source and a view of OW x OH that leaves an outside border"""
    return ra.lens(0.6 * iw, 0.61 * iw, (iw - 1) / 2 + 0.3, (ih - 1) / 2 - 0.2, k1=-0.25), ra.view(0.42 * OW, 0.43 * OW, (OW - 1) / 2, (OH - 1) / 2)


@lru_cache(maxsize=None)
def barrel_table(iw, ih):
    table, n = remap.table_lens(*barrel(iw, ih), OW, OH, iw, ih)
    assert 0 < n < OW * OH and (table[0, OW // 2] == -1).all() and (table[OH // 2, OW // 2] >= 0).all()
    return table, n


def pattern(n):
    return (np.arange(n, dtype=np.int64) * 7 % 251).astype(np.uint8)


def run_job(remapper, mem, fmt, planes, want, kind="device", out_kind="device", pad=0, offset=0, fill=(0, 0, 0), src_pad=5, what=""):
    """one job, waited for: the whole destination buffer - the bytes before `out`, the rows, their pitch padding - must be its pattern with the wanted rows in it"""
    job = start_job(remapper, mem, fmt, planes, kind, out_kind, pad, offset, fill, src_pad)
    remapper.wait()
    finish_job(mem, job, want, what)


def start_job(remapper, mem, fmt, planes, kind, out_kind, pad, offset, fill, src_pad=5):
    ow, oh = remapper.ow, remapper.oh
    args, pitches, kw = mem.place(kind, planes, src_pad)
    pitch = 3 * ow + pad
    init = pattern(offset + oh * pitch)
    p = mem.put(out_kind, init)
    remapper.enqueue(fmt, args, pitches, kw["on_device"], p + offset, pitch, fill, pinned=kw["pinned"], out_pinned=out_kind == "pinned")
    return out_kind, p, init, pitch, offset


def finish_job(mem, job, want, what=""):
    out_kind, p, init, pitch, offset = job
    oh, ow = want.shape[:2]
    exp = init.copy()
    for v in range(oh):
        exp[offset + v * pitch: offset + v * pitch + 3 * ow] = want[v].reshape(-1)
    got = mem.get(out_kind, p, init.shape)
    if not np.array_equal(got, exp):
        bad = np.nonzero(got != exp)[0]
        k = int(bad[0]) - offset
        raise AssertionError("%s: %d bytes differ, first at row %d byte %d (%s): got %d, expected %d" % (
            what, len(bad), k // pitch, k % pitch, "padding" if k < 0 or k % pitch >= 3 * ow else "pixel %d" % (k % pitch // 3), got[bad[0]], exp[bad[0]]))


@pytest.mark.parametrize("kind", ["host", "pinned", "device"])
@pytest.mark.parametrize("fmt", FORMATS, ids=[ra.PIX_NAMES[f] for f in FORMATS])
def test_formats_and_sources(fmt, kind, mem):
    iw, ih = source_size(fmt)
    planes, bgr = source(fmt, iw, ih)
    table, n = barrel_table(iw, ih)
    fill = (201, 17, 94)
    want = remap.apply(bgr, table, OW, OH, fill)
    lens, view = barrel(iw, ih)
    r = ra.Remapper(OW, OH, iw, ih, lens=lens, view=view, njobs=2)
    try:
        assert r.inside == n
        run_job(r, mem, fmt, planes, want, kind, "device", pad=7, fill=fill, what="%s from %s memory" % (ra.PIX_NAMES[fmt], kind))
    finally:
        r.close()


def random_maps(ow, oh, iw, ih, seed):
    """float32 maps of random positions, one in eight outside"""
    rng = np.random.default_rng(seed)
    mx = rng.uniform(0.0, iw - 1.0, (oh, ow)).astype(np.float32)
    my = rng.uniform(0.0, ih - 1.0, (oh, ow)).astype(np.float32)
    mx[rng.random((oh, ow)) < 0.125] = -3.0
    return np.minimum(mx, np.float32(iw - 1)), np.minimum(my, np.float32(ih - 1))


@pytest.mark.parametrize("oh", [1, 9])
@pytest.mark.parametrize("ow", [1, 2, 3, 4, 5, 33])
def test_row_tails_and_alignment(ow, oh, mem):
    iw, ih = 13, 7
    planes, bgr = source(ra.PIX_BGR, iw, ih)
    mx, my = random_maps(ow, oh, iw, ih, 100 * ow + oh)
    table, n = remap.table_map(mx, my, ow, oh, iw, ih)
    want = remap.apply(bgr, table, ow, oh, (9, 8, 7))
    r = ra.Remapper(ow, oh, iw, ih, maps=(mx, my), njobs=2)
    try:
        assert r.inside == n
        for pad in (0, 5):
            for offset in (0, 1, 2, 3):
                for out_kind in ("device", "pinned") if offset == 0 else ("device",):
                    run_job(r, mem, ra.PIX_BGR, planes, want, "device", out_kind, pad, offset, (9, 8, 7), what="%dx%d, out_pitch 3*ow+%d, out at +%d, %s" % (ow, oh, pad, offset, out_kind))
    finally:
        r.close()


def test_clamped_taps(mem):
    """entries on the last column and the last row (x1, y1 clamped) and in the last cell, with every fraction of 0, 1, 128 and 255"""
    iw, ih = 13, 7
    planes, bgr = source(ra.PIX_BGR, iw, ih)
    fr = [0.0, 1.0 / 256, 128.0 / 256, 255.0 / 256]
    pos = [(iw - 1.0, y + f) for y in (0.0, 3.0, ih - 2.0) for f in fr] + [(x + f, ih - 1.0) for x in (0.0, 5.0, iw - 2.0) for f in fr] + [(iw - 1.0, ih - 1.0)]
    pos += [(iw - 2.0 + fx, ih - 2.0 + fy) for fx in fr for fy in fr]
    ow, oh = len(pos), 1
    mx, my = np.array([p[0] for p in pos], np.float32), np.array([p[1] for p in pos], np.float32)
    table, n = remap.table_map(mx, my, ow, oh, iw, ih)
    assert n == ow and set((table[0, :, 0] & 255).tolist()) == {0, 1, 128, 255} and table[0, :, 0].max() == 256 * (iw - 1) and table[0, :, 1].max() == 256 * (ih - 1)
    r = ra.Remapper(ow, oh, iw, ih, maps=(mx, my))
    try:
        run_job(r, mem, ra.PIX_BGR, planes, remap.apply(bgr, table, ow, oh, (0, 0, 0)), what="clamped taps")
    finally:
        r.close()
    # a 2 x 2 NV12 source to 8 x 8: every tap of every pixel is a border tap, and the four pixels share one chroma sample
    planes, bgr = source(ra.PIX_NV12, 2, 2)
    v, u = np.mgrid[0:8, 0:8]
    mx, my = (u / 7.0).astype(np.float32), (v / 7.0).astype(np.float32)
    table, n = remap.table_map(mx, my, 8, 8, 2, 2)
    assert n == 64
    r = ra.Remapper(8, 8, 2, 2, maps=(mx, my))
    try:
        run_job(r, mem, ra.PIX_NV12, planes, remap.apply(bgr, table, 8, 8, (0, 0, 0)), kind="host", what="2x2 NV12 to 8x8")
    finally:
        r.close()


def test_outside_entries(mem):
    iw, ih = 13, 7
    planes, bgr = source(ra.PIX_BGR, iw, ih)
    # entirely outside: all fill
    ow, oh = 37, 5
    mx = np.full((oh, ow), -5.0, np.float32)
    r = ra.Remapper(ow, oh, iw, ih, maps=(mx, mx))
    try:
        assert r.inside == 0
        want = np.broadcast_to(np.array([1, 254, 77], np.uint8), (oh, ow, 3))
        run_job(r, mem, ra.PIX_BGR, planes, want, fill=(1, 254, 77), what="all outside")
    finally:
        r.close()
    # every pattern of inside and outside within one thread's 4 pixels: group g of a row has pixel k inside when bit k of g is set; the next row the complement
    ow, oh = 64, 2
    v, u = np.mgrid[0:oh, 0:ow]
    inside = (((u // 4) >> (u % 4)) & 1).astype(bool) ^ (v == 1)
    mx, my = random_maps(ow, oh, iw, ih, 5)
    mx, my = np.where(inside, np.abs(mx), np.float32(np.nan)).astype(np.float32), my
    table, n = remap.table_map(mx, my, ow, oh, iw, ih)
    assert n == ow * oh // 2 and np.array_equal(table[..., 0] >= 0, inside)
    r = ra.Remapper(ow, oh, iw, ih, maps=(mx, my))
    try:
        assert r.inside == n
        run_job(r, mem, ra.PIX_BGR, planes, remap.apply(bgr, table, ow, oh, (250, 3, 128)), fill=(250, 3, 128), what="checkerboards")
    finally:
        r.close()


def test_four_jobs_in_flight_to_pinned_and_device_memory(mem):
    iw, ih = 98, 62
    lens, view = barrel(iw, ih)
    table, _ = barrel_table(iw, ih)
    r = ra.Remapper(OW, OH, iw, ih, lens=lens, view=view, njobs=4)
    try:
        jobs = []
        for k, (fmt, kind, out_kind) in enumerate([(ra.PIX_NV12, "device", "pinned"), (ra.PIX_BGR, "host", "device"), (ra.PIX_I420, "pinned", "pinned"), (ra.PIX_RGBA, "device", "device")]):
            planes, bgr = source(fmt, iw, ih, seed=200 + k)
            fill = (10 + k, 100 + k, 200 + k)
            jobs.append((start_job(r, mem, fmt, planes, kind, out_kind, 4 * k + 1, 0, fill), remap.apply(bgr, table, OW, OH, fill)))
        for k, (job, want) in enumerate(jobs):
            r.wait()
            finish_job(mem, job, want, "job %d of four in flight" % k)
        with pytest.raises(RuntimeError):
            r.wait()
    finally:
        r.close()


def test_one_job_too_many_is_fatal():
    jobframes.assert_one_job_too_many_is_fatal("s = ra.Remapper(64, 64, 64, 64, lens=ra.lens(64, 64, 32, 32), njobs=3)\no = ra.lib().rd_device_alloc(64 * 64 * 3)",
                                               "s.enqueue(ra.PIX_BGR, (d,), (192,), True, o, 192)", "rd_remapper_enqueue")


def test_both_creators_agree_through_float32_maps(mem):
    """create_map from the float32 maps of the restatement's points gives the output of the table the restatement builds from those float32 maps: the rounding
    to float32 is part of the contract (and the table differs from the lens's own)"""
    iw, ih = 97, 61
    planes, bgr = source(ra.PIX_RGB, iw, ih)
    lens, view = barrel(iw, ih)
    XY = remap.points(lens, view, remap.grid(OW, OH)).astype(np.float32)
    table, n = remap.table_map(XY[:, 0], XY[:, 1], OW, OH, iw, ih)
    assert not np.array_equal(table, barrel_table(iw, ih)[0])
    r = ra.Remapper(OW, OH, iw, ih, maps=(XY[:, 0], XY[:, 1]))
    try:
        assert r.inside == n
        run_job(r, mem, ra.PIX_RGB, planes, remap.apply(bgr, table, OW, OH, (5, 6, 7)), fill=(5, 6, 7), what="create_map")
    finally:
        r.close()


def test_argument_errors(mem):
    iw, ih = 98, 62
    lens, view = barrel(iw, ih)
    planes, bgr = source(ra.PIX_NV12, iw, ih)
    (y, uv), pitches, _ = mem.place("device", planes, 0)
    pitch = 3 * OW + 1
    init = pattern(OH * pitch)
    out, pinned_out = mem.put("device", init), mem.put("pinned", init)
    pageable = init.copy()
    r = ra.Remapper(OW, OH, iw, ih, lens=lens, view=view, njobs=2)
    P3, I3 = ctypes.c_void_p * 3, ctypes.c_int * 3
    try:
        raw = lambda fmt, pl, pi, kind, o, op, ok: L().rd_remapper_enqueue(r.h, fmt, P3(*pl), I3(*pi), kind, 0x112233, o, op, ok)
        good = (ra.PIX_NV12, (y, uv, None), (pitches[0], pitches[1], 0), 1, out, pitch, 1)
        for what, change in [("format 6", {0: 6}), ("format -1", {0: -1}), ("NULL plane 0", {1: (None, uv, None)}), ("NULL plane 1", {1: (y, None, None)}),
                             ("short pitch 0", {2: (iw - 1, iw, 0)}), ("short pitch 1", {2: (iw, iw - 1, 0)}), ("on_device 3", {3: 3}), ("NULL out", {4: None}),
                             ("short out_pitch", {5: 3 * OW - 1}), ("out_kind 0", {6: 0}), ("out_kind 3", {6: 3}), ("pageable out as device", {4: pageable.ctypes.data}),
                             ("pageable out as pinned", {4: pageable.ctypes.data, 6: 2}), ("device out as pinned", {6: 2}), ("pinned out as device", {4: pinned_out})]:
            a = list(good)
            for k, v in change.items():
                a[k] = v
            assert raw(*a) == -1, what
        assert L().rd_remapper_enqueue(r.h, ra.PIX_NV12, None, I3(iw, iw, 0), 1, 0, out, pitch, 1) == -1 and L().rd_remapper_enqueue(r.h, ra.PIX_NV12, P3(y, uv, None), None, 1, 0, out, pitch, 1) == -1
        with pytest.raises(ValueError):
            r.enqueue(ra.PIX_NV12, (y, uv), pitches, True, out, 3 * OW - 1)
        # nothing was enqueued, nothing written
        with pytest.raises(RuntimeError):
            r.wait()
        assert np.array_equal(mem.get("device", out, init.shape), init) and np.array_equal(mem.get("pinned", pinned_out, init.shape), init) and np.array_equal(pageable, init)
        # ... and the good call is good
        assert raw(*good) == 0
        r.wait()
        finish_job(mem, ("device", out, init, pitch, 0), remap.apply(bgr, barrel_table(iw, ih)[0], OW, OH, (0x33, 0x22, 0x11)), "after the refused calls")
    finally:
        r.close()
    # create: NULL for each argument error of the tables, a bad device, a bad njobs
    lp, vp = lens.ctypes.data, view.ctypes.data
    mx = np.zeros(OW * OH, np.float32)
    cl, cm = L().rd_remapper_create_lens, L().rd_remapper_create_map
    assert not cl(0, None, vp, OW, OH, iw, ih, 2) and not cl(0, lp, None, OW, OH, iw, ih, 2)
    assert not cm(0, None, mx.ctypes.data, OW, OH, iw, ih, 2) and not cm(0, mx.ctypes.data, None, OW, OH, iw, ih, 2)
    for bad in ((0, OH, iw, ih), (OW, 0, iw, ih), (16385, OH, iw, ih), (OW, 16385, iw, ih), (OW, OH, 0, ih), (OW, OH, iw, 0), (OW, OH, 65537, ih), (OW, OH, iw, 65537), (-1, -1, -1, -1)):
        assert not cl(0, lp, vp, *bad, 2) and not cm(0, mx.ctypes.data, mx.ctypes.data, *bad, 2), bad
    for field, v in [("k1", np.nan), ("fx", np.inf), ("cy", -np.inf), ("k3", np.nan)]:
        l = lens.copy()
        l[field] = v
        assert not cl(0, l.ctypes.data, vp, OW, OH, iw, ih, 2), field
    for field, v in [("fx", 0.0), ("fy", -0.0), ("cx", np.nan), ("fy", np.inf)]:
        w = view.copy()
        w[field] = v
        assert not cl(0, lp, w.ctypes.data, OW, OH, iw, ih, 2), field
    for device, njobs in ((-1, 2), (L().rd_device_count(), 2), (0, 0), (0, -1), (0, 1025)):
        assert not cl(device, lp, vp, OW, OH, iw, ih, njobs) and not cm(device, mx.ctypes.data, mx.ctypes.data, OW, OH, iw, ih, njobs), (device, njobs)
    with pytest.raises(ValueError):
        ra.Remapper(OW, OH, iw, ih, lens=lens, view=ra.view(0.0, 1.0, 0.0, 0.0))
    assert L().rd_remapper_inside(None) == -1


# ---- end to end: a bent frame, remapped on the device, handed to the detector and to the rectifier behind its poll
EW, EH = 640, 480      # the smallest size the detector's own tests run synthetic frames at
PW, PH = 48, 32


def bend(img, lens, view):
    """`img` as a camera with this lens would have seen it, roughly: every pixel of the bent picture takes the nearest pixel of `img` at the position that a few
    rounds of x <- xd / rad(x) give for the inverse of the lens's radial term.  Any resampling will do - this only has to produce a bent picture."""
    ih, iw = img.shape[:2]
    Y, X = np.mgrid[0:ih, 0:iw].astype(np.float64)
    xd, yd = (X - float(lens["cx"])) / float(lens["fx"]), (Y - float(lens["cy"])) / float(lens["fy"])
    x, y = xd.copy(), yd.copy()
    for _ in range(20):
        r2 = x * x + y * y
        rad = 1.0 + float(lens["k1"]) * r2
        x, y = xd / rad, yd / rad
    u = np.rint(x * float(view["fx"]) + float(view["cx"])).astype(np.int64)
    v = np.rint(y * float(view["fy"]) + float(view["cy"])).astype(np.int64)
    ok = (u >= 0) & (u < iw) & (v >= 0) & (v < ih)
    out = np.zeros_like(img)
    out[ok] = img[v[ok], u[ok]]
    return out


def detect(frame, tan_aov, ws=None, on_device=False):
    det = ra.Detector(EW, EH, nslots=1)
    try:
        det.enqueue(frame, ws=ws, on_device=on_device)
        return det, det.poll(tan_aov)
    except Exception:
        det.close()
        raise


def test_end_to_end_remap_detect_rectify(mem):
    lens = ra.lens(500.0, 500.0, (EW - 1) / 2, (EH - 1) / 2, k1=-0.2)
    view = ra.view(500.0, 500.0, (EW - 1) / 2, (EH - 1) / 2)
    tan_aov = ra.view_tan_aov(view, EW)
    assert tan_aov == 320.0 / 500.0
    original = synth.frame(synth.SEED0, EW, EH, 0)
    bent = bend(original, lens, view)
    table, n = remap.table_lens(lens, view, EW, EH, EW, EH)
    want = remap.apply(bent, table, EW, EH, (0, 0, 0))
    assert not np.array_equal(bent, original) and not np.array_equal(want, bent)

    pitch = 3 * EW + 8
    init = pattern(EH * pitch)
    out = mem.put("device", init)
    r = ra.Remapper(EW, EH, EW, EH, lens=lens, view=view, njobs=2)
    rectifier = ra.Rectifier(PW, PH, max_quads=64, njobs=1)
    det = ref = None
    try:
        assert r.inside == n
        r.enqueue(ra.PIX_BGR, bent, None, False, out, pitch)
        r.wait()
        finish_job(mem, ("device", out, init, pitch, 0), want, "the remapped frame")
        det, rects = detect(out, tan_aov, ws=pitch, on_device=True)
        ref, wrects = detect(want, tan_aov)
        assert len(wrects) > 0, "the remapped synthetic frame holds no rectangle: the test shows nothing"
        assert helpers.rects_equal(rects, wrects), (len(rects), len(wrects))
        # the rectifier behind the poll reads the undistorted frame in place
        quads = ra.rect_quads(rects)
        pout = mem.out("device", len(quads) * PW * PH * 3)
        det.rectify_polled(rectifier, quads, pout)
        status = rectifier.wait()
        wpatches, wstatus = rectify.patches(want, quads, PW, PH)
        assert np.array_equal(status, wstatus)
        assert np.array_equal(mem.fetch("device", pout, len(quads) * PW * PH * 3).reshape(wpatches.shape), wpatches)
        # (recorded, not asserted: what the lens costs the detector - profiles/NOTES_remap.md)
        counts = {}
        for name, img in (("bent", bent), ("original", original)):
            d, rs = detect(img, tan_aov)
            d.close()
            counts[name] = len(rs)
        print("\nend to end at %dx%d, k1 = %g: rectangles on the bent frame %d, on the remapped frame %d, on the undistorted original %d" % (
            EW, EH, float(lens["k1"]), counts["bent"], len(rects), counts["original"]))
    finally:
        for s in (det, ref, rectifier, r):
            if s is not None:
                s.close()
