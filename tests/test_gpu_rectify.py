"""Rectified patches on the GPU (rd_rectifier, rd_detector_rectify_polled): every patch equals, in every byte, the numpy float64 restatement of the header's
contract (tests/rectify.py) - for the reference's own rectangles, all six pixel formats, host / device / pinned frames, device / pinned output, patch sizes with
and without a row tail, jobs in flight, empty and full jobs, invalid quads, argument errors, and behind the poll of both detector kinds.  No tolerance anywhere."""
import ctypes
import os
from functools import lru_cache

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers
from tests import jobframes
from tests import pixfmt
from tests import rectify
from tests.jobframes import L, cframe
from tests.rectjobs import TAN36, mem, noise_frame, stream_frames      # (mem: the fixture)

pytestmark = pytest.mark.gpu


def golden(name):
    return np.load(os.path.join(helpers.GOLDEN, name + ".npz"), allow_pickle=False)


def run_job(rect, mem, fmt, planes, iw, ih, quads, kind="host", out_kind="device", pad=0):
    """one job, waited for: ((n, ph, pw, 3) patches, status)"""
    q = np.asarray(quads, np.float64).reshape(-1, 8)
    nbytes = len(q) * rect.ph * rect.pw * 3
    args, pitches, kw = mem.place(kind, planes, pad)
    out = mem.out(out_kind, nbytes)
    rect.enqueue(fmt, args, pitches, iw, ih, q, out, out_pinned=out_kind == "pinned", **kw)
    status = rect.wait()
    return mem.fetch(out_kind, out, nbytes).reshape(len(q), rect.ph, rect.pw, 3), status


def assert_patches(got, status, want, wstatus, what=""):
    assert np.array_equal(status, wstatus), "%s: status %r, expected %r" % (what, status.tolist(), wstatus.tolist())
    assert got.shape == want.shape
    bad = [k for k in range(len(want)) if not np.array_equal(got[k], want[k])]
    assert not bad, "%s: patches %r differ (patch %d in %d bytes)" % (what, bad[:10], bad[0], int((got[bad[0]] != want[bad[0]]).sum()))


# ---------------------------------------------------------------------------------------------- anchor: no restatement involved
@pytest.mark.parametrize("x0,y0", [(37, 21), (0, 0), (333 - 64, 217 - 64)])
def test_axis_aligned_quad_at_pixel_pitch_is_the_crop(x0, y0, mem):
    iw, ih = 333, 217
    frame = noise_frame(iw, ih)
    crop = frame[y0:y0 + 64, x0:x0 + 64]
    a, b = (x0 - 0.5, y0 - 0.5), (x0 + 63.5, y0 + 63.5)
    cw = [a, (b[0], a[1]), b, (a[0], b[1])]          # s along x, t along y
    ccw = [a, (a[0], b[1]), b, (b[0], a[1])]         # s along y, t along x: the transpose
    rect = ra.Rectifier(64, 64, max_quads=2, njobs=1)
    try:
        got, status = run_job(rect, mem, ra.PIX_BGR, (frame,), iw, ih, [cw, ccw])
        assert status.tolist() == [1, 1]
        assert np.array_equal(got[0], crop)
        assert np.array_equal(got[1].transpose(1, 0, 2), crop)
        conv = rect.rectify(frame, [cw, ccw])      # the convenience call: through pinned memory
        assert conv.shape == (2, 64, 64, 3) and np.array_equal(conv, got)
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- the reference's rectangles
def golden_jobs():
    """(name, frame, rectangles) for frame 0 of rect_1920x1080_s0, the frames of stream_1280x720_s1 and the stills of hard_rect (empty lists included)"""
    g = golden("rect_1920x1080_s0")
    yield "rect_1920x1080_s0 f0", cframe(g["seed"], 1920, 1080, 0), g["f0_rects"]
    g = golden("stream_1280x720_s1")
    for t in range(int(g["nframes"])):
        yield "stream_1280x720_s1 f%d" % t, cframe(g["seed"], 1280, 720, t), g["f%d_rects" % t]
    g = golden("hard_rect")
    for k, (kind, (seed, iw, ih)) in enumerate(zip(g["kinds"].tolist(), g["params"].tolist())):
        yield "hard_rect h%d" % k, synth.hard_frame(kind, seed, iw, ih), g["h%d_rects" % k]


def test_quads_from_the_reference_match_numpy(mem):
    rect = ra.Rectifier(64, 64, max_quads=80, njobs=1)
    total = outside = empty = 0
    try:
        for name, frame, rects in golden_jobs():
            ih, iw = frame.shape[:2]
            quads = ra.rect_quads(rects)
            got, status = run_job(rect, mem, ra.PIX_BGR, (frame,), iw, ih, quads, kind="device")
            want, wstatus = rectify.patches(frame, quads, 64, 64)
            assert_patches(got, status, want, wstatus, name)
            assert status.all()
            total += len(quads)
            empty += len(quads) == 0
            outside += int(((quads[..., 0] < 0) | (quads[..., 0] > iw - 1) | (quads[..., 1] < 0) | (quads[..., 1] > ih - 1)).any(axis=1).sum())
            mem.close()
    finally:
        rect.close()
    print("golden quads rectified: %d, reaching outside their frame: %d, empty lists: %d" % (total, outside, empty))
    assert total > 400 and outside > 0 and empty > 0


# ---------------------------------------------------------------------------------------------- formats, frame kinds, output kinds, patch sizes
def small_quads(iw, ih):
    """convex quads in a small frame: rotated, in perspective, the other orientation, reaching outside on every side, larger than the frame, smaller than a pixel"""
    w, h = float(iw), float(ih)
    return np.array([
        [(40.25, 30.5), (200.75, 12.0), (230.0, 150.5), (25.5, 120.0)],
        [(25.5, 120.0), (230.0, 150.5), (200.75, 12.0), (40.25, 30.5)],
        [(-20.0, -15.5), (90.0, -4.0), (70.5, 60.0), (-9.0, 44.0)],
        [(w - 60.0, h - 50.0), (w + 25.5, h - 70.0), (w + 11.0, h + 30.0), (w - 80.0, h + 8.25)],
        [(-50.0, -40.0), (w + 50.0, -60.0), (w + 70.0, h + 45.0), (-30.0, h + 80.0)],
        [(100.1, 100.2), (100.9, 100.3), (100.8, 100.95), (100.05, 100.8)],
        [(150.0, 20.0), (300.0, 90.0), (170.0, 200.0), (120.0, 110.0)],
    ], np.float64)


@lru_cache(maxsize=None)
def small_case(fmt):
    """(iw, ih, planes, the contract's BGR frame, quads) - 333 x 217 for the packed formats, 334 x 218 for 4:2:0"""
    iw, ih = (333, 217) if fmt <= ra.PIX_RGBA else (334, 218)
    planes, bgr = pixfmt.convert(noise_frame(iw, ih, 11 + fmt), fmt)
    assert np.array_equal(rectify.contract_bgr(fmt, planes), bgr)
    return iw, ih, planes, bgr, small_quads(iw, ih)


@lru_cache(maxsize=None)
def small_reference(fmt, pw, ph):
    iw, ih, planes, bgr, quads = small_case(fmt)
    return rectify.patches(bgr, quads, pw, ph)


@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_every_format_frame_kind_output_kind_and_patch_size(fmt, mem):
    iw, ih, planes, bgr, quads = small_case(fmt)
    for pw, ph in ((64, 64), (100, 60), (31, 17)):
        want, wstatus = small_reference(fmt, pw, ph)
        assert wstatus.all()
        rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=2)
        try:
            for kind in ("host", "device", "pinned"):
                for out_kind in ("device", "pinned"):
                    for pad in (0, 13):
                        got, status = run_job(rect, mem, fmt, planes, iw, ih, quads, kind, out_kind, pad)
                        assert_patches(got, status, want, wstatus, "%s %dx%d %s frame, %s output, pad %d" % (ra.PIX_NAMES[fmt], pw, ph, kind, out_kind, pad))
        finally:
            rect.close()
        mem.close()


def test_yuv_formats_equal_the_contracts_bgr_frame_on_the_device(mem):
    """the header's claim itself, GPU against GPU: the patch from NV12 / I420 planes is the patch from the BGR frame the conversion contract gives"""
    rect = ra.Rectifier(100, 60, max_quads=8, njobs=1)
    try:
        for fmt in (ra.PIX_NV12, ra.PIX_I420):
            iw, ih, planes, bgr, quads = small_case(fmt)
            a, _ = run_job(rect, mem, fmt, planes, iw, ih, quads, "device")
            b, _ = run_job(rect, mem, ra.PIX_BGR, (bgr,), iw, ih, quads, "device")
            assert np.array_equal(a, b)
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- jobs in flight, empty and full jobs
@pytest.mark.parametrize("njobs", [1, 4])
def test_jobs_in_flight_come_back_in_order(njobs, mem):
    iw, ih, planes, bgr, quads = small_case(ra.PIX_BGR)
    pw, ph = 64, 64
    want, _ = small_reference(ra.PIX_BGR, pw, ph)
    rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=njobs)
    args, pitches, kw = mem.place("device", planes, 5)
    subsets = [list(range(len(quads)))[k % 3:k % 3 + 1 + k % 5] for k in range(11)]      # every job another selection of the quads
    pending, checked = [], 0
    try:
        for k, sel in enumerate(subsets):
            if len(pending) == njobs:
                s0, out0, kind0 = pending.pop(0)
                status = rect.wait()
                got = mem.fetch(kind0, out0, len(s0) * pw * ph * 3).reshape(len(s0), ph, pw, 3)
                assert_patches(got, status, want[s0], np.ones(len(s0), np.uint8), "job %d" % checked)
                checked += 1
            out_kind = "device" if k % 2 == 0 else "pinned"
            out = mem.out(out_kind, len(sel) * pw * ph * 3)
            assert rect.enqueue(ra.PIX_BGR, args, pitches, iw, ih, quads[sel], out, out_pinned=out_kind == "pinned", **kw) == k
            pending.append((sel, out, out_kind))
        while pending:
            s0, out0, kind0 = pending.pop(0)
            status = rect.wait()
            got = mem.fetch(kind0, out0, len(s0) * pw * ph * 3).reshape(len(s0), ph, pw, 3)
            assert_patches(got, status, want[s0], np.ones(len(s0), np.uint8), "job %d" % checked)
            checked += 1
        assert checked == len(subsets)
        with pytest.raises(RuntimeError):
            rect.wait()      # nothing in flight
    finally:
        rect.close()


def test_one_job_too_many_is_fatal():
    """in a child process: the fourth enqueue with njobs = 3 and nothing waited for ends the process with a message"""
    jobframes.assert_one_job_too_many_is_fatal("s = ra.Rectifier(8, 8, max_quads=1, njobs=3)\no = ra.lib().rd_device_alloc(8 * 8 * 3)\nq = [[(4, 4), (40, 4), (40, 40), (4, 40)]]",
                                               "s.enqueue(ra.PIX_BGR, (d,), (64 * 3,), 64, 64, q, o, on_device=True)", "rd_rectifier_enqueue")


def test_staging_buffers_grow_with_jobs_in_flight(mem):
    """host frames, pinned output: the second job's frame is larger than the first's and enqueued while that is in flight, the third is the small one again"""
    pw, ph = 16, 12
    rect = ra.Rectifier(pw, ph, max_quads=3, njobs=2)
    try:
        jobs = []
        for k, (fmt, iw, ih, nq) in enumerate([(ra.PIX_BGR, 34, 18, 1), (ra.PIX_NV12, 98, 62, 3), (ra.PIX_BGR, 34, 18, 2)]):
            planes, bgr = pixfmt.convert(noise_frame(iw, ih, 50 + k), fmt)
            w, h = float(iw), float(ih)
            quads = np.array([[(2.5, 1.25), (w - 4.0, 3.0), (w - 5.5, h - 2.0), (4.0, h - 3.5)], [(-6.0, -4.0), (w * 0.6, -2.5), (w * 0.5, h * 0.7), (-3.0, h * 0.5)],
                              [(w * 0.4, h * 0.3), (w + 7.0, h * 0.2), (w + 3.0, h + 5.0), (w * 0.3, h + 2.0)]])[:nq]
            args, pitches, kw = mem.place("host", planes, 3 - k)
            jobs.append((fmt, args, pitches, iw, ih, quads, mem.out("pinned", nq * pw * ph * 3), kw, bgr))

        def check(job, status):
            fmt, _, _, iw, ih, quads, out, _, bgr = job
            want, wstatus = rectify.patches(bgr, quads, pw, ph)
            assert wstatus.all()
            got = mem.fetch("pinned", out, len(quads) * pw * ph * 3).reshape(len(quads), ph, pw, 3)
            assert_patches(got, status, want, wstatus, "%s %dx%d" % (ra.PIX_NAMES[fmt], iw, ih))

        jobframes.growing_jobs(rect, jobs, lambda job: rect.enqueue(*job[:7], out_pinned=True, **job[7]), check)
    finally:
        rect.close()


def test_empty_job_and_full_job(mem):
    iw, ih, planes, bgr, quads = small_case(ra.PIX_RGBA)
    pw, ph = 31, 17
    want, _ = small_reference(ra.PIX_RGBA, pw, ph)
    nmax = 2 * len(quads)
    rect = ra.Rectifier(pw, ph, max_quads=nmax, njobs=2)
    try:
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.zeros((0, 4, 2)), "device")      # n = 0: nothing written, nothing returned
        assert got.shape == (0, ph, pw, 3) and len(status) == 0
        assert rect.enqueue(ra.PIX_RGBA, planes, None, iw, ih, np.zeros((0, 8)), None) == 1      # (no output buffer needed either)
        assert len(rect.wait()) == 0
        full = np.concatenate([quads, quads[::-1]])
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, full, "device")      # n = max_quads
        assert_patches(got, status, np.concatenate([want, want[::-1]]), np.ones(nmax, np.uint8), "full job")
        with pytest.raises(ValueError):
            run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.concatenate([full, quads[:1]]), "device")      # one more
    finally:
        rect.close()


def test_invalid_quads_give_zero_patches_and_leave_their_neighbours_alone(mem):
    iw, ih, planes, bgr, quads = small_case(ra.PIX_BGR)
    nan = np.array([(10, 20), (np.nan, 25), (100, 80), (5, 70)])
    bowtie = quads[0][[0, 2, 1, 3]]
    concave = np.array([(0, 0), (100, 0), (20, 20), (0, 100)], np.float64)
    collinear = np.array([(0, 0), (50, 0), (100, 0), (50, 60)], np.float64)
    repeated = quads[0][[0, 0, 2, 3]]
    mixed = np.stack([bowtie, quads[0], nan, concave, quads[2], quads[3], collinear, repeated, quads[6]])
    valid = np.array([0, 1, 0, 0, 1, 1, 0, 0, 1], np.uint8)
    for pw, ph in ((64, 64), (31, 17)):
        want, wstatus = rectify.patches(bgr, mixed, pw, ph)
        assert np.array_equal(wstatus, valid)
        rect = ra.Rectifier(pw, ph, max_quads=len(mixed), njobs=1)
        try:
            for out_kind in ("device", "pinned"):
                got, status = run_job(rect, mem, ra.PIX_BGR, planes, iw, ih, mixed, "device", out_kind)      # (the output buffer starts as 0xA5)
                assert_patches(got, status, want, valid, "mixed job")
                assert not got[valid == 0].any() and got[valid == 1].any()
        finally:
            rect.close()


def test_argument_errors_return_minus_one_and_the_next_job_is_correct(mem):
    iw, ih, planes, bgr, quads = small_case(ra.PIX_BGR)
    yw, yh, yplanes, ybgr, _ = small_case(ra.PIX_NV12)
    pw, ph = 64, 64
    want, wstatus = small_reference(ra.PIX_BGR, pw, ph)
    rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=1)
    (dframe,), (pitch,), _ = mem.place("device", planes, 3)
    (dy, duv), (py, puv), _ = mem.place("device", yplanes, 0)
    out = mem.out("device", len(quads) * pw * ph * 3)
    pageable = np.zeros(len(quads) * pw * ph * 3, np.uint8)
    q = np.ascontiguousarray(quads).reshape(-1, 8)
    P, I = ctypes.c_void_p * 3, ctypes.c_int * 3

    def call(fmt=ra.PIX_BGR, pl=(dframe, None, None), pi=(pitch, 0, 0), w=iw, h=ih, kind=1, quads_p=q.ctypes.data, n=len(q), out_p=out, out_kind=1):
        return L().rd_rectifier_enqueue(rect.h, fmt, P(*pl), I(*pi), w, h, kind, quads_p, n, out_p, out_kind)

    errors = {
        "unknown format": dict(fmt=6), "negative format": dict(fmt=-1),
        "NULL plane": dict(pl=(None, None, None)),
        "NULL chroma plane": dict(fmt=ra.PIX_NV12, pl=(dy, None, None), pi=(py, puv, 0), w=yw, h=yh),
        "NULL third plane": dict(fmt=ra.PIX_I420, pl=(dy, duv, None), pi=(py, yw // 2, yw // 2), w=yw, h=yh),
        "short pitch": dict(pi=(iw * 3 - 1, 0, 0)),
        "short chroma pitch": dict(fmt=ra.PIX_NV12, pl=(dy, duv, None), pi=(py, yw - 1, 0), w=yw, h=yh),
        "odd width with 4:2:0": dict(fmt=ra.PIX_NV12, pl=(dy, duv, None), pi=(py, puv, 0), w=yw - 1, h=yh),
        "odd height with 4:2:0": dict(fmt=ra.PIX_I420, pl=(dy, duv, duv), pi=(py, puv, puv), w=yw, h=yh - 1),
        "n < 0": dict(n=-1), "n > max_quads": dict(n=len(q) + 1),
        "pageable out": dict(out_p=pageable.ctypes.data, out_kind=2),
        "pageable out as device memory": dict(out_p=pageable.ctypes.data),
        "unknown out_kind": dict(out_kind=0), "unknown on_device": dict(kind=3),
        "no size": dict(w=0), "NULL quads": dict(quads_p=None), "NULL out": dict(out_p=None),
    }
    try:
        for name, kw in errors.items():
            assert call(**kw) == -1, name
            assert L().rd_rectifier_wait(rect.h, None) == -1, name + ": nothing may have been enqueued"
        assert call() == 0      # the first job after all of them: sequence number 0, the right bytes
        status = rect.wait()
        got = mem.fetch("device", out, pageable.nbytes).reshape(want.shape)
        assert_patches(got, status, want, wstatus, "the job after the refused ones")
        with pytest.raises(ValueError):
            rect.enqueue(6, (dframe,), (pitch,), iw, ih, quads, out, on_device=True)
        with pytest.raises(ValueError):
            ra.Rectifier(0, 64)
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- behind the detector's poll
PW, PH = 100, 60
SIW, SIH, SN = 640, 480, 12
FIXED_QUAD = np.array([[(101.5, 80.25), (420.0, 60.0), (500.5, 400.0), (60.0, 330.5)]])


def drive(nslots, n, enqueue, poll):
    out, inflight = [], 0
    for i in range(n):
        if inflight == nslots:
            out.append(poll(len(out)))
            inflight -= 1
        enqueue(i)
        inflight += 1
    while inflight:
        out.append(poll(len(out)))
        inflight -= 1
    return out


def stream_run(poly, nslots, fmt, kind, mem, rectifier=None):
    """the stream through a detector, the slots kept full; with a rectifier: after each poll the frame's own rectangles (polyline kind: FIXED_QUAD) are rectified
    from the polled slot and the job is waited for before anything else is enqueued.  [(result of the poll, quads, patches, status)]"""
    items = stream_frames(fmt, SN)      # [(planes, the contract's BGR frame)]
    det = ra.PolylineDetector(SIW, SIH, nslots=nslots) if poly else ra.Detector(SIW, SIH, nslots=nslots, aperture=TAN36)
    placed = [mem.place(kind, planes, 8) for planes, _ in items] if kind != "host" else None
    out = mem.out("device", 64 * PW * PH * 3) if rectifier else None

    def enqueue(i):
        if kind == "host":
            det.enqueue_planes(fmt, items[i][0])
        else:
            det.enqueue_planes(fmt, placed[i][0], placed[i][1], **placed[i][2])

    def poll(i):
        res = det.poll()[0] if poly else det.poll(TAN36)
        if rectifier is None:
            return res, None, None, None
        quads = FIXED_QUAD if poly else ra.rect_quads(res)
        assert len(quads) <= 64
        det.rectify_polled(rectifier, quads, out)
        status = rectifier.wait()
        nbytes = len(quads) * PW * PH * 3
        a = np.zeros(nbytes, np.uint8)
        L().rd_download(a.ctypes.data, out, nbytes)
        return res, quads, a.reshape(len(quads), PH, PW, 3), status

    try:
        return drive(nslots, len(items), enqueue, poll)
    finally:
        det.close()


@pytest.mark.parametrize("poly,nslots", [(False, 1), (False, 2), (False, 64), (True, 8)], ids=["rect-1", "rect-2", "rect-64", "poly-8"])
@pytest.mark.parametrize("fmt,kind", [(ra.PIX_BGR, "host"), (ra.PIX_NV12, "device")], ids=["bgr-host", "nv12-device"])
def test_rectify_polled_behind_every_poll(poly, nslots, fmt, kind, mem):
    items = stream_frames(fmt, SN)      # [(planes, the contract's BGR frame)]
    plain = stream_run(poly, nslots, fmt, kind, mem)
    rectifier = ra.Rectifier(PW, PH, max_quads=64, njobs=2)
    alone = ra.Rectifier(PW, PH, max_quads=64, njobs=1)
    total = 0
    try:
        det = ra.Detector(SIW, SIH, nslots=1)
        try:
            first = mem.out("device", PW * PH * 3)
            with pytest.raises(ValueError):      # nothing polled yet
                det.rectify_polled(rectifier, FIXED_QUAD, first)
        finally:
            det.close()
        got = stream_run(poly, nslots, fmt, kind, mem, rectifier)
        assert len(got) == len(plain) == len(items)
        for t, ((res, quads, patches, status), (res0, _, _, _), (planes, bgr)) in enumerate(zip(got, plain, items)):
            if poly:
                assert helpers.segments_equal(res, res0), "frame %d: the segment list changed with the rectifier behind the poll" % t
            else:
                assert helpers.rects_equal(res, res0), "frame %d: the rectangle list changed with the rectifier behind the poll" % t
            want, wstatus = rectify.patches(bgr, quads, PW, PH)
            assert_patches(patches, status, want, wstatus, "frame %d, from the polled slot" % t)
            mine, mstatus = run_job(alone, mem, fmt, planes, SIW, SIH, quads, "host")
            assert_patches(patches, status, mine, mstatus, "frame %d, against the standalone rectifier" % t)
            total += len(quads)
    finally:
        rectifier.close()
        alone.close()
    print("rectified behind the poll: %d quads over %d frames" % (total, len(items)))
    assert total > 0
    if not poly:
        assert total > len(items), "the stream's frames hold several rectangles each"


# ---------------------------------------------------------------------------------------------- the example program
def test_rdpatches_writes_the_patches_the_binding_gives(tmp_path):
    """examples/rdpatches on a PPM: one PPM per rectangle, each the patch Rectifier.rectify makes of the same image and the same rectangles"""
    import subprocess
    iw, ih, pw, ph = 640, 480, 96, 64
    img = cframe(synth.SEED0, iw, ih, 0)
    with open(tmp_path / "in.ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (iw, ih) + img[..., ::-1].tobytes())
    res = subprocess.run([os.path.join(helpers.ROOT, "examples", "rdpatches"), str(tmp_path / "in.ppm"), "0", str(tmp_path / "p"), str(pw), str(ph)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path, timeout=60)
    assert res.returncode == 0, res.stderr.decode()
    ctx = ra.Context(0)
    det = ra.RectDetector(ctx, iw, ih)
    rects = det.execute_once(img, np.tan(72.0 / 2 / 180.0 * np.pi))
    det.close()
    ctx.close()
    assert len(rects) > 0 and ("%d rectangle(s)" % len(rects)) in res.stdout.decode()
    rect = ra.Rectifier(pw, ph, max_quads=len(rects), njobs=1)
    try:
        want = rect.rectify(img, ra.rect_quads(rects))
    finally:
        rect.close()
    assert np.array_equal(want, rectify.patches(img, ra.rect_quads(rects), pw, ph)[0])
    for k in range(len(rects)):
        data = open(tmp_path / ("p%02d.ppm" % k), "rb").read()
        head = b"P6\n%d %d\n255\n" % (pw, ph)
        assert data.startswith(head)
        got = np.frombuffer(data[len(head):], np.uint8).reshape(ph, pw, 3)[..., ::-1]
        assert np.array_equal(got, want[k]), "patch %d" % k
