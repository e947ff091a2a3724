"""Matched quads on the GPU (rd_matcher, rd_detector_match_polled): the dot matrix of the matrix-core kernel equals numpy int64 on asymmetric data, an anchor
that involves no restatement pins the rotation convention, and every record equals, in every bit, the numpy restatement of the header's contract
(tests/match.py) - for the reference's own rectangles, all six pixel formats, host / device / pinned frames, jobs in flight against a growing library, every
status and argument error, and behind the poll of both detector kinds.  No tolerance anywhere."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import jobframes
from tests import match
from tests import pixfmt
from tests.jobframes import L, cframe
from tests.test_gpu_rectify import golden_jobs, noise_frame, small_case

pytestmark = pytest.mark.gpu
TAN36 = float(np.tan(36.0 / 180.0 * np.pi))


@pytest.fixture
def mem():
    m = jobframes.Mem()
    yield m
    m.close()


def pixel_quad(x0, y0, N):
    """the axis-aligned quad over the N x N pixels at (x0, y0), s along x: its patch at pw = ph = N is the crop"""
    a, b = (x0 - 0.5, y0 - 0.5), (x0 + N - 0.5, y0 + N - 0.5)
    return np.array([a, (b[0], a[1]), b, (a[0], b[1])], np.float64)


def run_job(matcher, mem, fmt, planes, iw, ih, quads, kind="host", pad=0, flags=0):
    """one job, waited for: its records (with MATCH_DOTS: records and dots)"""
    args, pitches, kw = mem.place(kind, planes, pad)
    matcher.enqueue(fmt, args, pitches, iw, ih, quads, flags=flags, **kw)
    return matcher.wait(dots=bool(flags & ra.MATCH_DOTS))


# ---------------------------------------------------------------------------------------------- the dot kernel: exact, on asymmetric data
@pytest.mark.parametrize("G,m", [(8, 4), (16, 2), (32, 1), (64, 1)], ids=["G8", "G16", "G32", "G64"])
def test_dots_equal_numpy_int64_for_every_tile_edge(G, m, mem):
    """templates and quads from noise images: every byte of A and B differs from its neighbours, so a wrong lane map of the A, B or C/D fragments cannot pass.
    n in {1, 16, 17} quads against T in {1, 15, 16, 17} templates: neither n nor 4T stops at a tile edge; D / 64 = 1 .. 64 steps of k"""
    N = G * m
    iw, ih = 333, 217
    frame = noise_frame(iw, ih, 70 + G)
    rng = np.random.default_rng(G)
    quads = np.array([pixel_quad(int(rng.integers(0, iw - N + 1)), int(rng.integers(0, ih - N + 1)), N) for _ in range(17)])
    quads[3] = [(40.25, 30.5), (200.75, 12.0), (230.0, 150.5), (25.5, 120.0)]      # (and two that are not at pixel pitch)
    quads[11] = [(-20.0, -15.5), (90.0, -4.0), (70.5, 60.0), (-9.0, 44.0)]
    sig, st = match.signatures(frame, quads, G, m)
    assert st.all()
    images = [noise_frame(N, N, 1000 + 10 * G + k) for k in range(17)]
    tsig = [match.signatures(img, [match.whole(N, N)], G, m)[0][0] for img in images]
    matcher = ra.Matcher(G, m, max_templates=17, max_quads=17, njobs=1)
    (dframe,), (pitch,), kw = mem.place("device", (frame,), 5)
    try:
        for T in (1, 15, 16, 17):
            while matcher.templates() < T:
                assert matcher.add_image(images[matcher.templates()]) == matcher.templates() - 1
            lib = match.library(tsig[:T])
            for k in (0, T - 1):
                for r in range(4):
                    got, sb, sbb = matcher.signature(k, r)
                    assert np.array_equal(got.reshape(-1), lib[4 * k + r]) and sb == lib[4 * k + r].sum() and sbb == (lib[4 * k + r] ** 2).sum(), "column %d of T = %d" % (4 * k + r, T)
            for n in (1, 16, 17):
                matcher.enqueue(ra.PIX_BGR, (dframe,), (pitch,), iw, ih, quads[:n], flags=ra.MATCH_DOTS, **kw)
                recs, dots = matcher.wait(dots=True)
                want, wdots = match.records(sig[:n], st[:n], lib)
                assert dots.shape == (n, 4 * T) and np.array_equal(dots.astype(np.int64), wdots), "G = %d, n = %d, T = %d: %d dots differ" % (G, n, T, int((dots != wdots).sum()))
                match.assert_records(recs, want, "G = %d, n = %d, T = %d" % (G, n, T))
    finally:
        matcher.close()


# ---------------------------------------------------------------------------------------------- anchor: no restatement involved
@pytest.mark.parametrize("G,m", [(8, 4), (16, 2), (32, 1), (64, 1)], ids=["G8", "G16", "G32", "G64"])
def test_a_pasted_template_is_found_with_the_documented_rotation(G, m):
    """the header: column 4k + r is the template turned r quarter turns CLOCKWISE, and then the template's first corner lies at the quad's corner r.  np.rot90(img, r)
    turns r times counter-clockwise, so a template pasted that way is found with rot = (4 - r) % 4"""
    N = G * m
    iw, ih, x0, y0 = 333, 217, 37, 21
    images = [noise_frame(N, N, 300 + G + k) for k in range(3)]
    k = 1

    def box_mean(img):      # plain integer numpy, from the header's text
        p = img.astype(np.int64)
        grey = (29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8
        cell = np.zeros((G, G), np.int64)
        for j in range(G):
            for i in range(G):
                cell[j, i] = (grey[j * m:(j + 1) * m, i * m:(i + 1) * m].sum() + m * m // 2) >> {1: 0, 2: 2, 4: 4}[m]
        return cell - 128

    matcher = ra.Matcher(G, m, max_templates=3, max_quads=4, njobs=1)
    try:
        for img in images:
            matcher.add_image(img)
        up, sb, sbb = matcher.signature(k, 0)
        assert np.array_equal(up, box_mean(images[k])) and sb == int(up.astype(np.int64).sum()) and sbb == int((up.astype(np.int64) ** 2).sum())
        for r in range(4):
            frame = noise_frame(iw, ih, 9)
            frame[y0:y0 + N, x0:x0 + N] = np.rot90(images[k], r)
            rec = matcher.match(frame, [pixel_quad(x0, y0, N)])[0]
            rot = (4 - r) % 4
            assert (rec["status"], rec["tmpl"], rec["rot"]) == (1, k, rot), (r, rec)
            assert rec["dot"] == sbb and rec["sa"] == sb and rec["saa"] == sbb and rec["score"] == 1.0, (r, rec)
            assert rec["tmpl2"] in (0, 2), (r, rec)
            col, csb, csbb = matcher.signature(k, rot)
            assert np.array_equal(col, box_mean(np.rot90(images[k], r))) and (csb, csbb) == (sb, sbb), r
            # the template's first corner is the quad's corner `rot`: the quad started there is the template upright
            turned = np.roll(pixel_quad(x0, y0, N), -rot, axis=0)
            rec = matcher.match(frame, [turned])[0]
            assert (rec["tmpl"], rec["rot"], rec["score"]) == (k, 0, 1.0), (r, rec)
    finally:
        matcher.close()


# ---------------------------------------------------------------------------------------------- the reference's rectangles
def test_records_of_the_references_rectangles_match_numpy(mem):
    G, m, NT = 16, 2, 9
    jobs = list(golden_jobs())
    matcher = ra.Matcher(G, m, max_templates=NT, max_quads=80, njobs=1)
    tsig = []
    total = outside = empty = 0
    try:
        # the library: the first rectangles of the set, one frame after the other, until there are nine
        for name, frame, rects in jobs:
            ih, iw = frame.shape[:2]
            for quad in ra.rect_quads(rects)[:3]:
                if len(tsig) == NT:
                    break
                S, st = match.signatures(frame, [quad], G, m)
                assert st[0] and not match.flat(S[0])
                assert matcher.add_image(frame, quad) == len(tsig)
                got, sb, sbb = matcher.signature(len(tsig), 0)
                assert np.array_equal(got, S[0]), "template %d from %s" % (len(tsig), name)
                tsig.append(S[0])
        assert len(tsig) == NT
        lib = match.library(tsig)
        for name, frame, rects in jobs:
            ih, iw = frame.shape[:2]
            quads = ra.rect_quads(rects)
            got = run_job(matcher, mem, ra.PIX_BGR, (frame,), iw, ih, quads, kind="device")
            sig, st = match.signatures(frame, quads, G, m)
            want, _ = match.records(sig, st, lib)
            match.assert_records(got, want, name)
            total += len(quads)
            empty += len(quads) == 0
            outside += int(((quads[..., 0] < 0) | (quads[..., 0] > iw - 1) | (quads[..., 1] < 0) | (quads[..., 1] > ih - 1)).any(axis=1).sum())
            mem.close()
    finally:
        matcher.close()
    print("golden quads matched: %d, reaching outside their frame: %d, empty lists: %d" % (total, outside, empty))
    assert total > 400 and outside > 0 and empty > 0


# ---------------------------------------------------------------------------------------------- formats, frame kinds, jobs in flight
G0, M0 = 16, 2


@lru_cache(maxsize=None)
def small_library():
    """template images (noise, and one cut from the small BGR frame so that something correlates) and their restated signatures"""
    iw, ih, planes, bgr, quads = small_case(ra.PIX_BGR)
    images = [(noise_frame(G0 * M0, G0 * M0, 41), None), (bgr, quads[0]), (noise_frame(50, 70, 42), None), (bgr, quads[6]), (noise_frame(G0 * M0, G0 * M0, 43), None)]
    sigs = [match.signatures(img, [match.whole(img.shape[1], img.shape[0]) if q is None else q], G0, M0)[0][0] for img, q in images]
    return images, sigs


@lru_cache(maxsize=None)
def small_signatures(fmt):
    iw, ih, planes, bgr, quads = small_case(fmt)
    return match.signatures(bgr, quads, G0, M0)


@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_every_format_and_frame_kind(fmt, mem):
    iw, ih, planes, bgr, quads = small_case(fmt)
    images, sigs = small_library()
    matcher = ra.Matcher(G0, M0, max_templates=8, max_quads=len(quads), njobs=2)
    try:
        for img, q in images[:3]:
            matcher.add_image(img, q)
        sig, st = small_signatures(fmt)
        want, _ = match.records(sig, st, match.library(sigs[:3]))
        for kind in ("host", "device", "pinned"):
            for pad in (0, 13):
                got = run_job(matcher, mem, fmt, planes, iw, ih, quads, kind, pad)
                match.assert_records(got, want, "%s %s frame, pad %d" % (ra.PIX_NAMES[fmt], kind, pad))
        # a template handed over in this format, as a device frame with padded rows: the signature of the contract's BGR frame
        args, pitches, kw = mem.place("device", planes, 7)
        assert matcher.add(fmt, args, pitches, iw, ih, quads[1], **kw) == 3
        assert np.array_equal(matcher.signature(3, 0)[0], sig[1])
    finally:
        matcher.close()


def test_four_jobs_in_flight_see_the_library_of_their_enqueue(mem):
    iw, ih, planes, bgr, quads = small_case(ra.PIX_BGR)
    images, sigs = small_library()
    sig, st = small_signatures(ra.PIX_BGR)
    matcher = ra.Matcher(G0, M0, max_templates=8, max_quads=len(quads), njobs=4)
    args, pitches, kw = mem.place("pinned", planes, 3)
    try:
        sel = [slice(0, 7), slice(2, 5), slice(0, 0), slice(1, 7)]
        for k in range(4):
            assert matcher.add_image(*images[k]) == k
            assert matcher.enqueue(ra.PIX_BGR, args, pitches, iw, ih, quads[sel[k]], flags=ra.MATCH_DOTS if k % 2 else 0, **kw) == k
        assert matcher.add_image(*images[4]) == 4      # (after the last job: none of them sees it)
        for k in range(4):
            want, wdots = match.records(sig[sel[k]], st[sel[k]], match.library(sigs[:k + 1]))
            got, dots = matcher.wait(dots=True)
            match.assert_records(got, want, "job %d against %d templates" % (k, k + 1))
            assert (dots is None) == (k % 2 == 0) and (dots is None or np.array_equal(dots, wdots))
        with pytest.raises(RuntimeError):
            matcher.wait()
    finally:
        matcher.close()


def test_one_job_too_many_is_fatal():
    jobframes.assert_one_job_too_many_is_fatal("s = ra.Matcher(8, 1, max_templates=1, max_quads=1, njobs=3)\nq = [[(4, 4), (40, 4), (40, 40), (4, 40)]]",
                                               "s.enqueue(ra.PIX_BGR, (d,), (64 * 3,), 64, 64, q, on_device=True)", "rd_matcher_enqueue")


# ---------------------------------------------------------------------------------------------- statuses and errors
def test_statuses(mem):
    iw, ih, planes, bgr, quads = small_case(ra.PIX_BGR)
    frame = bgr.copy()
    frame[100:180, 200:300] = (17, 130, 240)      # a constant area
    nan = np.array([(10, 20), (np.nan, 25), (100, 80), (5, 70)])
    concave = np.array([(0, 0), (100, 0), (20, 20), (0, 100)], np.float64)
    const = np.array([(210.0, 110.0), (290.0, 112.0), (288.0, 170.0), (212.0, 168.0)])
    mixed = np.stack([quads[0], concave, const, nan, quads[6]])
    sig, st = match.signatures(frame, mixed, G0, M0)
    assert st.tolist() == [1, 0, 1, 0, 1] and match.flat(sig[2])
    images, sigs = small_library()
    matcher = ra.Matcher(G0, M0, max_templates=2, max_quads=len(mixed), njobs=1)
    try:
        got = run_job(matcher, mem, ra.PIX_BGR, (frame,), iw, ih, mixed, "device", flags=ra.MATCH_DOTS)      # an empty library
        assert got[0]["status"].tolist() == [3, 0, 3, 0, 3] and got[1].shape == (5, 0)
        match.assert_records(got[0], match.records(sig, st, match.library([]))[0], "empty library")
        with pytest.raises(ArithmeticError):
            matcher.add_image(np.full((40, 40, 3), 99, np.uint8))      # flat
        with pytest.raises(ArithmeticError):
            matcher.add_image(frame, const)      # flat, from a quad
        with pytest.raises(ArithmeticError):
            matcher.add_image(frame, concave)      # an invalid quad
        with pytest.raises(ArithmeticError):
            matcher.add_image(frame, nan)
        assert matcher.templates() == 0
        with pytest.raises(IndexError):
            matcher.signature(0, 0)
        assert matcher.add_image(*images[0]) == 0      # one template: no runner-up
        got, dots = run_job(matcher, mem, ra.PIX_BGR, (frame,), iw, ih, mixed, "device", flags=ra.MATCH_DOTS)
        want, wdots = match.records(sig, st, match.library(sigs[:1]))
        match.assert_records(got, want, "one template")
        assert got["status"].tolist() == [1, 0, 2, 0, 1] and (got["tmpl2"][[0, 4]] == -1).all() and np.array_equal(dots, wdots) and not dots[[1, 3]].any()
        for k in (1, 2, 3):
            assert got[k].tobytes()[4:] == bytes(52)
        assert matcher.add_image(*images[1]) == 1
        with pytest.raises(ValueError):
            matcher.add_image(*images[2])      # the library is full
        with pytest.raises(IndexError):
            matcher.signature(1, 4)
        got = run_job(matcher, mem, ra.PIX_BGR, (frame,), iw, ih, mixed, "host")
        match.assert_records(got, match.records(sig, st, match.library(sigs[:2]))[0], "two templates")
    finally:
        matcher.close()


def test_empty_job_and_full_job(mem):
    iw, ih, planes, bgr, quads = small_case(ra.PIX_RGBA)
    images, sigs = small_library()
    sig, st = small_signatures(ra.PIX_RGBA)
    nmax = 2 * len(quads)
    matcher = ra.Matcher(G0, M0, max_templates=2, max_quads=nmax, njobs=2)
    try:
        matcher.add_image(*images[0])
        matcher.add_image(*images[1])
        lib = match.library(sigs[:2])
        got, dots = run_job(matcher, mem, ra.PIX_RGBA, planes, iw, ih, np.zeros((0, 4, 2)), "device", flags=ra.MATCH_DOTS)      # n = 0
        assert len(got) == 0 and dots.shape == (0, 8)
        full = np.concatenate([quads, quads[::-1]])
        got = run_job(matcher, mem, ra.PIX_RGBA, planes, iw, ih, full, "device")      # n = max_quads
        match.assert_records(got, match.records(np.concatenate([sig, sig[::-1]]), np.concatenate([st, st[::-1]]), lib)[0], "full job")
        with pytest.raises(ValueError):
            run_job(matcher, mem, ra.PIX_RGBA, planes, iw, ih, np.concatenate([full, quads[:1]]), "device")      # one more
    finally:
        matcher.close()


def test_argument_errors_return_minus_one_and_the_next_job_is_correct(mem):
    iw, ih, planes, bgr, quads = small_case(ra.PIX_BGR)
    yw, yh, yplanes, ybgr, _ = small_case(ra.PIX_NV12)
    images, sigs = small_library()
    sig, st = small_signatures(ra.PIX_BGR)
    lim = ra.match_limits()
    for bad in (dict(grid=12), dict(grid=128), dict(grid=0), dict(oversample=3), dict(oversample=8), dict(oversample=0), dict(max_templates=0),
                dict(max_templates=lim["max_templates"] + 1), dict(max_quads=0), dict(max_quads=lim["max_quads"] + 1), dict(njobs=0), dict(njobs=1025), dict(device=-1), dict(device=64)):
        with pytest.raises(ValueError):
            ra.Matcher(**{**dict(grid=16, oversample=2, max_templates=4, max_quads=4, njobs=1), **bad})
    matcher = ra.Matcher(G0, M0, max_templates=4, max_quads=len(quads), njobs=1)
    (dframe,), (pitch,), _ = mem.place("device", planes, 3)
    (dy, duv), (py, puv), _ = mem.place("device", yplanes, 0)
    q = np.ascontiguousarray(quads).reshape(-1, 8)
    P, I = ctypes.c_void_p * 3, ctypes.c_int * 3

    def enqueue(fmt=ra.PIX_BGR, pl=(dframe, None, None), pi=(pitch, 0, 0), w=iw, h=ih, kind=1, quads_p=q.ctypes.data, n=len(q), flags=0):
        return L().rd_matcher_enqueue(matcher.h, fmt, P(*pl), I(*pi), w, h, kind, quads_p, n, flags)

    def add(fmt=ra.PIX_BGR, pl=(dframe, None, None), pi=(pitch, 0, 0), w=iw, h=ih, kind=1, quad_p=q.ctypes.data):
        return L().rd_matcher_add(matcher.h, fmt, P(*pl), I(*pi), w, h, kind, quad_p)

    frame_errors = {
        "unknown format": dict(fmt=6), "negative format": dict(fmt=-1),
        "NULL plane": dict(pl=(None, None, None)),
        "NULL chroma plane": dict(fmt=ra.PIX_NV12, pl=(dy, None, None), pi=(py, puv, 0), w=yw, h=yh),
        "NULL third plane": dict(fmt=ra.PIX_I420, pl=(dy, duv, None), pi=(py, yw // 2, yw // 2), w=yw, h=yh),
        "short pitch": dict(pi=(iw * 3 - 1, 0, 0)),
        "short chroma pitch": dict(fmt=ra.PIX_NV12, pl=(dy, duv, None), pi=(py, yw - 1, 0), w=yw, h=yh),
        "odd width with 4:2:0": dict(fmt=ra.PIX_NV12, pl=(dy, duv, None), pi=(py, puv, 0), w=yw - 1, h=yh),
        "odd height with 4:2:0": dict(fmt=ra.PIX_I420, pl=(dy, duv, duv), pi=(py, puv, puv), w=yw, h=yh - 1),
        "unknown on_device": dict(kind=3), "no size": dict(w=0), "too wide": dict(w=65537),
    }
    job_errors = {"n < 0": dict(n=-1), "n > max_quads": dict(n=len(q) + 1), "NULL quads": dict(quads_p=None), "unknown flag": dict(flags=2), "negative flags": dict(flags=-2)}
    try:
        for name, kw in frame_errors.items():
            assert add(**kw) == -1, name
            assert matcher.templates() == 0, name
        for k in range(4):
            assert matcher.add_image(*images[k]) == k
        assert add() == -1 and matcher.templates() == 4      # a full library
        for name, kw in {**frame_errors, **job_errors}.items():
            assert enqueue(**kw) == -1, name
            assert L().rd_matcher_wait(matcher.h, None, None) == -1, name + ": nothing may have been enqueued"
        assert enqueue() == 0      # the first job after all of them: sequence number 0, the right records
        matcher._jobs.append((len(q), 4, 0))
        match.assert_records(matcher.wait(), match.records(sig, st, match.library(sigs[:4]))[0], "the job after the refused ones")
        assert L().rd_matcher_signature(matcher.h, -1, 0, None, None) == -1 and L().rd_matcher_signature(matcher.h, 4, 0, None, None) == -1
        assert L().rd_matcher_signature(matcher.h, 0, -1, None, None) == -1 and L().rd_matcher_signature(matcher.h, 3, 3, None, None) == 0
    finally:
        matcher.close()


# ---------------------------------------------------------------------------------------------- behind the detector's poll
SIW, SIH, SN = 640, 480, 4
FIXED_QUADS = np.array([[(101.5, 80.25), (420.0, 60.0), (500.5, 400.0), (60.0, 330.5)], [(300.0, 200.0), (620.0, 210.0), (600.5, 470.0), (310.0, 440.5)]])


@pytest.mark.parametrize("kind", ["rect", "poly", "scaled"])
def test_match_polled_equals_enqueue_on_the_same_planes(kind, mem):
    """after Detector.poll, after PolylineDetector.poll, and on a frame that came in at scale 2 (quads in detector coordinates, mapped X = 2x + 0.5): the records of
    match_polled are those of Matcher.enqueue on the frame's planes and the mapped corners"""
    fmt = ra.PIX_NV12 if kind == "rect" else ra.PIX_BGR
    frames = [pixfmt.convert(cframe(synth.SEED0, SIW, SIH, t), fmt) for t in range(SN)]
    scale = 2 if kind == "scaled" else 1
    dw, dh = SIW // scale, SIH // scale
    det = ra.PolylineDetector(dw, dh, nslots=2) if kind == "poly" else ra.Detector(dw, dh, nslots=2, aperture=TAN36)
    matcher = ra.Matcher(G0, M0, max_templates=4, max_quads=64, njobs=2)
    alone = ra.Matcher(G0, M0, max_templates=4, max_quads=64, njobs=1)
    total = 0
    try:
        with pytest.raises(ValueError):      # nothing polled yet
            det.match_polled(matcher, FIXED_QUADS)
        for mt in (matcher, alone):
            mt.add_image(frames[0][1], FIXED_QUADS[0])
            mt.add_image(frames[1][1], FIXED_QUADS[1])
            mt.add_image(noise_frame(40, 40, 77))
        for t, (planes, bgr) in enumerate(frames):
            if kind == "scaled":
                det.enqueue_scaled(fmt, planes)
            elif t % 2:
                args, pitches, kw = mem.place("device", planes, 8)
                det.enqueue_planes(fmt, args, pitches, **kw)
            else:
                det.enqueue_planes(fmt, planes)
            res = det.poll()[0] if kind == "poly" else det.poll(TAN36)
            quads = FIXED_QUADS / scale if kind == "poly" or len(res) == 0 else np.concatenate([ra.rect_quads(res), FIXED_QUADS / scale])
            assert det.match_polled(matcher, quads, flags=ra.MATCH_DOTS) == t
            got, dots = matcher.wait(dots=True)
            mapped = quads * 2.0 + 0.5 if scale == 2 else quads
            alone.enqueue(fmt, planes, None, SIW, SIH, mapped, flags=ra.MATCH_DOTS)
            want, wdots = alone.wait(dots=True)
            match.assert_records(got, want, "%s frame %d" % (kind, t))
            assert np.array_equal(dots, wdots)
            total += len(quads)
        assert total > 2 * SN or kind != "rect", "the stream's frames hold rectangles"
    finally:
        matcher.close()
        alone.close()
        det.close()
