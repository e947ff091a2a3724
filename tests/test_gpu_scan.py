"""Scanned pages on the GPU (rd_rectifier_create_scan): every byte equals the numpy restatement of the header's contract (tests/scan.py on tests/tensor.py's gray
plane) - for every mode, oversampling, polarity and a range of (k, d), output sizes on every side of the pad bits, the byte, the 64-pixel word and the kernel's
tile, radii that make a window larger than the patch, larger than the tile, and a halo that crosses two tiles, all six pixel formats, host / device / pinned
frames, device / pinned output, a misaligned output, a constant and a two-level frame, invalid quads, jobs in flight, empty and full jobs, argument errors, behind
the poll of both detector kinds, into memory that torch allocated, and from the example program.  Every case also runs the { U8, NHWC, GRAY, m } tensor rectifier on
the same job and compares the pages with the restatement's steps 2-5 applied to THAT plane, so that a failure names the launch at fault.  Every device output lies
between guard bytes that must not change.  No tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers
from tests import pixfmt
from tests import rectjobs
from tests import scan
from tests import tensor
from tests.rectjobs import L, Out, STATUS, case, cframe, gray_job, gray_planes, job_quads, mem, run_job      # (mem: the fixture)

pytestmark = pytest.mark.gpu
TW, TH = ra.scan_limits()["tile_w"], ra.scan_limits()["tile_h"]
# the pad bits alone; a tail byte; whole bytes; one bit into the next byte with rows that start misaligned; one short of the 64-pixel word, the word, one more;
# the tile, one pixel into the next tile in both directions, and three tile columns with a tail, one row short of the tile
SIZES = ((1, 1), (7, 3), (8, 8), (9, 5), (63, 2), (64, 1), (65, 2), (TW, TH), (TW + 1, TH + 1), (2 * TW + 3, TH - 1))
RADII = (1, 2, 8, 63)
KD = ((0, 0), (26, 0), (38, 7), (255, 255))


def reference(fmt, pw, ph, spec, sel=None, seed=0):
    """(the pages of the case's quads - or of those in sel -, status) from the shared planes"""
    g, st = gray_planes(fmt, pw, ph, int(spec["oversample"]), seed)
    sel = list(range(len(st))) if sel is None else list(sel)
    return scan.from_planes(g[sel], st[sel], spec), st[sel].copy()


def test_shared_reference_is_the_restatement():
    spec = ra.scan_spec(ra.SCAN_BITS, 2, 26, 0, oversample=2, invert=True)
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    a, b = reference(ra.PIX_BGR, 9, 5, spec), scan.pages(bgr, quads, 9, 5, spec)
    scan.assert_pages(a[0], a[1], b[0], b[1])
    assert a[1].tolist() == STATUS.tolist() and a[0].shape == (4, 5, 2)


def localise(got, status, gpu_plane, want, wstatus, spec, what):
    """(a) the pages against steps 2-5 of the restatement on the plane the GPU's first launch made - a difference here is the scan kernel's -, (b) against the full
    restatement - a difference here alone is the tensor kernel's"""
    scan.assert_pages(got, status, scan.from_planes(gpu_plane, status, spec), wstatus, what + ": rdk::scan, from the GPU's own G plane")
    scan.assert_pages(got, status, want, wstatus, what + ": the full restatement")


def check_specs(mem, fmt, pw, ph, specs, kinds=(("device", "device", 0),), offset=0, seed=0):
    """every spec (all of one oversampling) on the case's job, with the tensor rectifier's plane of the same job"""
    iw, ih, planes, bgr, quads = case(fmt, seed)
    m = int(specs[0]["oversample"])
    plane, pstatus = gray_job(mem, fmt, planes, iw, ih, quads, pw, ph, m)
    assert pstatus.tolist() == STATUS.tolist()
    for spec in specs:
        assert int(spec["oversample"]) == m
        want, wstatus = reference(fmt, pw, ph, spec, seed=seed)
        rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=2, scan=spec)
        try:
            assert rect.patch_bytes == ra.scan_bytes(spec, pw, ph) == want[0].nbytes and rect.dtype == np.uint8 and rect.shape(len(quads)) == want.shape
            for kind, out_kind, pad in kinds:
                got, status = run_job(rect, mem, fmt, planes, iw, ih, quads, kind, out_kind, pad, offset)
                localise(got, status, plane, want, wstatus, spec, "%s %s %dx%d %s frame, %s output, pad %d, offset %d" % (ra.PIX_NAMES[fmt], scan.name(spec), pw, ph, kind, out_kind, pad, offset))
                assert not got[1].any(), "an invalid quad gives zero bytes"
        finally:
            rect.close()


# ---------------------------------------------------------------------------------------------- every size, radius and mode; every oversampling, polarity, (k, d)
def size_specs():
    """every (radius, mode) pair once, as three lists by oversampling: each mode meets every oversampling and both polarities, each radius every mode"""
    by_m = {1: [], 2: [], 4: []}
    for n, (r, mode) in enumerate((r, mode) for r in RADII for mode in scan.MODES):
        m = (1, 2, 4)[(n + n // 3) % 3]
        k, d = KD[n % 4]
        by_m[m].append(ra.scan_spec(mode, r, k, d, (230, 255, 128)[(n // 3) % 3], m, (n // 2) % 2 == 1))
    return by_m


@pytest.mark.parametrize("pw,ph", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_every_output_size_radius_and_mode(pw, ph, mem):
    by_m = size_specs()
    assert sorted((int(s["radius"]), int(s["mode"])) for specs in by_m.values() for s in specs) == sorted((r, mode) for r in RADII for mode in scan.MODES)
    for specs in by_m.values():
        check_specs(mem, ra.PIX_BGR, pw, ph, specs)
        mem.close()


@pytest.mark.parametrize("mode", scan.MODES, ids=[scan.MODE_NAMES[m] for m in scan.MODES])
def test_full_cross_of_oversampling_polarity_and_thresholds(mode, mem):
    for m in (1, 2, 4):
        check_specs(mem, ra.PIX_BGR, TW + 1, TH + 1, [ra.scan_spec(mode, 2, k, d, 200, m, inv) for inv in (False, True) for k, d in KD])
        mem.close()


# ---------------------------------------------------------------------------------------------- formats, frame kinds, output kinds, a misaligned output
@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_every_format_frame_kind_and_output_kind(fmt, mem):
    kinds = [(kind, out_kind, 13 if kind == "device" else 0) for kind in ("host", "device", "pinned") for out_kind in ("device", "pinned")]
    check_specs(mem, fmt, TW + 1, 9, [ra.scan_spec(scan.MODES[fmt % 3], 8, 26, 0, oversample=2, invert=fmt % 2 == 1)], kinds)


def test_out_offset_by_one_byte_takes_the_misaligned_store_paths(mem):
    for pw, ph in ((TW, 5), (2 * TW + 3, 3), (2 * TW, 4)):      # (whole 8-byte words of bit rows that no longer start on an 8-byte boundary among them)
        check_specs(mem, ra.PIX_BGR, pw, ph, [ra.scan_spec(mode, 2, 26, 0) for mode in scan.MODES], offset=1)
        check_specs(mem, ra.PIX_BGR, pw, ph, [ra.scan_spec(ra.SCAN_BITS, 8, 38, 7)], offset=4)


# ---------------------------------------------------------------------------------------------- frames that meet the contract's special cases
def test_constant_frame_has_no_ink_and_flat_is_white(mem):
    iw, ih = 97, 61
    quads = job_quads(iw, ih)
    for v in (0, 93, 255):
        frame = np.full((ih, iw, 3), v, np.uint8)
        for inv in (False, True):
            for k, d in KD:
                for mode in scan.MODES:
                    rect = ra.Rectifier(TW + 1, TH + 1, max_quads=4, njobs=1, scan=ra.scan_spec(mode, 8, k, d, 217, 1, inv))
                    try:
                        got, status = run_job(rect, mem, ra.PIX_BGR, [frame], iw, ih, quads)
                    finally:
                        rect.close()
                    assert status.tolist() == STATUS.tolist()
                    valid = got[status == 1]
                    assert (valid == {ra.SCAN_FLAT: 217, ra.SCAN_BILEVEL: 255, ra.SCAN_BITS: 0}[mode]).all(), (v, inv, k, d, mode)
                    assert not got[1].any()
        mem.close()


def test_two_level_checker_meets_the_equality_of_the_comparison(mem):
    """blocks of 8 x 8 pixels of two gray levels, sampled pixel for pixel: most windows of radius 1 and 2 are constant, and 256 N (G + d) == (256 - k) T there"""
    iw, ih, pw, ph = 97, 61, 64, 32
    yy, xx = np.mgrid[0:ih, 0:iw]
    frame = np.repeat(np.where(((xx >> 3) + (yy >> 3)) & 1, 192, 64).astype(np.uint8)[..., None], 3, axis=2)
    quad = np.array([[(10.5, 8.5), (74.5, 8.5), (74.5, 40.5), (10.5, 40.5)]])      # patch pixel (i, j) is frame pixel (11 + i, 9 + j)
    g0, st = tensor.tensors(frame, quad, pw, ph, ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, 1))
    g0 = g0.reshape(1, ph, pw)
    assert np.array_equal(g0[0], frame[9:9 + ph, 11:11 + pw, 0]) and set(np.unique(g0)) == {64, 192}
    for r in (1, 2):
        N, T = scan.window(g0[0], r)
        assert int((256 * N * g0[0] == 256 * T).sum()) > pw * ph // 8      # the equality case, in an eighth of the pixels at least
        for mode in scan.MODES:
            for k, d in ((0, 0), (26, 0)):
                spec = ra.scan_spec(mode, r, k, d)
                rect = ra.Rectifier(pw, ph, max_quads=1, njobs=1, scan=spec)
                try:
                    got, status = run_job(rect, mem, ra.PIX_BGR, [frame], iw, ih, quad)
                finally:
                    rect.close()
                scan.assert_pages(got, status, scan.from_planes(g0, st, spec), st, scan.name(spec))
                if (k, d) == (0, 0) and mode == ra.SCAN_BILEVEL:
                    assert (got[0][256 * N * g0[0] == 256 * T] == 255).all(), "equal is not darker"


# ---------------------------------------------------------------------------------------------- jobs in flight, empty and full jobs, argument errors
def test_four_jobs_in_flight_on_four_frames(mem):
    pw, ph, njobs = TW + 1, 5, 4
    spec = ra.scan_spec(ra.SCAN_BITS, 8, 26, 0, oversample=2)
    rect = ra.Rectifier(pw, ph, max_quads=4, njobs=njobs, scan=spec)
    try:
        for rnd in range(2):      # (the second round reuses every slot's G plane)
            pending = []
            for k in range(njobs):
                iw, ih, planes, bgr, quads = case(ra.PIX_BGR, seed=k)
                sel = list(range(4))[k % 2:4 - k // 2] if rnd else list(range(4))
                args, pitches, kw = mem.place("device", planes, 5)
                out = Out(mem, "device" if k % 2 == 0 else "pinned", len(sel) * rect.patch_bytes)
                assert rect.enqueue(ra.PIX_BGR, args, pitches, iw, ih, quads[sel], out.ptr, out_pinned=k % 2 == 1, **kw) == rnd * njobs + k
                pending.append((k, sel, out))
            for k, sel, out in pending:
                status = rect.wait()
                want, wstatus = reference(ra.PIX_BGR, pw, ph, spec, sel, seed=k)
                scan.assert_pages(out.fetch().reshape(rect.shape(len(sel))), status, want, wstatus, "round %d job %d" % (rnd, k))
        with pytest.raises(RuntimeError):
            rect.wait()      # nothing in flight
    finally:
        rect.close()


def test_empty_job_and_full_job(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_RGBA)
    pw, ph = 9, 5
    spec = ra.scan_spec(ra.SCAN_BITS, 2, 26, 0, oversample=4)
    want, wstatus = reference(ra.PIX_RGBA, pw, ph, spec)
    nmax = 2 * len(quads)
    rect = ra.Rectifier(pw, ph, max_quads=nmax, njobs=2, scan=spec)
    try:
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.zeros((0, 4, 2)))      # n = 0: nothing written, nothing returned
        assert got.shape == (0, ph, 2) and len(status) == 0
        assert rect.enqueue(ra.PIX_RGBA, planes, None, iw, ih, np.zeros((0, 8)), None) == 1      # (no output buffer needed either)
        assert len(rect.wait()) == 0
        full = np.concatenate([quads, quads[::-1]])
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, full, "host", "pinned")      # n = max_quads
        scan.assert_pages(got, status, np.concatenate([want, want[::-1]]), np.concatenate([wstatus, wstatus[::-1]]), "full job")
        with pytest.raises(ValueError):
            run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.concatenate([full, quads[:1]]))      # one more
        conv = rect.rectify(bgr, quads)      # the convenience call
        scan.assert_pages(conv, wstatus, want, wstatus, "rectify()")
    finally:
        rect.close()


def test_argument_errors_return_minus_one_and_the_next_job_is_correct(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = TW + 1, 9
    spec = ra.scan_spec(ra.SCAN_FLAT, 8, 26, 0, oversample=2)
    want, wstatus = reference(ra.PIX_BGR, pw, ph, spec)
    create = lambda *a: L().rd_rectifier_create_scan(*a)
    assert not create(0, pw, ph, 4, 1, None)      # a NULL spec
    for field, v in (("mode", 3), ("radius", 0), ("radius", 64), ("k", 256), ("d", -1), ("white", 0), ("oversample", 3), ("invert", 2), ("reserved", 1)):
        bad = spec.copy()
        bad[field] = v
        assert not create(0, pw, ph, 4, 1, bad.ctypes.data), field
        with pytest.raises(ValueError):
            ra.Rectifier(pw, ph, scan=bad)
    with pytest.raises(ValueError):
        ra.Rectifier(pw, ph, scan=spec, tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, 2))      # one or the other
    for args in ((0, 0, ph, 4, 1), (0, pw, 0, 4, 1), (0, 8193, ph, 4, 1), (0, pw, 8193, 4, 1), (0, pw, ph, 0, 1), (0, pw, ph, 4, 0), (99, pw, ph, 4, 1)):
        assert not create(*args, spec.ctypes.data), args      # rd_rectifier_create's bad arguments (pw * m > 16384 among them)
    rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=1, scan=spec)
    out = Out(mem, "device", len(quads) * rect.patch_bytes)
    try:
        q = rectjobs.refused_enqueues(mem, rect, planes, iw, ih, quads, out)      # and the first job after all of them: the right bytes
        status = rect.wait()
        scan.assert_pages(out.fetch().reshape(rect.shape(len(q))), status, want, wstatus, "the job after the refused ones")
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- behind the detector's poll
POLL_SPEC = ra.scan_spec(ra.SCAN_BITS, 15, 26, 0, oversample=2)


@pytest.mark.parametrize("kind", ["rect-host", "rect-device", "poly-host", "poly-device", "scaled"])
def test_rectify_polled_behind_every_poll(kind, mem):
    """after Detector.poll and PolylineDetector.poll, on host frames (the detector's own copy) and device frames, and on a frame that came in at scale 2 - quads in
    detector coordinates, the page from the full-size source (X = 2x + 0.5)"""
    rectjobs.polled_behind_a_poll(mem, kind, dict(scan=POLL_SPEC), lambda bgr, quads: scan.pages(bgr, quads, rectjobs.PW, rectjobs.PH, POLL_SPEC),
                                  lambda got, status, plane, want, wstatus, what: localise(got, status, plane, want, wstatus, POLL_SPEC, what), beside=dict(tensor=scan.gray_spec(POLL_SPEC)))


# ---------------------------------------------------------------------------------------------- memory that torch allocated
TORCH_CHILD = """
import sys
import torch                      # first: the process then holds ONE HIP runtime, torch's (INTEGRATION.md, section 3)
import numpy as np
import rectdetect_amd as ra
d = np.load(sys.argv[1])
frame, quads, pw, ph = d["frame"], d["quads"], int(d["pw"]), int(d["ph"])
ih, iw, n = frame.shape[0], frame.shape[1], len(quads)
dframe = ra.lib().rd_device_alloc(frame.nbytes)
ra.lib().rd_upload(dframe, frame.ctypes.data, frame.nbytes)
for name, mode in (("bits", ra.SCAN_BITS), ("flat", ra.SCAN_FLAT)):
    rect = ra.Rectifier(pw, ph, max_quads=n, njobs=1, scan=ra.scan_spec(mode, 8, 26, 0, oversample=2))
    t = torch.empty(rect.shape(n), dtype=torch.uint8, device="cuda")
    assert rect.patch_bytes * n == t.numel()
    t.fill_(7)
    torch.cuda.synchronize()      # the caller's own streams are done with the memory before the enqueue
    rect.enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, t.data_ptr(), on_device=True)
    status = rect.wait()          # after which the data is visible to every stream
    np.save(sys.argv[2] + name + ".npy", t.cpu().numpy())
    np.save(sys.argv[2] + name + "_status.npy", status)
    print(name, "sum", int(t.sum().item()), flush=True)      # a torch op on the tensor afterwards
    rect.close()
ra.lib().rd_device_free(dframe)
print("done", flush=True)
"""


def test_torch_tensors_are_written_through_data_ptr(tmp_path):
    """torch.uint8 tensors of packed bit rows and of flat pages, allocated by torch on the device and written through data_ptr(), read back with t.cpu(): the
    restatement's bytes.  In a child process, because what is tested is a process that imports torch first and so holds one HIP runtime."""
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = TW + 1, 9
    modes = {"bits": ra.SCAN_BITS, "flat": ra.SCAN_FLAT}
    child = rectjobs.torch_child(tmp_path, TORCH_CHILD, modes, frame=bgr, quads=quads, pw=pw, ph=ph)
    for name, mode in modes.items():
        want, wstatus = reference(ra.PIX_BGR, pw, ph, ra.scan_spec(mode, 8, 26, 0, oversample=2))
        got, status, total = child[name]
        scan.assert_pages(got, status, want, wstatus, name)
        assert int(total) == int(want.astype(np.int64).sum()), "torch summed the bytes the job wrote"


# ---------------------------------------------------------------------------------------------- the example program
def test_rdscan_writes_the_pages_of_the_restatement(tmp_path):
    """examples/rdscan on a PPM with a scan spec on its command line: every page_K.pbm is a P4 header and the restatement's bit rows, its size from rd_rect_aspect"""
    iw, ih, pw = 640, 480, 72
    img = cframe(synth.SEED0, iw, ih, 0)
    with open(tmp_path / "in.ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (iw, ih) + img[..., ::-1].tobytes())
    res = subprocess.run([os.path.join(helpers.ROOT, "examples", "rdscan"), str(tmp_path / "in.ppm"), "0", "page_", str(pw), "bits", "8", "30", "2", "230", "2", "0"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path, timeout=60)
    assert res.returncode == 0, res.stderr.decode()
    ctx = ra.Context(0)
    det = ra.RectDetector(ctx, iw, ih)
    rects = det.execute_once(img, np.tan(72.0 / 2 / 180.0 * np.pi))
    det.close()
    ctx.close()
    n = len(rects)
    text = res.stdout.decode()
    assert n > 0 and ("%d rectangle(s)" % n) in text
    spec = ra.scan_spec(ra.SCAN_BITS, 8, 30, 2, 230, 2)
    quads = ra.rect_quads(rects)
    for k in range(n):
        ph = min(max(int(np.floor(pw * ra.rect_aspect(rects[k]) + 0.5)), 1), 8192)
        want, st = scan.pages(img, quads[k:k + 1], pw, ph, spec)
        assert ("page %d x %d bits bytes %d " % (pw, ph, want.nbytes)) in text and ("-> page_%d.pbm" % k) in text
        assert open(tmp_path / ("page_%d.pbm" % k), "rb").read() == b"P4\n%d %d\n" % (pw, ph) + want.tobytes(), k
    res = subprocess.run([os.path.join(helpers.ROOT, "examples", "rdscan"), str(tmp_path / "in.ppm"), "0", "flat_", str(pw), "flat", "8"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path, timeout=60)
    assert res.returncode == 0, res.stderr.decode()
    ph = min(max(int(np.floor(pw * ra.rect_aspect(rects[0]) + 0.5)), 1), 16384)
    want, _ = scan.pages(img, quads[:1], pw, ph, ra.scan_spec(ra.SCAN_FLAT, 8))
    assert open(tmp_path / "flat_0.pgm", "rb").read() == b"P5\n%d %d\n255\n" % (pw, ph) + want.tobytes()
