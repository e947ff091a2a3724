"""Page components on the GPU (rd_rectifier_create_blobs, rd_blobs_pages_device): every byte equals the restatement of the header's contract (tests/blobs.py) and
rd_blob_page_host - the whole catalogue of crafted pages (tests/blobcases.py) through the component stage alone, several pages in one call, two rounds on one slot's
scratch, and the frame path: the scan tests' noise frames and quads with an invalid quad between valid ones, all six pixel formats, host / device / pinned frames,
device / pinned output, radii 1, 8 and 63, oversampling 1, 2 and 4, both polarities, the fixed level (radius 0) on frames sampled pixel for pixel, jobs in flight,
empty and full jobs, argument errors, behind the poll of both detector kinds, into memory that torch allocated, and from the example program.  Every frame-path case
also runs the RD_SCAN_BITS rectifier on the same job and compares the records with the restatement's steps 2-7 applied to THOSE bits, so that a failure names the
launch at fault.  Every output lies between guard bytes that must not change.  No tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import blobcases
from tests import blobs
from tests import helpers
from tests import pixfmt
from tests import rectjobs
from tests import tensor
from tests.rectjobs import L, Out, STATUS, case, cframe, gray_planes, mem, run_job      # (mem: the fixture)

pytestmark = pytest.mark.gpu
TW, TH = blobcases.TW, blobcases.TH
CASES = blobcases.cases()
GUARD = rectjobs.GUARD


def assert_rows(got, want, spec, pw, ph, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8, "%s: %r %r, expected %r" % (what, got.shape, got.dtype, want.shape)
    for q in range(len(want)):
        blobs.explain(got[q], want[q], spec, pw, ph, "%s: quad %d" % (what, q))


# ---------------------------------------------------------------------------------------------- the component stage alone
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_catalogue_through_the_component_stage(case):
    got, info = ra.blobs_pages(case.bits, case.pw, case.ph, case.spec, guard=GUARD)
    what = repr(case)
    assert info["path"] == 0 and (info["tiles_x"], info["tiles_y"]) == ((case.pw + TW - 1) // TW, (case.ph + TH - 1) // TH), info
    assert info["border"] == int(info["tiles_x"] * info["tiles_y"] > 1) and info["launches"] == 4 + info["border"], info
    blobs.explain(got[0], blobcases.want(case), case.spec, case.pw, case.ph, what + ": the restatement")
    blobs.explain(got[0], ra.blob_page_host(case.bits, case.pw, case.ph, case.spec), case.spec, case.pw, case.ph, what + ": rd_blob_page_host")


def mixed_pages(pw, ph, seed):
    """different pages of one size, a full one next to an empty one among them"""
    rng = np.random.default_rng(seed)
    board = (np.add.outer(np.arange(ph), np.arange(pw)) & 1) == 0
    masks = [rng.random((ph, pw)) < 0.58, np.ones((ph, pw), bool), np.zeros((ph, pw), bool), board, blobcases.spiral(pw, ph, 0, 2), rng.random((ph, pw)) < 0.2, np.zeros((ph, pw), bool),
             blobcases.comb(pw, ph, ph - 1, (0, ph))]
    return masks


@pytest.mark.parametrize("connectivity", (4, 8))
def test_no_leaks_between_the_quads_of_a_call(connectivity):
    pw, ph = 2 * TW + 3, 3 * TH - 1
    masks = mixed_pages(pw, ph, 3)
    spec = ra.blob_spec(connectivity=connectivity, min_area=2, max_area=5000, max_blobs=64, page=True)
    bits = np.stack([blobs.pack(m) for m in masks])
    got, info = ra.blobs_pages(bits, pw, ph, spec, guard=GUARD)
    want = np.stack([blobs.page(m, spec) for m in masks])
    assert_rows(got, want, spec, pw, ph, "eight pages in one call")
    assert not got[2].any() and not got[6].any(), "an empty page between full ones gives zero bytes"
    for q, m in enumerate(masks):      # and each page alone gives the same bytes
        assert np.array_equal(ra.blobs_pages(bits[q], pw, ph, spec, guard=GUARD)[0][0], got[q]), q


def test_tap_argument_errors():
    spec, bits, out, info = ra.blob_spec(), np.zeros(8, np.uint8), np.zeros(2048, np.uint64), np.zeros(8, np.int32)
    tap = L().rd_blobs_pages_device
    bad = ra.blob_spec(connectivity=5)
    for args in ((0, None, 8, 8, 1, spec.ctypes.data, out.ctypes.data, info.ctypes.data), (0, bits.ctypes.data, 8, 8, 1, None, out.ctypes.data, info.ctypes.data),
                 (0, bits.ctypes.data, 8, 8, 1, spec.ctypes.data, None, info.ctypes.data), (0, bits.ctypes.data, 8, 8, 1, spec.ctypes.data, out.ctypes.data, None),
                 (0, bits.ctypes.data, 8, 8, 0, spec.ctypes.data, out.ctypes.data, info.ctypes.data), (0, bits.ctypes.data, 8, 8, 65536, spec.ctypes.data, out.ctypes.data, info.ctypes.data),
                 (0, bits.ctypes.data, 0, 8, 1, spec.ctypes.data, out.ctypes.data, info.ctypes.data), (0, bits.ctypes.data, 8, 8, 1, bad.ctypes.data, out.ctypes.data, info.ctypes.data),
                 (0, bits.ctypes.data, 2048, 2048, 33, spec.ctypes.data, out.ctypes.data, info.ctypes.data)):      # (33 * 2^22 > 2^27)
        assert tap(*args) == -1, args
    assert not out.any()
    with pytest.raises(ValueError):
        ra.blobs_pages(np.zeros(7, np.uint8), 8, 8, spec)


# ---------------------------------------------------------------------------------------------- the frame path
def level_frame(mask, ink=0, paper=255):
    """(a gray BGR frame whose pixel (11 + i, 9 + j) is `ink` where mask[j, i] and `paper` elsewhere, the quad that samples it pixel for pixel (up to one gray level where ink meets paper: the interpolation rounds): test_gpu_scan's
    two-level quad, stretched to the mask's size)"""
    ph, pw = mask.shape
    g = np.full((ph + 20, pw + 24), paper, np.uint8)
    g[9:9 + ph, 11:11 + pw][mask] = ink
    quad = np.array([[(10.5, 8.5), (10.5 + pw, 8.5), (10.5 + pw, 8.5 + ph), (10.5, 8.5 + ph)]])
    return np.repeat(g[..., None], 3, axis=2), quad


def bits_of_the_job(mem, fmt, planes, iw, ih, quads, pw, ph, spec):
    """the RD_SCAN_BITS rectifier on the same job: ((n, ph, rb) pages, status)"""
    srect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=1, scan=blobs.scan_spec(spec))
    try:
        return run_job(srect, mem, fmt, planes, iw, ih, quads)
    finally:
        srect.close()


def localise(got, status, bitpages, want, wstatus, spec, pw, ph, what):
    """(a) against steps 2-7 of the restatement on the bits the GPU's scan launch made - a difference here is the component stage's -, (b) against the full
    restatement - a difference here alone lies in front of it"""
    assert np.array_equal(status, wstatus), "%s: status %r, expected %r" % (what, status.tolist(), wstatus.tolist())
    if bitpages is not None:
        assert_rows(got, blobs.from_pages(bitpages, status, pw, spec), spec, pw, ph, what + ": the component stage, from the GPU's own ink bits")
    assert_rows(got, want, spec, pw, ph, what + ": the full restatement")


def reference(fmt, pw, ph, spec, sel=None, seed=0):
    g, st = gray_planes(fmt, pw, ph, int(spec["oversample"]), seed)
    sel = list(range(len(st))) if sel is None else list(sel)
    return blobs.from_planes(g[sel], st[sel], spec), st[sel].copy()


def check_specs(mem, fmt, pw, ph, specs, kinds=(("device", "device", 0),), seed=0):
    iw, ih, planes, bgr, quads = case(fmt, seed)
    for spec in specs:
        want, wstatus = reference(fmt, pw, ph, spec, seed=seed)
        bitpages = bits_of_the_job(mem, fmt, planes, iw, ih, quads, pw, ph, spec)[0] if int(spec["radius"]) else None
        rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=2, blobs=spec)
        try:
            assert rect.patch_bytes == ra.blob_bytes(spec, pw, ph) == want.shape[1] and rect.dtype == np.uint8 and rect.shape(len(quads)) == want.shape
            for kind, out_kind, pad in kinds:
                got, status = run_job(rect, mem, fmt, planes, iw, ih, quads, kind, out_kind, pad)
                localise(got, status, bitpages, want, wstatus, spec, pw, ph, "%s %s %dx%d %s frame, %s output, pad %d" % (ra.PIX_NAMES[fmt], blobs.name(spec), pw, ph, kind, out_kind, pad))
                assert status.tolist() == STATUS.tolist() and not got[1].any(), "an invalid quad gives zero bytes"
        finally:
            rect.close()


def test_shared_reference_is_the_restatement():
    spec = ra.blob_spec(2, 26, 0, 2, True, 4, 2, 0, 8, True)
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    a, b = reference(ra.PIX_BGR, 9, 5, spec), blobs.job(bgr, quads, 9, 5, spec)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].tolist() == STATUS.tolist() and a[0].shape == (4, ra.blob_bytes(spec, 9, 5))


@pytest.mark.parametrize("radius", (1, 8, 63))
def test_radii_oversamplings_polarities_and_connectivities(radius, mem):
    pw, ph = 2 * TW + 3, TH + 1
    specs = [ra.blob_spec(radius, k, d, m, inv, conn, lo, hi, B, page)
             for (k, d), m, inv, conn, lo, hi, B, page in (((26, 0), 1, False, 8, 1, 0, 64, True), ((38, 7), 2, True, 4, 2, 40, 16, True), ((26, 0), 4, False, 4, 1, 0, 4096, False),
                                                           ((0, 0), 2, False, 8, 3, 0, 1, True), ((26, 0), 4, True, 8, 1, 0, 256, True))]
    check_specs(mem, ra.PIX_BGR, pw, ph, specs)


@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_every_format_frame_kind_and_output_kind(fmt, mem):
    kinds = [(kind, out_kind, 13 if kind == "device" else 0) for kind in ("host", "device", "pinned") for out_kind in ("device", "pinned")]
    check_specs(mem, fmt, TW + 1, TH + 2, [ra.blob_spec(8, 26, 0, 2, fmt % 2 == 1, (4, 8)[fmt % 2], 2, 0, 32, True)], kinds)


@pytest.mark.parametrize("pw,ph", ((1, 1), (7, 3), (9, 5), (64, 1), (65, 2), (TW, TH)), ids=lambda v: str(v))
def test_small_and_odd_pages_on_the_frame_path(pw, ph, mem):
    check_specs(mem, ra.PIX_BGR, pw, ph, [ra.blob_spec(2, 26, 0, 1, False, 8, 1, 0, 8, True), ra.blob_spec(0, 128, 0, 2, True, 4, 1, 0, 8, True)])


def fixed_level_cases():
    keep = ("corners", "full", "checker", "diagonal", "antidiagonal", "comb-joined-at-the-bottom", "comb-bar-on-the-next-tile's-first-row", "spiral", "two-spirals", "filter", "noise-60")
    return [c for c in CASES if c.name in keep and blobcases.SMALL(c)]


@pytest.mark.parametrize("case", fixed_level_cases(), ids=repr)
def test_fixed_level_brings_the_catalogue_to_the_frame_path_unchanged(case, mem):
    """radius 0 on a gray frame sampled pixel for pixel: ink = G <= k reproduces the case's mask, so the job's bytes are the case's"""
    frame, quad = level_frame(case.mask)
    spec = case.spec.copy()
    spec["radius"], spec["k"], spec["d"] = 0, 100, 0
    g0, st = tensor.tensors(frame, quad, case.pw, case.ph, blobs.gray_spec(spec))
    assert st.tolist() == [1] and np.array_equal(g0.reshape(case.ph, case.pw) <= 100, case.mask), "the quad samples the frame pixel for pixel"
    rect = ra.Rectifier(case.pw, case.ph, max_quads=1, njobs=1, blobs=spec)
    try:
        got, status = run_job(rect, mem, ra.PIX_BGR, [frame], frame.shape[1], frame.shape[0], quad)
    finally:
        rect.close()
    assert status.tolist() == [1]
    blobs.explain(got[0], blobs.page(case.mask, spec), spec, case.pw, case.ph, repr(case))


def test_fixed_level_at_its_ends_and_inverted(mem):
    """k = 255: everything is ink; k = 0 on a frame without black: nothing is; a level between the frame's two grays gives the mask, and inverted - the level then
    applies to 255 - G - its complement.  The expectation is the restatement's on the restatement's G plane."""
    pw, ph = TW + 5, TH + 3
    mask = np.random.default_rng(9).random((ph, pw)) < 0.5
    frame, quad = level_frame(mask, ink=40, paper=200)
    g0, st = tensor.tensors(frame, quad, pw, ph, ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, 1))
    g0 = g0.reshape(ph, pw)
    for k, invert, claim in ((255, False, np.ones_like(mask)), (0, False, np.zeros_like(mask)), (120, False, mask), (30, False, np.zeros_like(mask)), (120, True, ~mask), (255, True, np.ones_like(mask))):
        spec = ra.blob_spec(0, k, 0, 1, invert, 8, 1, 0, 4096, True)
        ink = blobs.ink(g0, spec)
        assert np.array_equal(ink, claim), (k, invert)
        rect = ra.Rectifier(pw, ph, max_quads=1, njobs=1, blobs=spec)
        try:
            got, status = run_job(rect, mem, ra.PIX_BGR, [frame], frame.shape[1], frame.shape[0], quad)
        finally:
            rect.close()
        blobs.explain(got[0], blobs.page(ink, spec), spec, pw, ph, "k %d invert %d" % (k, invert))
        if k == 255:
            h, r, _ = ra.blob_view(got, spec, pw, ph)
            assert int(h[0]["all"]) == 1 and int(r[0][0]["area"]) == pw * ph


def test_no_stale_scratch_in_two_rounds_on_one_slot(mem):
    """one slot (njobs = 1), the same quads, different pages from round to round - a full page before an empty one in the same place among them"""
    pw, ph = 2 * TW + 3, 2 * TH + 5
    spec = ra.blob_spec(0, 100, 0, 1, False, 8, 2, 0, 64, True)
    rounds = (mixed_pages(pw, ph, 11)[:4], mixed_pages(pw, ph, 12)[1:5][::-1], mixed_pages(pw, ph, 13)[4:8])
    rect = ra.Rectifier(pw, ph, max_quads=4, njobs=1, blobs=spec)
    try:
        for rnd, masks in enumerate(rounds):
            wide = np.zeros((ph + 20, 4 * (pw + 24), 3), np.uint8)
            quads = []
            for q, m in enumerate(masks):
                frame, quad = level_frame(m)
                wide[:, q * (pw + 24):(q + 1) * (pw + 24)] = frame
                quads.append(quad[0] + (q * (pw + 24), 0))
            got, status = run_job(rect, mem, ra.PIX_BGR, [wide], wide.shape[1], wide.shape[0], np.array(quads))
            assert status.tolist() == [1] * 4
            assert_rows(got, np.stack([blobs.page(m, spec) for m in masks]), spec, pw, ph, "round %d" % rnd)
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- jobs in flight, empty and full jobs, argument errors
def test_four_jobs_in_flight_on_four_frames(mem):
    pw, ph, njobs = TW + 1, TH + 2, 4
    spec = ra.blob_spec(8, 26, 0, 2, False, 8, 2, 0, 32, True)
    rect = ra.Rectifier(pw, ph, max_quads=4, njobs=njobs, blobs=spec)
    try:
        for rnd in range(2):      # (the second round reuses every slot's planes)
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
                localise(out.fetch().reshape(rect.shape(len(sel))), status, None, want, wstatus, spec, pw, ph, "round %d job %d" % (rnd, k))
        with pytest.raises(RuntimeError):
            rect.wait()      # nothing in flight
    finally:
        rect.close()


def test_empty_job_and_full_job(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_RGBA)
    pw, ph = 9, 5
    spec = ra.blob_spec(2, 26, 0, 4, False, 4, 1, 0, 8, True)
    want, wstatus = reference(ra.PIX_RGBA, pw, ph, spec)
    nmax = 2 * len(quads)
    rect = ra.Rectifier(pw, ph, max_quads=nmax, njobs=2, blobs=spec)
    try:
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.zeros((0, 4, 2)))      # n = 0: nothing written, nothing returned
        assert got.shape == (0, rect.patch_bytes) and len(status) == 0
        assert rect.enqueue(ra.PIX_RGBA, planes, None, iw, ih, np.zeros((0, 8)), None) == 1      # (no output buffer needed either)
        assert len(rect.wait()) == 0
        full = np.concatenate([quads, quads[::-1]])
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, full, "host", "pinned")      # n = max_quads
        localise(got, status, None, np.concatenate([want, want[::-1]]), np.concatenate([wstatus, wstatus[::-1]]), spec, pw, ph, "full job")
        with pytest.raises(ValueError):
            run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.concatenate([full, quads[:1]]))      # one more
        conv = rect.rectify(bgr, quads)      # the convenience call
        assert_rows(conv, want, spec, pw, ph, "rectify()")
        heads, recs, pages = ra.blob_view(conv, spec, pw, ph)
        wh, wr, wp = blobs.view(want, spec, pw, ph)
        assert np.array_equal(heads, wh) and np.array_equal(recs, wr) and np.array_equal(pages, wp)
    finally:
        rect.close()


def test_argument_errors_return_minus_one_or_null_and_the_next_job_is_correct(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = TW + 1, 9
    spec = ra.blob_spec(8, 26, 0, 2, False, 8, 2, 100, 16, True)
    want, wstatus = reference(ra.PIX_BGR, pw, ph, spec)
    create = lambda *a: L().rd_rectifier_create_blobs(*a)
    assert not create(0, pw, ph, 4, 1, None)      # a NULL spec
    for field, v in (("radius", -1), ("radius", 64), ("k", 256), ("k", -1), ("d", 256), ("d", -1), ("oversample", 3), ("invert", 2), ("connectivity", 6), ("min_area", 0), ("min_area", 101),
                     ("max_area", 1), ("max_area", (1 << 22) + 1), ("max_blobs", 0), ("max_blobs", 4097), ("page", 2), ("reserved", 1)):
        bad = spec.copy()
        bad[field] = v
        assert not create(0, pw, ph, 4, 1, bad.ctypes.data), field
        with pytest.raises(ValueError):
            ra.Rectifier(pw, ph, blobs=bad)
    bad = ra.blob_spec(radius=0, d=1)
    assert not create(0, pw, ph, 4, 1, bad.ctypes.data)      # a fixed level has no d
    with pytest.raises(ValueError):
        ra.Rectifier(pw, ph, blobs=spec, scan=ra.scan_spec(ra.SCAN_BITS))      # one or the other
    for args in ((0, 0, ph, 4, 1), (0, pw, 0, 4, 1), (0, 8193, ph, 4, 1), (0, pw, 8193, 4, 1), (0, pw, ph, 0, 1), (0, pw, ph, 4, 0), (99, pw, ph, 4, 1), (0, 2048, 2049, 1, 1)):
        assert not create(*args, spec.ctypes.data), args      # rd_rectifier_create's bad arguments (pw * m > 16384 among them), a page of more than 2^22 pixels
    one = ra.blob_spec(oversample=1)
    assert not create(0, 2048, 2048, 33, 1, one.ctypes.data) and not create(0, 1024, 1024, 129, 1, one.ctypes.data)      # max_quads * pw * ph > 2^27
    h = create(0, 1024, 1024, 128, 1, one.ctypes.data)      # exactly 2^27: made (its scratch is allocated on first use only)
    assert h
    L().rd_rectifier_destroy(h)
    rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=1, blobs=spec)
    out = Out(mem, "device", len(quads) * rect.patch_bytes + 8)
    try:
        assert out.ptr % 8 == 0
        q = rectjobs.refused_enqueues(mem, rect, planes, iw, ih, quads, out, {"out misaligned by 4": dict(out_p=out.ptr + 4)})
        status = rect.wait()
        localise(out.fetch(len(q) * rect.patch_bytes).reshape(rect.shape(len(q))), status, None, want, wstatus, spec, pw, ph, "the job after the refused ones")
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- behind the detector's poll
PW, PH = rectjobs.PW, rectjobs.PH
POLL_SPEC = ra.blob_spec(15, 26, 0, 2, False, 8, 3, 0, 128, True)


@pytest.mark.parametrize("kind", ["rect-host", "poly-device", "scaled"])
def test_rectify_polled_behind_every_poll(kind, mem):
    """after Detector.poll and PolylineDetector.poll, on host frames and device frames, and on a frame that came in at scale 2 - quads in detector coordinates, the
    page from the full-size source (X = 2x + 0.5)"""
    rectjobs.polled_behind_a_poll(mem, kind, dict(blobs=POLL_SPEC), lambda bgr, quads: blobs.job(bgr, quads, PW, PH, POLL_SPEC),
                                  lambda got, status, bitpages, want, wstatus, what: localise(got, status, bitpages, want, wstatus, POLL_SPEC, PW, PH, what), beside=dict(scan=blobs.scan_spec(POLL_SPEC)),
                                  nframes=2)


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
rect = ra.Rectifier(pw, ph, max_quads=n, njobs=1, blobs=ra.blob_spec(8, 26, 0, 2, False, 8, 2, 0, 32, True))
t = torch.empty(rect.shape(n), dtype=torch.uint8, device="cuda")
assert rect.patch_bytes * n == t.numel() and t.data_ptr() % 8 == 0
t.fill_(7)
torch.cuda.synchronize()      # the caller's own streams are done with the memory before the enqueue
rect.enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, t.data_ptr(), on_device=True)
status = rect.wait()          # after which the data is visible to every stream
np.save(sys.argv[2] + "blobs.npy", t.cpu().numpy())
np.save(sys.argv[2] + "blobs_status.npy", status)
print("blobs sum", int(t.sum().item()), flush=True)      # a torch op on the tensor afterwards
rect.close()
ra.lib().rd_device_free(dframe)
print("done", flush=True)
"""


def test_torch_tensors_are_written_through_data_ptr(tmp_path):
    """a torch.uint8 tensor allocated by torch on the device and written through data_ptr(), read back with t.cpu(): the restatement's bytes.  In a child process,
    because what is tested is a process that imports torch first and so holds one HIP runtime."""
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = TW + 1, TH + 2
    got, status, total = rectjobs.torch_child(tmp_path, TORCH_CHILD, ["blobs"], frame=bgr, quads=quads, pw=pw, ph=ph)["blobs"]
    spec = ra.blob_spec(8, 26, 0, 2, False, 8, 2, 0, 32, True)
    want, wstatus = reference(ra.PIX_BGR, pw, ph, spec)
    localise(got, status, None, want, wstatus, spec, pw, ph, "torch")
    assert int(total) == int(want.astype(np.int64).sum()), "torch summed the bytes the job wrote"


# ---------------------------------------------------------------------------------------------- the example program
def test_rdblobs_prints_the_heads_and_boxes_and_writes_the_clean_pages_of_the_restatement(tmp_path):
    """examples/rdblobs on a PPM with a blob spec on its command line: the printed head and boxes and every clean_K.pbm are the restatement's"""
    iw, ih, pw = 640, 480, 72
    img = cframe(synth.SEED0, iw, ih, 0)
    with open(tmp_path / "in.ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (iw, ih) + img[..., ::-1].tobytes())
    res = subprocess.run([os.path.join(helpers.ROOT, "examples", "rdblobs"), str(tmp_path / "in.ppm"), "0", "clean_", str(pw), "8", "30", "2", "2", "0", "4", "3", "0", "16"],
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
    spec = ra.blob_spec(8, 30, 2, 2, False, 4, 3, 0, 16, True)
    quads = ra.rect_quads(rects)
    for k in range(n):
        ph = min(max(int(np.floor(pw * ra.rect_aspect(rects[k]) + 0.5)), 1), 8192)
        want, st = blobs.job(img, quads[k:k + 1], pw, ph, spec)
        heads, recs, pages = blobs.view(want, spec, pw, ph)
        h = heads[0]
        line = "page %d x %d ink %d all %d found %d written %d ink_kept %d largest %d flags %d " % ((pw, ph) + tuple(int(h[f]) for f in ("ink", "all", "found", "written", "ink_kept", "largest", "flags")))
        assert line in text and ("-> clean_%d.pbm" % k) in text, (k, line)
        block = text[text.index("-> clean_%d.pbm" % k):]
        block = block[:block.index("\nstatus ", 1)] if "\nstatus " in block[1:] else block
        printed = [ln.strip() for ln in block.splitlines()[1:] if ln.startswith("  blob ")]
        assert printed == ["blob %d box %d %d %d %d area %d first %d sx %d sy %d" % ((b,) + tuple(int(recs[0][b][f]) for f in ("x0", "y0", "x1", "y1", "area", "first", "sx", "sy"))) for b in range(int(h["written"]))], k
        assert open(tmp_path / ("clean_%d.pbm" % k), "rb").read() == b"P4\n%d %d\n" % (pw, ph) + pages[0].tobytes(), k
