"""Graded quads on the GPU (rd_rectifier_create_grade): every byte equals the numpy restatement of the header's contract (tests/grade.py on tests/tensor.py's gray
plane) - for every cells, oversampling and both hist values, output sizes on every side of the 64-pixel wave row and the kernel's tile, with cell edges inside a
wave's row, on a tile's edge and one pixel per cell, thresholds at their ends on noise, constant frames and a one-pixel checkerboard, the sums past 2^32, all six
pixel formats, host / device / pinned frames, device / pinned output, invalid quads, outputs reused by later jobs (the zeroing), jobs in flight, empty and full
jobs, argument errors, behind the poll of both detector kinds, into memory that torch allocated, and from the example program.  Every case also runs the
{ U8, NHWC, GRAY, m } tensor rectifier on the same job and compares the records with the restatement's steps 2-5 applied to THAT plane, so that a failure names the
launch at fault.  Every device output lies between guard bytes that must not change.  No tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import grade
from tests import helpers
from tests import pixfmt
from tests import rectjobs
from tests import tensor
from tests.rectjobs import L, Out, STATUS, case, cframe, gray_job, gray_planes, job_quads, mem, run_job      # (mem: the fixture)

pytestmark = pytest.mark.gpu
TW, TH = ra.grade_limits()["tile_w"], ra.grade_limits()["tile_h"]
# one pixel; one pixel per cell at cells = 8; cell edges that are no multiple of anything; one short of the 64-pixel wave row, the row, one more; the tile, one pixel
# into the next tile in both directions, three tile columns with a tail one row short of the tile, and four tile rows with a tail
SIZES = ((1, 1), (8, 8), (9, 5), (63, 2), (64, 1), (65, 2), (TW, TH), (TW + 1, TH + 1), (2 * TW + 3, TH - 1), (100, 3 * TH + 1))
THRESHOLDS = ((8, 247, 64), (0, 255, 0), (255, 0, 1020), (100, 100, 300))      # (dark, bright, edge): the defaults, each at both ends, and values in between


def reference(fmt, pw, ph, spec, sel=None, seed=0):
    """(the bytes of the case's quads - or of those in sel -, status) from the shared planes"""
    g, st = gray_planes(fmt, pw, ph, int(spec["oversample"]), seed)
    sel = list(range(len(st))) if sel is None else list(sel)
    return grade.from_planes(g[sel], st[sel], spec), st[sel].copy()


def test_shared_reference_is_the_restatement():
    spec = ra.grade_spec(2, oversample=2, hist=True)
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    a, b = reference(ra.PIX_BGR, 9, 5, spec), grade.records(bgr, quads, 9, 5, spec)
    grade.assert_records(a[0], a[1], b[0], b[1], spec)
    assert a[1].tolist() == STATUS.tolist() and a[0].shape == (4, 4 * 48 + 1024)


def localise(got, status, gpu_plane, want, wstatus, spec, what):
    """(a) the records against steps 2-5 of the restatement on the plane the GPU's first launch made - a difference here is the grade kernel's -, (b) against the
    full restatement - a difference here alone is the tensor kernel's"""
    grade.assert_records(got, status, grade.from_planes(gpu_plane, status, spec), wstatus, spec, what + ": rdk::grade, from the GPU's own G plane")
    grade.assert_records(got, status, want, wstatus, spec, what + ": the full restatement")


def check_specs(mem, fmt, pw, ph, specs, kinds=(("device", "device", 0),), seed=0):
    """every spec on the case's job, with the tensor rectifier's plane of the same job (one per oversampling)"""
    iw, ih, planes, bgr, quads = case(fmt, seed)
    plane_of = {}
    for spec in specs:
        m = int(spec["oversample"])
        if m not in plane_of:
            plane_of[m], pstatus = gray_job(mem, fmt, planes, iw, ih, quads, pw, ph, m)
            assert pstatus.tolist() == STATUS.tolist()
        want, wstatus = reference(fmt, pw, ph, spec, seed=seed)
        rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=2, grade=spec)
        try:
            assert rect.patch_bytes == ra.grade_bytes(spec, pw, ph) == want[0].nbytes and rect.dtype == np.uint8 and rect.shape(len(quads)) == want.shape
            for kind, out_kind, pad in kinds:
                got, status = run_job(rect, mem, fmt, planes, iw, ih, quads, kind, out_kind, pad)
                localise(got, status, plane_of[m], want, wstatus, spec, "%s %s %dx%d %s frame, %s output, pad %d" % (ra.PIX_NAMES[fmt], grade.name(spec), pw, ph, kind, out_kind, pad))
                assert not got[1].any(), "an invalid quad gives zero bytes"
        finally:
            rect.close()


# ---------------------------------------------------------------------------------------------- every size at every cells; every oversampling, both hist values
def size_specs(pw, ph, k):
    """one spec per legal cells for size number k: over the sizes every cells meets every oversampling, both hist values and every threshold set"""
    out = []
    for n, c in enumerate(grade.CELLS):
        if min(pw, ph) >= c:
            dark, bright, edge = THRESHOLDS[(k + n) % 4]
            out.append(ra.grade_spec(c, dark, bright, edge, (1, 2, 4)[(k + n) % 3], (k + n // 2) % 2 == 1))
    return out


def test_the_size_specs_meet_every_value():
    met = {(int(s["cells"]), int(s["oversample"]), int(s["hist"])) for k, (pw, ph) in enumerate(SIZES) for s in size_specs(pw, ph, k)}
    for c in grade.CELLS:
        assert {m for cc, m, h in met if cc == c} == {1, 2, 4} and {h for cc, m, h in met if cc == c} == {0, 1}, c
    assert [len(size_specs(pw, ph, 0)) for pw, ph in SIZES] == [1, 4, 3, 2, 1, 2, 4, 4, 4, 4]


@pytest.mark.parametrize("k", range(len(SIZES)), ids=["%dx%d" % s for s in SIZES])
def test_every_output_size_at_every_cells(k, mem):
    pw, ph = SIZES[k]
    check_specs(mem, ra.PIX_BGR, pw, ph, size_specs(pw, ph, k))
    for c in grade.CELLS:
        if min(pw, ph) < c:
            with pytest.raises(ValueError):
                ra.Rectifier(pw, ph, grade=ra.grade_spec(c))      # a cell would be empty


@pytest.mark.parametrize("cells", grade.CELLS)
def test_full_cross_of_oversampling_hist_and_thresholds(cells, mem):
    check_specs(mem, ra.PIX_BGR, TW + 1, TH + 1, [ra.grade_spec(cells, d, b, e, m, h) for m in (1, 2, 4) for h in (False, True) for d, b, e in THRESHOLDS[h::2]])


# ---------------------------------------------------------------------------------------------- formats, frame kinds, output kinds
@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_every_format_frame_kind_and_output_kind(fmt, mem):
    kinds = [(kind, out_kind, 13 if kind == "device" else 0) for kind in ("host", "device", "pinned") for out_kind in ("device", "pinned")]
    check_specs(mem, fmt, TW + 1, 9, [ra.grade_spec(grade.CELLS[fmt % 4], oversample=2, hist=fmt % 2 == 1)], kinds)


# ---------------------------------------------------------------------------------------------- thresholds at their ends; frames that meet the contract's special cases
END_SPECS = [ra.grade_spec(c, d, b, e, 1, True) for c, (d, b, e) in zip((1, 2, 4, 8, 4, 2), ((0, 0, 0), (255, 255, 1020), (0, 255, 0), (255, 0, 1020), (93, 93, 1), (92, 94, 1019)))]


def test_thresholds_at_their_ends_on_noise(mem):
    check_specs(mem, ra.PIX_BGR, TW + 1, TH + 1, END_SPECS)
    spec = END_SPECS[0]      # dark 0, bright 0, edge 0
    cells, hist = ra.grade_view(reference(ra.PIX_BGR, TW + 1, TH + 1, spec)[0][[0, 2, 3]], spec)
    assert np.array_equal(cells["ne"], cells["n"]) and np.array_equal(cells["hi"], cells["n"]), "edge 0 and bright 0: every pixel counts"
    assert np.array_equal(cells["lo"][:, 0, 0], hist[:, 0])


def test_constant_frames(mem):
    """a constant frame: G is the constant (step 1, asserted on the tensor rectifier's plane), L = 0, the records in closed form"""
    iw, ih, pw, ph = 97, 61, TW + 1, TH + 1
    quads = job_quads(iw, ih)
    for v in (0, 93, 255):
        frame = np.full((ih, iw, 3), v, np.uint8)
        plane, pstatus = gray_job(mem, ra.PIX_BGR, [frame], iw, ih, quads, pw, ph, 1)
        assert (plane[pstatus == 1] == v).all() and not plane[1].any() and pstatus.tolist() == STATUS.tolist()
        for spec in END_SPECS:
            rect = ra.Rectifier(pw, ph, max_quads=4, njobs=1, grade=spec)
            try:
                got, status = run_job(rect, mem, ra.PIX_BGR, [frame], iw, ih, quads)
            finally:
                rect.close()
            grade.assert_records(got, status, grade.from_planes(plane, pstatus, spec), STATUS, spec, "constant %d %s" % (v, grade.name(spec)))
            cells, hist = ra.grade_view(got[[0, 2, 3]], spec)
            n = cells["n"].astype(np.int64)
            assert int(n.sum()) == 3 * pw * ph and (hist[:, v] == pw * ph).all() and int(hist.sum()) == 3 * pw * ph
            assert np.array_equal(cells["sg"], n * v) and np.array_equal(cells["sgg"], n * v * v) and not cells["sl"].any() and not cells["sll"].any()
            assert np.array_equal(cells["lo"], n * (v <= int(spec["dark"]))) and np.array_equal(cells["hi"], n * (v >= int(spec["bright"]))) and np.array_equal(cells["ne"], n * (0 >= int(spec["edge"])))
        mem.close()


def test_one_pixel_checkerboard_carries_sll_past_32_bits(mem):
    """0 and 255 in a one-pixel checkerboard, sampled pixel for pixel: L = +-1020 in the interior, and the 64 x 128 patch has sll > 2^32"""
    iw, ih, pw, ph = 97, 150, 64, 128
    yy, xx = np.mgrid[0:ih, 0:iw]
    frame = np.repeat(np.where((xx + yy) & 1, 255, 0).astype(np.uint8)[..., None], 3, axis=2)
    quad = np.array([[(10.5, 8.5), (74.5, 8.5), (74.5, 136.5), (10.5, 136.5)]])      # patch pixel (i, j) is frame pixel (11 + i, 9 + j)
    g, st = tensor.tensors(frame, quad, pw, ph, ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, 1))
    g = g.reshape(1, ph, pw)
    assert np.array_equal(g[0], frame[9:9 + ph, 11:11 + pw, 0]) and (np.abs(grade.laplacian(g[0]))[1:-1, 1:-1] == 1020).all()
    plane, pstatus = gray_job(mem, ra.PIX_BGR, [frame], iw, ih, quad, pw, ph, 1)
    for spec in END_SPECS + [ra.grade_spec(1, 0, 255, 1020)]:
        rect = ra.Rectifier(pw, ph, max_quads=1, njobs=1, grade=spec)
        try:
            got, status = run_job(rect, mem, ra.PIX_BGR, [frame], iw, ih, quad)
        finally:
            rect.close()
        localise(got, status, plane, grade.from_planes(g, st, spec), st, spec, "checkerboard " + grade.name(spec))
        cells, _ = ra.grade_view(got, spec)
        assert int(cells["sll"].sum()) > 2 ** 32 and int(cells["sll"].sum()) >= 62 * 126 * 1020 * 1020
        if int(spec["edge"]) == 1020:
            assert int(cells["ne"].sum()) == 62 * 126, "the interior is on an edge at the largest threshold, the border is not"


def closed_form(n, v, spec):
    """the record of n pixels of the constant v"""
    r = np.zeros((), ra.GRADE_CELL_DTYPE)
    r["n"], r["lo"], r["hi"], r["ne"] = n, n * (v <= int(spec["dark"])), n * (v >= int(spec["bright"])), n * (0 >= int(spec["edge"]))
    r["sg"], r["sgg"] = n * v, n * v * v
    return r


@pytest.mark.parametrize("side", [258, 4105])
def test_constant_255_carries_the_sums_of_g_past_32_bits(side, mem):
    """one cell over a side x side patch of 255s: sgg > 2^32 at 258, sg > 2^32 at 4105 (step 1 for a constant frame: test_constant_frames)"""
    iw, ih = 97, 61
    frame = np.full((ih, iw, 3), 255, np.uint8)
    quad = job_quads(iw, ih)[:1]
    spec = ra.grade_spec(1, 8, 247, 64, hist=True)
    rect = ra.Rectifier(side, side, max_quads=1, njobs=1, grade=spec)
    try:
        got, status = run_job(rect, mem, ra.PIX_BGR, [frame], iw, ih, quad)
    finally:
        rect.close()
    n = side * side
    want = closed_form(n, 255, spec)
    assert int(want["sgg"]) > 2 ** 32 and (side == 258 or int(want["sg"]) > 2 ** 32)
    restated = grade.from_planes(np.full((1, side, side), 255, np.uint8), [1], spec)
    wc, wh = ra.grade_view(restated, spec)
    assert wc[0, 0, 0] == want and int(wh[0, 255]) == n
    grade.assert_records(got, status, restated, [1], spec, "%d x %d of 255" % (side, side))


# ---------------------------------------------------------------------------------------------- the zeroing, jobs in flight, empty and full jobs, argument errors
def test_the_same_output_reused_by_consecutive_jobs_is_not_doubled(mem):
    pw, ph = TW + 1, TH + 1
    spec = ra.grade_spec(4, hist=True)
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    for out_kind in ("device", "pinned"):
        rect = ra.Rectifier(pw, ph, max_quads=4, njobs=2, grade=spec)
        out = Out(mem, out_kind, 4 * rect.patch_bytes)
        try:
            for rnd, sel in enumerate(([0, 1, 2, 3], [0, 1, 2, 3], [2, 0], [1], [3, 2, 0])):      # (a shorter job leaves the rest of the buffer as the job before left it)
                got, status = run_job(rect, mem, ra.PIX_BGR, planes, iw, ih, quads[sel], out_kind=out_kind, out=out)
                want, wstatus = reference(ra.PIX_BGR, pw, ph, spec, sel)
                grade.assert_records(got, status, want, wstatus, spec, "%s output, job %d" % (out_kind, rnd))
                after = out.fetch()
                assert rnd == 0 or np.array_equal(after[got.size:], before[got.size:]), "job %d wrote behind its last byte" % rnd
                before = after
        finally:
            rect.close()


def test_four_jobs_in_flight_over_two_rounds_into_the_same_outputs(mem):
    pw, ph, njobs = TW + 1, 5, 4
    spec = ra.grade_spec(2, oversample=2, hist=True)
    rect = ra.Rectifier(pw, ph, max_quads=4, njobs=njobs, grade=spec)
    outs = [Out(mem, "device" if k % 2 == 0 else "pinned", 4 * rect.patch_bytes) for k in range(njobs)]
    try:
        for rnd in range(2):      # (the second round reuses every slot's G plane, every staging buffer and every output)
            pending = []
            for k in range(njobs):
                iw, ih, planes, bgr, quads = case(ra.PIX_BGR, seed=k)
                sel = list(range(4))[k % 2:4 - k // 2] if rnd else list(range(4))
                args, pitches, kw = mem.place("device", planes, 5)
                assert rect.enqueue(ra.PIX_BGR, args, pitches, iw, ih, quads[sel], outs[k].ptr, out_pinned=k % 2 == 1, **kw) == rnd * njobs + k
                pending.append((k, sel))
            for k, sel in pending:
                status = rect.wait()
                want, wstatus = reference(ra.PIX_BGR, pw, ph, spec, sel, seed=k)
                grade.assert_records(outs[k].fetch()[:len(sel) * rect.patch_bytes].reshape(rect.shape(len(sel))), status, want, wstatus, spec, "round %d job %d" % (rnd, k))
        with pytest.raises(RuntimeError):
            rect.wait()      # nothing in flight
    finally:
        rect.close()


def test_empty_job_and_full_job_of_64_quads(mem):
    """n = 0; n = max_quads = 64 quads of 8 x 8 with 8 x 8 cells - many blocks, few records each; one quad too many"""
    iw, ih, planes, bgr, quads4 = case(ra.PIX_RGBA)
    rng = np.random.default_rng(41)
    base = np.array([(0.0, 0.0), (30.0, 2.0), (28.0, 26.0), (-3.0, 22.0)])
    quads = np.array([base + rng.uniform(0, 60, 2) * (1.0, 0.5) + rng.uniform(-2, 2, (4, 2)) for _ in range(64)])
    quads[17] = quads4[1]      # an invalid one
    pw = ph = 8
    spec = ra.grade_spec(8, oversample=4, hist=True)
    want, wstatus = grade.records(bgr, quads, pw, ph, spec)
    assert wstatus.sum() == 63 and not wstatus[17]
    rect = ra.Rectifier(pw, ph, max_quads=64, njobs=2, grade=spec)
    try:
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.zeros((0, 4, 2)))      # n = 0: nothing written, nothing returned
        assert got.shape == (0, rect.patch_bytes) and len(status) == 0
        assert rect.enqueue(ra.PIX_RGBA, planes, None, iw, ih, np.zeros((0, 8)), None) == 1      # (no output buffer needed either)
        assert len(rect.wait()) == 0
        plane, pstatus = gray_job(mem, ra.PIX_RGBA, planes, iw, ih, quads, pw, ph, 4)
        for kind, out_kind in (("device", "device"), ("host", "pinned")):
            got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, quads, kind, out_kind)      # n = max_quads
            localise(got, status, plane, want, wstatus, spec, "full job, %s output" % out_kind)
        with pytest.raises(ValueError):
            run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.concatenate([quads, quads[:1]]))      # one more
        conv = rect.rectify(bgr, quads[:5])      # the convenience call
        grade.assert_records(conv, wstatus[:5], want[:5], wstatus[:5], spec, "rectify()")
        cells, hist = ra.grade_view(conv, spec)
        assert cells.shape == (5, 8, 8) and (cells["n"] == 1).all() and hist.shape == (5, 256) and (hist.sum(1) == 64).all()
    finally:
        rect.close()


def test_argument_errors_return_minus_one_and_the_next_job_is_correct(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = TW + 1, 9
    spec = ra.grade_spec(4, oversample=2, hist=True)
    want, wstatus = reference(ra.PIX_BGR, pw, ph, spec)
    create = lambda *a: L().rd_rectifier_create_grade(*a)
    assert not create(0, pw, ph, 4, 1, None)      # a NULL spec
    for field, v in (("cells", 0), ("cells", 3), ("cells", 16), ("dark", -1), ("dark", 256), ("bright", -1), ("bright", 256), ("edge", -1), ("edge", 1021), ("oversample", 3), ("oversample", 0), ("hist", 2),
                     ("hist", -1), ("reserved", (1, 0)), ("reserved", (0, 1))):
        bad = spec.copy()
        bad[field] = v
        assert not create(0, pw, ph, 4, 1, bad.ctypes.data), field
        with pytest.raises(ValueError):
            ra.Rectifier(pw, ph, grade=bad)
    for other in (dict(tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, 2)), dict(scan=ra.scan_spec(ra.SCAN_FLAT))):
        with pytest.raises(ValueError):
            ra.Rectifier(pw, ph, grade=spec, **other)      # one or the other
    for args in ((0, 0, ph, 4, 1), (0, pw, 0, 4, 1), (0, 3, ph, 4, 1), (0, pw, 3, 4, 1), (0, 8193, ph, 4, 1), (0, pw, 8193, 4, 1), (0, pw, ph, 0, 1), (0, pw, ph, 4, 0), (99, pw, ph, 4, 1)):
        assert not create(*args, spec.ctypes.data), args      # rd_rectifier_create's bad arguments (pw < cells and pw * m > 16384 among them)
    rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=1, grade=spec)
    out = Out(mem, "device", len(quads) * rect.patch_bytes + 8)
    pinned = mem.out("pinned", len(quads) * rect.patch_bytes + 8)
    try:
        q = rectjobs.refused_enqueues(mem, rect, planes, iw, ih, quads, out, {"out misaligned by 4": dict(out_p=out.ptr + 4), "pinned out misaligned by 4": dict(out_p=pinned + 4, out_kind=2)})
        status = rect.wait()
        grade.assert_records(out.fetch()[:len(q) * rect.patch_bytes].reshape(rect.shape(len(q))), status, want, wstatus, spec, "the job after the refused ones")
        assert (out.fetch()[len(q) * rect.patch_bytes:] == 0xA5).all()
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- behind the detector's poll
POLL_SPEC = ra.grade_spec(4, oversample=2, hist=True)


@pytest.mark.parametrize("kind", ["rect-host", "rect-device", "poly-host", "poly-device", "scaled"])
def test_rectify_polled_behind_every_poll(kind, mem):
    """after Detector.poll and PolylineDetector.poll, on host frames (the detector's own copy) and device frames, and on a frame that came in at scale 2 - quads in
    detector coordinates, the records from the full-size source (X = 2x + 0.5)"""
    rectjobs.polled_behind_a_poll(mem, kind, dict(grade=POLL_SPEC), lambda bgr, quads: grade.records(bgr, quads, rectjobs.PW, rectjobs.PH, POLL_SPEC),
                                  lambda got, status, plane, want, wstatus, what: localise(got, status, plane, want, wstatus, POLL_SPEC, what), beside=dict(tensor=grade.gray_spec(POLL_SPEC)),
                                  misaligned_refused=True, out_reused=True)


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
for name, hist in (("cells", False), ("hist", True)):
    rect = ra.Rectifier(pw, ph, max_quads=n, njobs=1, grade=ra.grade_spec(4, oversample=2, hist=hist))
    t = torch.empty(rect.shape(n), dtype=torch.uint8, device="cuda")
    assert rect.patch_bytes * n == t.numel() and t.data_ptr() % 8 == 0
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
    """torch.uint8 tensors of records, with and without the histogram, allocated by torch on the device and written through data_ptr(), read back with t.cpu(): the
    restatement's bytes.  In a child process, because what is tested is a process that imports torch first and so holds one HIP runtime."""
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = TW + 1, 9
    hists = {"cells": False, "hist": True}
    child = rectjobs.torch_child(tmp_path, TORCH_CHILD, hists, frame=bgr, quads=quads, pw=pw, ph=ph)
    for name, hist in hists.items():
        spec = ra.grade_spec(4, oversample=2, hist=hist)
        want, wstatus = reference(ra.PIX_BGR, pw, ph, spec)
        got, status, total = child[name]
        grade.assert_records(got, status, want, wstatus, spec, name)
        assert int(total) == int(want.astype(np.int64).sum()), "torch summed the bytes the job wrote"


# ---------------------------------------------------------------------------------------------- the example program
def test_rdgrade_prints_the_numbers_of_the_restatement(tmp_path):
    """examples/rdgrade on a PPM with a grade spec on its command line: every cell's counts and sharpness (%.17g: every bit) and the two percentiles are the
    restatement's, the patch's size from rd_rect_aspect"""
    iw, ih, pw, c = 640, 480, 72, 2
    img = cframe(synth.SEED0, iw, ih, 0)
    with open(tmp_path / "in.ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (iw, ih) + img[..., ::-1].tobytes())
    res = subprocess.run([os.path.join(helpers.ROOT, "examples", "rdgrade"), str(tmp_path / "in.ppm"), "0", str(pw), str(c), "20", "230", "40", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path, timeout=60)
    assert res.returncode == 0, res.stderr.decode()
    ctx = ra.Context(0)
    det = ra.RectDetector(ctx, iw, ih)
    rects = det.execute_once(img, np.tan(72.0 / 2 / 180.0 * np.pi))
    det.close()
    ctx.close()
    n = len(rects)
    text = res.stdout.decode()
    assert n > 0 and ("%d rectangle(s)" % n) in text
    spec = ra.grade_spec(c, 20, 230, 40, 2, True)
    quads = ra.rect_quads(rects)
    for k in range(n):
        ph = min(max(int(np.floor(pw * ra.rect_aspect(rects[k]) + 0.5)), c), 8192)
        want, st = grade.records(img, quads[k:k + 1], pw, ph, spec)
        cells, hist = ra.grade_view(want, spec)
        assert ("rect %d status %d " % (k, rects[k]["status"])) in text and (" patch %d x %d cells %d bytes %d\n" % (pw, ph, c, want.nbytes)) in text
        for cy in range(c):
            for cx in range(c):
                r = cells[0, cy, cx]
                line = "  rect %d cell %d %d : n %d lo %d hi %d ne %d sharpness %s\n" % (k, cx, cy, r["n"], r["lo"], r["hi"], r["ne"], "%.17g" % grade.sharpness(r))
                assert line in text, line
        whole = np.zeros((), ra.GRADE_CELL_DTYPE)
        for f in grade.FIELDS:
            whole[f] = cells[0][f].sum()
        line = "  rect %d whole : n %d lo %d hi %d ne %d sharpness %s p1 %d p99 %d\n" % (k, whole["n"], whole["lo"], whole["hi"], whole["ne"], "%.17g" % grade.sharpness(whole), grade.percentile(hist[0], 1, 100), grade.percentile(hist[0], 99, 100))
        assert line in text, line
        assert int(whole["n"]) == pw * ph
