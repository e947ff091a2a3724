"""Model-ready tensors on the GPU (rd_rectifier_create_tensor): every element equals, in every bit, the numpy restatement of the header's contract (tests/tensor.py) -
for every dtype, layout, channel kind and oversampling, output sizes on every side of the kernel's tile and tail, all six pixel formats, host / device / pinned
frames, device / pinned output, a misaligned output, invalid quads, jobs in flight, empty and full jobs, argument errors, behind the poll of both detector kinds,
into memory that torch allocated, and from the example program.  Every device output lies between guard bytes that must not change.  No tolerance anywhere."""
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers
from tests import match
from tests import pixfmt
from tests import rectify
from tests import rectjobs
from tests import tensor
from tests.rectjobs import L, Out, STATUS, case, cframe, mem, run_job      # (mem: the fixture)

pytestmark = pytest.mark.gpu
# the output sizes at which the kernel can go wrong: one element; the tail path alone; exactly one wave; one pixel into the next wave in both directions, with a
# row tail and rows that start misaligned; several threads of a second wave, rows a multiple of 4
SHAPES = ((1, 1), (5, 3), (32, 8), (33, 9), (36, 12))
NORM = dict(scale=(1 / 58.395 / 1.0, 1 / 57.12, 1 / 57.375), bias=(-2.1179, -2.0357, -1.8044))


@lru_cache(maxsize=None)
def patches_of(fmt, pwm, phm):
    """the restated patches at (pw*m) x (ph*m), computed once and shared (read only)"""
    iw, ih, planes, bgr, quads = case(fmt)
    out = [rectify.patch(bgr, q, pwm, phm) for q in quads]
    for p, _ in out:
        p.setflags(write=False)
    return out


def reference(fmt, pw, ph, spec, sel=None):
    """(the tensors of the case's quads - or of those in sel -, status) from the shared patches"""
    m = int(spec["oversample"])
    pt = patches_of(fmt, pw * m, ph * m)
    sel = range(len(pt)) if sel is None else sel
    out, st = np.zeros(tensor.shape(spec, len(sel), pw, ph), tensor.numpy_dtype(spec)), np.zeros(len(sel), np.uint8)
    for k, q in enumerate(sel):
        patch, st[k] = pt[q]
        if st[k]:
            S = tensor.box_sums(patch, spec, pw, ph)
            for c in range(S.shape[-1]):
                e = tensor.elements(spec, c, S[..., c])
                if int(spec["layout"]) == ra.TENSOR_NCHW:
                    out[k, c] = e
                else:
                    out[k, :, :, c] = e
    return out, st


def test_shared_reference_is_the_restatement():
    spec = ra.tensor_spec(ra.TENSOR_BF16, ra.TENSOR_NCHW, ra.TENSOR_RGB, 2, **NORM)
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    a, b = reference(ra.PIX_BGR, 33, 9, spec), tensor.tensors(bgr, quads, 33, 9, spec)
    tensor.assert_tensors(a[0], a[1], b[0], b[1])
    assert a[1].tolist() == STATUS.tolist()


def check_spec(mem, fmt, pw, ph, spec, kinds=(("device", "device", 0),), offset=0):
    iw, ih, planes, bgr, quads = case(fmt)
    want, wstatus = reference(fmt, pw, ph, spec)
    assert wstatus.tolist() == STATUS.tolist()
    rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=2, tensor=spec)
    try:
        assert rect.patch_bytes == ra.tensor_bytes(spec, pw, ph) == want[0].nbytes and rect.dtype == want.dtype and rect.shape(len(quads)) == want.shape
        for kind, out_kind, pad in kinds:
            got, status = run_job(rect, mem, fmt, planes, iw, ih, quads, kind, out_kind, pad, offset)
            tensor.assert_tensors(got, status, want, wstatus, "%s %s %dx%d %s frame, %s output, pad %d, offset %d" % (ra.PIX_NAMES[fmt], tensor.name(spec), pw, ph, kind, out_kind, pad, offset))
            assert not got[1].view(np.uint8).any(), "an invalid quad gives zero BYTES"
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- every spec, every shape
@pytest.mark.parametrize("dtype", tensor.DTYPES, ids=[tensor.DTYPE_NAMES[d] for d in tensor.DTYPES])
def test_full_cross_of_layout_channels_and_oversampling(dtype, mem):
    for layout in tensor.LAYOUTS:
        for ch in tensor.CHANNELS:
            for m in tensor.OVERSAMPLINGS:
                check_spec(mem, ra.PIX_BGR, 33, 9, ra.tensor_spec(dtype, layout, ch, m, **NORM))
        mem.close()


@pytest.mark.parametrize("pw,ph", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_every_output_size(pw, ph, mem):
    k = 0
    for dtype in tensor.DTYPES:
        for layout in tensor.LAYOUTS:
            for ch in (ra.TENSOR_RGB, ra.TENSOR_GRAY):
                check_spec(mem, ra.PIX_BGR, pw, ph, ra.tensor_spec(dtype, layout, ch, tensor.OVERSAMPLINGS[k % 3], **NORM))
                k += 1
    mem.close()


def test_extreme_scales_reach_the_device_unchanged(mem):
    """a negative scale, a bias of -0.0, overflow of binary16 and of binary32 to infinity: the device's roundings are the restatement's"""
    for dtype in (ra.TENSOR_F16, ra.TENSOR_BF16, ra.TENSOR_F32):
        for scale, bias in (((-1.0, 1.0, -0.0171), (-0.0, -0.0, 2.0)), ((1000.0, 3.0e38, -3.0e38), (0.0, 1.0, 0.0)), ((1.0, 1.0, 1.0e-7), (2048.0, 256.0, 0.0))):
            check_spec(mem, ra.PIX_BGR, 33, 9, ra.tensor_spec(dtype, ra.TENSOR_NCHW, ra.TENSOR_BGR, 2, scale, bias))
            check_spec(mem, ra.PIX_BGR, 36, 12, ra.tensor_spec(dtype, ra.TENSOR_NHWC, ra.TENSOR_RGB, 1, scale, bias))


# ---------------------------------------------------------------------------------------------- formats, frame kinds, output kinds
SPEC_PER_DTYPE = (ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NCHW, ra.TENSOR_RGB, 2), ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, 1, **NORM),
                  ra.tensor_spec(ra.TENSOR_BF16, ra.TENSOR_NHWC, ra.TENSOR_BGR, 4, **NORM), ra.tensor_spec(ra.TENSOR_F32, ra.TENSOR_NHWC, ra.TENSOR_GRAY, 2, **NORM))


@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_every_format_frame_kind_and_output_kind(fmt, mem):
    kinds = [(kind, out_kind, 13 if kind == "device" else 0) for kind in ("host", "device", "pinned") for out_kind in ("device", "pinned")]
    for spec in SPEC_PER_DTYPE:
        check_spec(mem, fmt, 33, 9, spec, kinds)
        mem.close()


def test_out_offset_by_one_element_takes_the_misaligned_store_path(mem):
    for pw, ph in ((36, 12), (33, 9)):
        for m in (1, 2):
            check_spec(mem, ra.PIX_BGR, pw, ph, ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, m, **NORM), offset=2)
    check_spec(mem, ra.PIX_BGR, 36, 12, ra.tensor_spec(ra.TENSOR_BF16, ra.TENSOR_NHWC, ra.TENSOR_RGB, 1, **NORM), offset=2)
    check_spec(mem, ra.PIX_BGR, 36, 12, ra.tensor_spec(ra.TENSOR_F32, ra.TENSOR_NHWC, ra.TENSOR_BGR, 1, **NORM), offset=4)
    check_spec(mem, ra.PIX_BGR, 36, 12, ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NCHW, ra.TENSOR_BGR, 1), offset=1)


# ---------------------------------------------------------------------------------------------- where the contract says two things coincide: GPU against GPU
def test_u8_nhwc_bgr_m1_equals_the_classic_rectifier_on_the_device(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_NV12)
    for pw, ph in SHAPES:
        classic = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=1)
        as_tensor = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=1, tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_BGR, 1))
        try:
            assert classic.patch_bytes == as_tensor.patch_bytes == pw * ph * 3 and classic.shape(2) == as_tensor.shape(2) == (2, ph, pw, 3) and classic.dtype == np.uint8
            a, sa = run_job(classic, mem, ra.PIX_NV12, planes, iw, ih, quads)
            b, sb = run_job(as_tensor, mem, ra.PIX_NV12, planes, iw, ih, quads)
            tensor.assert_tensors(b, sb, a, sa, "%dx%d" % (pw, ph))
            assert a[0].any()
        finally:
            classic.close()
            as_tensor.close()


@pytest.mark.parametrize("m", tensor.OVERSAMPLINGS)
def test_u8_nchw_gray_equals_the_matchers_signature_plus_128(m, mem):
    G = 8
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    matcher = ra.Matcher(G, m, max_templates=1, max_quads=1, njobs=1)
    rect = ra.Rectifier(G, G, max_quads=1, njobs=1, tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NCHW, ra.TENSOR_GRAY, m))
    try:
        t = matcher.add_image(bgr)
        sig = matcher.signature(t, 0)[0]
        got, status = run_job(rect, mem, ra.PIX_BGR, planes, iw, ih, match.whole(iw, ih)[None])
        assert status.tolist() == [1] and got.shape == (1, 1, G, G)
        assert np.array_equal(got[0, 0].astype(np.int64), sig.astype(np.int64) + 128)
    finally:
        matcher.close()
        rect.close()


# ---------------------------------------------------------------------------------------------- jobs in flight, empty and full jobs, argument errors
def test_jobs_in_flight_come_back_in_order_with_different_n(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph, njobs = 33, 9, 3
    spec = ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, 2, **NORM)
    rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=njobs, tensor=spec)
    args, pitches, kw = mem.place("device", planes, 5)
    subsets = [list(range(len(quads)))[k % 3:k % 3 + 1 + k % 4] for k in range(8)]      # every job another selection of the quads
    pending, checked = [], 0

    def take():
        sel, out = pending.pop(0)
        status = rect.wait()
        want, wstatus = reference(ra.PIX_BGR, pw, ph, spec, sel)
        tensor.assert_tensors(out.fetch().view(rect.dtype).reshape(rect.shape(len(sel))), status, want, wstatus, "job %d" % checked)

    try:
        for k, sel in enumerate(subsets):
            if len(pending) == njobs:
                take()
                checked += 1
            out = Out(mem, "device" if k % 2 == 0 else "pinned", len(sel) * rect.patch_bytes)
            assert rect.enqueue(ra.PIX_BGR, args, pitches, iw, ih, quads[sel], out.ptr, out_pinned=k % 2 == 1, **kw) == k
            pending.append((sel, out))
        while pending:
            take()
            checked += 1
        assert checked == len(subsets) and len({len(s) for s in subsets}) > 2
        with pytest.raises(RuntimeError):
            rect.wait()      # nothing in flight
    finally:
        rect.close()


def test_empty_job_and_full_job(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_RGBA)
    pw, ph = 5, 3
    spec = ra.tensor_spec(ra.TENSOR_BF16, ra.TENSOR_NHWC, ra.TENSOR_RGB, 4, **NORM)
    want, wstatus = reference(ra.PIX_RGBA, pw, ph, spec)
    nmax = 2 * len(quads)
    rect = ra.Rectifier(pw, ph, max_quads=nmax, njobs=2, tensor=spec)
    try:
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.zeros((0, 4, 2)))      # n = 0: nothing written, nothing returned
        assert got.shape == (0, ph, pw, 3) and len(status) == 0
        assert rect.enqueue(ra.PIX_RGBA, planes, None, iw, ih, np.zeros((0, 8)), None) == 1      # (no output buffer needed either)
        assert len(rect.wait()) == 0
        full = np.concatenate([quads, quads[::-1]])
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, full, "host", "pinned")      # n = max_quads
        tensor.assert_tensors(got, status, np.concatenate([want, want[::-1]]), np.concatenate([wstatus, wstatus[::-1]]), "full job")
        with pytest.raises(ValueError):
            run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.concatenate([full, quads[:1]]))      # one more
        conv = rect.rectify(bgr, quads)      # the convenience call
        tensor.assert_tensors(conv, wstatus, want, wstatus, "rectify()")
    finally:
        rect.close()


def test_argument_errors_return_minus_one_and_the_next_job_is_correct(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = 33, 9
    spec = ra.tensor_spec(ra.TENSOR_F32, ra.TENSOR_NCHW, ra.TENSOR_BGR, 2, **NORM)
    want, wstatus = reference(ra.PIX_BGR, pw, ph, spec)
    create = lambda *a: L().rd_rectifier_create_tensor(*a)
    sp = spec.copy()
    assert not create(0, pw, ph, 4, 1, None)      # a NULL spec
    for field, v in (("dtype", 4), ("layout", 2), ("channels", 3), ("oversample", 3), ("scale", np.nan), ("bias", np.inf)):
        bad = spec.copy()
        bad[field] = v
        assert not create(0, pw, ph, 4, 1, bad.ctypes.data), field
        with pytest.raises(ValueError):
            ra.Rectifier(pw, ph, tensor=bad)
    for args in ((0, 0, ph, 4, 1), (0, pw, 0, 4, 1), (0, 8193, ph, 4, 1), (0, pw, ph, 0, 1), (0, pw, ph, 4, 0), (99, pw, ph, 4, 1)):
        assert not create(*args, sp.ctypes.data), args      # rd_rectifier_create's bad arguments (pw * m > 16384 among them)
    assert L().rd_rectifier_patch_bytes(None) == 0
    rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=1, tensor=spec)
    out = Out(mem, "device", len(quads) * rect.patch_bytes)
    try:
        q = rectjobs.refused_enqueues(mem, rect, planes, iw, ih, quads, out)      # and the first job after all of them: the right elements
        status = rect.wait()
        tensor.assert_tensors(out.fetch().view(rect.dtype).reshape(rect.shape(len(q))), status, want, wstatus, "the job after the refused ones")
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- behind the detector's poll
POLL_SPEC = ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, 2, **NORM)


@pytest.mark.parametrize("kind", ["rect-host", "rect-device", "poly-host", "poly-device", "scaled"])
def test_rectify_polled_behind_every_poll(kind, mem):
    """after Detector.poll and PolylineDetector.poll, on host frames (the detector's own copy) and device frames, and on a frame that came in at scale 2 - quads in
    detector coordinates, the tensor from the full-size source (X = 2x + 0.5)"""
    rectjobs.polled_behind_a_poll(mem, kind, dict(tensor=POLL_SPEC), lambda bgr, quads: tensor.tensors(bgr, quads, rectjobs.PW, rectjobs.PH, POLL_SPEC),
                                  lambda got, status, _, want, wstatus, what: tensor.assert_tensors(got, status, want, wstatus, what), max_quads=64, nrects=6, nframes=4)


# ---------------------------------------------------------------------------------------------- memory that torch allocated
TORCH_CHILD = """
import sys
import torch                      # first: the process then holds ONE HIP runtime, torch's (INTEGRATION.md, section 3)
import numpy as np
import rectdetect_amd as ra
d = np.load(sys.argv[1])
frame, quads, pw, ph = d["frame"], d["quads"], int(d["pw"]), int(d["ph"])
ih, iw, n = frame.shape[0], frame.shape[1], len(quads)
norm = dict(scale=d["scale"], bias=d["bias"])
dframe = ra.lib().rd_device_alloc(frame.nbytes)
ra.lib().rd_upload(dframe, frame.ctypes.data, frame.nbytes)
for name, spec, t in (("f16_nchw", ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, 2, **norm), torch.empty((n, 3, ph, pw), dtype=torch.float16, device="cuda")),
                      ("bf16_nhwc", ra.tensor_spec(ra.TENSOR_BF16, ra.TENSOR_NHWC, ra.TENSOR_RGB, 1, **norm), torch.empty((n, ph, pw, 3), dtype=torch.bfloat16, device="cuda"))):
    rect = ra.Rectifier(pw, ph, max_quads=n, njobs=1, tensor=spec)
    assert rect.shape(n) == tuple(t.shape) and rect.patch_bytes * n == t.numel() * t.element_size()
    t.fill_(7.0)
    torch.cuda.synchronize()      # the caller's own streams are done with the memory before the enqueue
    rect.enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, t.data_ptr(), on_device=True)
    status = rect.wait()          # after which the data is visible to every stream
    np.save(sys.argv[2] + name + ".npy", t.cpu().view(torch.int16).numpy())
    np.save(sys.argv[2] + name + "_status.npy", status)
    print(name, "sum", float(t.float().sum().item()), flush=True)      # a torch op on the tensor afterwards
    rect.close()
ra.lib().rd_device_free(dframe)
print("done", flush=True)
"""


def test_torch_tensors_are_written_through_data_ptr(tmp_path):
    """a torch.float16 NCHW and a torch.bfloat16 NHWC tensor, allocated by torch on the device and written through data_ptr(), read back with t.cpu(): the
    restatement's bits.  In a child process, because what is tested is a process that imports torch first and so holds one HIP runtime."""
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = 33, 9
    specs = {"f16_nchw": ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, 2, **NORM), "bf16_nhwc": ra.tensor_spec(ra.TENSOR_BF16, ra.TENSOR_NHWC, ra.TENSOR_RGB, 1, **NORM)}
    child = rectjobs.torch_child(tmp_path, TORCH_CHILD, specs, frame=bgr, quads=quads, pw=pw, ph=ph, scale=np.array(NORM["scale"], np.float32), bias=np.array(NORM["bias"], np.float32))
    for name, spec in specs.items():
        want, wstatus = reference(ra.PIX_BGR, pw, ph, spec)
        got, status, total = child[name]
        tensor.assert_tensors(got.view(np.uint16), status, np.ascontiguousarray(want).view(np.uint16), wstatus, name)
        assert np.isfinite(float(total)), "the tensors hold finite values and torch summed them"


# ---------------------------------------------------------------------------------------------- the example program
def test_rdtensors_writes_the_bytes_the_binding_gives(tmp_path):
    """examples/rdtensors on a PPM with a spec on its command line: the raw tensor file is what Rectifier.rectify makes of the same image and rectangles"""
    iw, ih, pw, ph = 640, 480, 36, 20
    img = cframe(synth.SEED0, iw, ih, 0)
    with open(tmp_path / "in.ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (iw, ih) + img[..., ::-1].tobytes())
    raw = tmp_path / "t.raw"
    res = subprocess.run([os.path.join(helpers.ROOT, "examples", "rdtensors"), str(tmp_path / "in.ppm"), "0", str(raw), str(pw), str(ph), "f16", "nchw", "rgb", "2", "0.017", "-2.0"],
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
    spec = ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, 2, 0.017, -2.0)
    rect = ra.Rectifier(pw, ph, max_quads=n, njobs=1, tensor=spec)
    try:
        want = rect.rectify(img, ra.rect_quads(rects))
    finally:
        rect.close()
    ref, _ = tensor.tensors(img, ra.rect_quads(rects), pw, ph, spec)
    assert want.tobytes() == ref.tobytes()
    assert ("shape %d x 3 x %d x %d dtype f16 bytes %d" % (n, ph, pw, want.nbytes)) in text
    assert open(raw, "rb").read() == want.tobytes()
