"""What the GPU tests of the rectifier's output kinds share (test_gpu_tensor.py, test_gpu_scan.py, test_gpu_grade.py, test_gpu_code.py, test_gpu_blobs.py): the noise
frames and quads of a job with their restated G planes, an output between guard bytes, one job waited for, the job behind every kind of poll, the raw enqueue with
one argument wrong at a time, and the child process that imports torch first.  What a kind's bytes must be stays in the kind's own file."""
import ctypes
import os
import re
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers
from tests import jobframes
from tests import pixfmt
from tests import rectify
from tests import tensor
from tests.jobframes import L, cframe

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
GUARD = 64


@pytest.fixture
def mem():
    m = jobframes.Mem()
    yield m
    m.close()


def noise_frame(iw, ih, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (ih, iw, 3), dtype=np.uint8)


def job_quads(iw, ih):
    """an axis-aligned quad, a non-convex (invalid) one BETWEEN valid ones, a rotated quad in perspective, a quad that reaches outside the frame on two sides"""
    w, h = float(iw), float(ih)
    return np.array([
        [(10.5, 8.5), (74.5, 8.5), (74.5, 40.5), (10.5, 40.5)],
        [(0.0, 0.0), (60.0, 0.0), (20.0, 20.0), (0.0, 50.0)],
        [(30.25, 6.5), (88.75, 14.0), (80.0, 55.5), (12.5, 41.0)],
        [(w - 40.0, h - 30.0), (w + 12.5, h - 36.0), (w + 7.0, h + 9.0), (w - 48.0, h + 4.25)],
    ], np.float64)


STATUS = np.array([1, 0, 1, 1], np.uint8)


@lru_cache(maxsize=None)
def case(fmt, seed=0):
    """(iw, ih, planes, the contract's BGR frame, quads): 97 x 61 for the packed formats, 96 x 60 for 4:2:0"""
    iw, ih = (97, 61) if fmt <= ra.PIX_RGBA else (96, 60)
    planes, bgr = pixfmt.convert(noise_frame(iw, ih, 21 + fmt + 100 * seed), fmt)
    assert np.array_equal(rectify.contract_bgr(fmt, planes), bgr)
    return iw, ih, planes, bgr, job_quads(iw, ih)


@lru_cache(maxsize=None)
def gray_planes(fmt, pw, ph, m, seed=0):
    """step 1 of the kinds with a G plane restated, computed once and shared (read only): ((n, ph, pw) uint8 G planes of the case's quads, status)"""
    iw, ih, planes, bgr, quads = case(fmt, seed)
    g, st = tensor.tensors(bgr, quads, pw, ph, ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, m))
    g = g.reshape(len(quads), ph, pw)
    g.setflags(write=False)
    st.setflags(write=False)
    return g, st


class Out:
    """an output of nbytes in device memory between guards (0xA5, like the output itself before its job), `offset` bytes off its aligned start; or in pinned memory"""

    def __init__(self, mem, kind, nbytes, offset=0):
        self.mem, self.kind, self.nbytes, self.offset = mem, kind, nbytes, offset
        if kind == "device":
            self.total = GUARD + offset + nbytes + GUARD
            self.base = L().rd_device_alloc(self.total)
            mem.dev.append(self.base)
            fill = np.full(self.total, 0xA5, np.uint8)
            L().rd_upload(self.base, fill.ctypes.data, self.total)
            self.ptr = self.base + GUARD + offset
        else:
            assert offset == 0
            self.ptr = mem.out("pinned", nbytes)

    def fetch(self, nbytes=None):
        """the first nbytes the job wrote (default: all); everything around them must be 0xA5 still.  A buffer that several jobs wrote: fetch()[:n], for what lies
        behind a shorter job's bytes is what a longer one left"""
        nbytes = self.nbytes if nbytes is None else nbytes
        if self.kind != "device":
            a = self.mem.fetch("pinned", self.ptr, self.nbytes)
            assert (a[nbytes:] == 0xA5).all(), "bytes behind the job's last byte were written"
            return a[:nbytes]
        a = np.zeros(self.total, np.uint8)
        L().rd_download(a.ctypes.data, self.base, self.total)
        lo = GUARD + self.offset
        assert (a[:lo] == 0xA5).all(), "bytes before `out` were written"
        assert (a[lo + nbytes:] == 0xA5).all(), "bytes behind the job's last byte were written"
        return a[lo:lo + nbytes].copy()


def run_job(rect, mem, fmt, planes, iw, ih, quads, kind="device", out_kind="device", pad=0, offset=0, out=None):
    """one job, waited for: (the array of rect.shape(n) and rect.dtype, status).  Into a new output of exactly its size, `offset` bytes off its aligned start, or into `out`"""
    q = np.asarray(quads, np.float64).reshape(-1, 8)
    nbytes = len(q) * rect.patch_bytes
    args, pitches, kw = mem.place(kind, planes, pad)
    reused = out is not None      # (then the bytes behind the job's are what earlier jobs left there: the caller looks at them)
    out = out if reused else Out(mem, out_kind, nbytes, offset)
    rect.enqueue(fmt, args, pitches, iw, ih, q, out.ptr, out_pinned=out_kind == "pinned", **kw)
    status = rect.wait()
    return out.fetch(None if reused else nbytes)[:nbytes].view(rect.dtype).reshape(rect.shape(len(q))), status


def gray_job(mem, fmt, planes, iw, ih, quads, pw, ph, m):
    """the (n, ph, pw) G planes the GPU's tensor kernel makes of a job, and its status"""
    trect = ra.Rectifier(pw, ph, max_quads=max(len(quads), 1), njobs=1, tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, m))
    try:
        plane, pstatus = run_job(trect, mem, fmt, planes, iw, ih, quads)
    finally:
        trect.close()
    return plane.reshape(len(quads), ph, pw), pstatus


# ---------------------------------------------------------------------------------------------- argument errors
def refused_enqueues(mem, rect, planes, iw, ih, quads, out, more=()):
    """rd_rectifier_enqueue itself on the BGR frame `planes` with one argument wrong at a time - the rows every kind shares and the file's own (`more`: name ->
    the arguments of call() that differ): each returns -1 and enqueues nothing.  Then the same call with nothing wrong: job 0, left in flight.  Returns the quads as
    enqueued"""
    (dframe,), (pitch,), _ = mem.place("device", planes, 3)
    pageable = np.zeros(len(quads) * rect.patch_bytes, np.uint8)
    q = np.ascontiguousarray(quads).reshape(-1, 8)
    P, I = ctypes.c_void_p * 3, ctypes.c_int * 3

    def call(fmt=ra.PIX_BGR, pl=(dframe, None, None), pi=(pitch, 0, 0), w=iw, h=ih, kind=1, quads_p=q.ctypes.data, n=len(q), out_p=out.ptr, out_kind=1):
        return L().rd_rectifier_enqueue(rect.h, fmt, P(*pl), I(*pi), w, h, kind, quads_p, n, out_p, out_kind)

    errors = {"unknown format": dict(fmt=6), "NULL plane": dict(pl=(None, None, None)), "short pitch": dict(pi=(iw * 3 - 1, 0, 0)), "odd width with 4:2:0": dict(fmt=ra.PIX_NV12, pl=(dframe, dframe, None), pi=(pitch, pitch, 0)),
              "n < 0": dict(n=-1), "n > max_quads": dict(n=len(q) + 1), "pageable out": dict(out_p=pageable.ctypes.data, out_kind=2), "pageable out as device memory": dict(out_p=pageable.ctypes.data),
              "unknown out_kind": dict(out_kind=0), "unknown on_device": dict(kind=3), "no size": dict(w=0), "NULL quads": dict(quads_p=None), "NULL out": dict(out_p=None)}
    errors.update(more)
    for name, kw in errors.items():
        assert call(**kw) == -1, name
        assert L().rd_rectifier_wait(rect.h, None) == -1, name + ": nothing may have been enqueued"
    assert call() == 0      # the first job after all of them: sequence number 0
    return q


# ---------------------------------------------------------------------------------------------- behind the detector's poll
PW, PH = 100, 60
SIW, SIH = 640, 480
FIXED_QUAD = np.array([[(101.5, 80.25), (420.0, 60.0), (500.5, 400.0), (60.0, 330.5)]])


@lru_cache(maxsize=None)
def stream_frames(fmt, n=3):
    return tuple(pixfmt.convert(cframe(synth.SEED0, SIW, SIH, t), fmt) for t in range(n))


def polled_behind_a_poll(mem, kind, make, restate, compare, beside=None, max_quads=8, nrects=3, nframes=3, misaligned_refused=False, out_reused=False):
    """A PW x PH rectifier made with the keywords `make` behind one kind of poll: "rect-host" / "rect-device" / "poly-host" / "poly-device" after Detector.poll and
    PolylineDetector.poll on host frames (the detector's own copy) and device frames, "scaled" on a frame that came in at scale 2 - quads in detector coordinates,
    the output from the full-size source (X = 2x + 0.5).  Every one of nframes frames: its first nrects rectangles and FIXED_QUAD through rectify_polled on the
    rectifier and on the one made with `beside` (the rectifier whose output is the kind's intermediate, or None), then compare(got, status, what the one beside
    gave as (n, PH, its row), restate(bgr, quads), what).  misaligned_refused: `out` + 4 must raise ValueError.  out_reused: later jobs may be shorter than
    earlier ones, and what lies behind their bytes is not looked at (otherwise it must be 0xA5 still)"""
    poly, scaled, device = kind.startswith("poly"), kind == "scaled", kind.endswith("device")
    fmt = ra.PIX_NV12 if device else ra.PIX_BGR
    scale = 2 if scaled else 1
    dw, dh = SIW // scale, SIH // scale
    det = ra.PolylineDetector(dw, dh, nslots=2) if poly else ra.Detector(dw, dh, nslots=2, aperture=TAN36)
    rects = [ra.Rectifier(PW, PH, max_quads=max_quads, njobs=2, **kw) for kw in (make, beside) if kw is not None]
    rect = rects[0]
    total = 0
    try:
        outs = [Out(mem, "device", max_quads * r.patch_bytes) for r in rects]
        with pytest.raises(ValueError):      # nothing polled yet
            det.rectify_polled(rect, FIXED_QUAD, outs[0].ptr)
        for t, (planes, bgr) in enumerate(stream_frames(fmt, nframes)):
            if scaled:
                det.enqueue_scaled(fmt, planes)
            elif device:
                args, pitches, kw = mem.place("device", planes, 8)
                det.enqueue_planes(fmt, args, pitches, **kw)
            else:
                det.enqueue_planes(fmt, planes)
            res = det.poll()[0] if poly else det.poll(TAN36)
            quads = FIXED_QUAD / scale if poly or len(res) == 0 else np.concatenate([ra.rect_quads(res)[:nrects], FIXED_QUAD / scale])
            if misaligned_refused:
                with pytest.raises(ValueError):
                    det.rectify_polled(rect, quads, outs[0].ptr + 4)      # refused here as well
            for r, o in zip(rects, outs):
                assert det.rectify_polled(r, quads, o.ptr) == t
            statuses = [r.wait() for r in rects]
            n = len(quads)
            got = [(o.fetch()[:n * r.patch_bytes] if out_reused else o.fetch(n * r.patch_bytes)).view(r.dtype).reshape(r.shape(n)) for r, o in zip(rects, outs)]
            want, wstatus = restate(bgr, quads * 2.0 + 0.5 if scaled else quads)
            if beside is not None:
                assert statuses[1].tolist() == wstatus.tolist()
            compare(got[0], statuses[0], got[1].reshape(got[1].shape[:3]) if beside is not None else None, want, wstatus, "%s frame %d" % (kind, t))
            total += n
        assert total > nframes or not kind.startswith("rect"), "the stream's frames hold rectangles"
    finally:
        for r in rects:
            r.close()
        det.close()


# ---------------------------------------------------------------------------------------------- memory that torch allocated
def torch_child(tmp_path, script, names, **inputs):
    """`script` in a child process - because what is tested is a process that imports torch first and so holds one HIP runtime - with `inputs` as an .npz file in
    argv[1] and a prefix for its outputs in argv[2].  For every name it saves <name>.npy and <name>_status.npy and prints "<name> sum <number>", and "done" at its
    end: {name: (the array, the status, the number's text)}"""
    pytest.importorskip("torch")
    np.savez(tmp_path / "in.npz", **inputs)
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path / "in.npz"), str(tmp_path) + os.sep], cwd=helpers.ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return {name: (np.load(tmp_path / (name + ".npy")), np.load(tmp_path / (name + "_status.npy")), re.search(name + r" sum (\S+)", r.stdout).group(1)) for name in names}
