"""What the GPU tests of the services behind the poll share (test_gpu_rectify.py, test_gpu_annotate.py, test_gpu_composite.py): frames with pitch padding, device
and pinned buffers with a guard behind each, a job that is in flight, and the comparison of planes byte for byte."""
import ctypes
import subprocess
import sys

import numpy as np

import rectdetect_amd as ra
from tests import helpers

L = ra.lib
GUARD = 64      # bytes of 0xA5 behind every buffer: nothing may write there
PAD, FILL = 0x5A, 0xC3      # pitch padding; what a destination holds before its job
MODES = {"inplace": ("device", None), "dev2dev": ("device", "device"), "dev2pinned": ("device", "pinned"), "host2dev": ("host", "device"), "host2pinned": ("host", "pinned"),
         "pinned2dev": ("pinned", "device")}      # (where the source lies, where the destination)


def cframe(seed, iw, ih, t):
    a = np.zeros((ih, iw, 3), np.uint8)
    L().rd_synth_frame(a.ctypes.data, iw, ih, iw * 3, int(seed), int(t), 1)
    return a


def shapes(fmt, iw, ih):
    return ra._source_shapes(fmt, iw, ih)      # [(rows, row bytes)] per plane


def padded(fmt, iw, ih, pad, content):
    """planes of (rows, row bytes + pad): content is a seed (random bytes), a byte value, or a list of (rows, row bytes) arrays; the padding is PAD"""
    rng = np.random.default_rng(content) if isinstance(content, int) and content > 255 else None
    out = []
    for k, (rows, row) in enumerate(shapes(fmt, iw, ih)):
        a = np.full((rows, row + pad), PAD, np.uint8)
        a[:, :row] = rng.integers(0, 256, (rows, row), dtype=np.uint8) if rng is not None else (content if isinstance(content, int) else np.asarray(content[k]).reshape(rows, row))
        out.append(a)
    return out


def into(out_init, want, fmt, iw, ih):
    """what a destination holds after the job: its own padding, the wanted frame's rows (no destination: the wanted frame)"""
    if out_init is None:
        return want
    exp = [o.copy() for o in out_init]
    for e, w, (_, row) in zip(exp, want, shapes(fmt, iw, ih)):
        e[:, :row] = w[:, :row]
    return exp


def assert_planes(got, want, what=""):
    for k, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            ys, xs = np.nonzero(g != w)
            raise AssertionError("%s: plane %d differs in %d bytes, first at row %d byte %d: got %d, expected %d" % (what, k, len(ys), ys[0], xs[0], g[ys[0], xs[0]], w[ys[0], xs[0]]))


class Mem:
    """device and pinned buffers of a test, each with a guard behind it, freed together"""

    def __init__(self):
        self.dev, self.pin = [], []

    def put(self, kind, plane):
        buf = np.concatenate([np.ascontiguousarray(plane).reshape(-1), np.full(GUARD, 0xA5, np.uint8)])
        if kind == "device":
            p = L().rd_device_alloc(buf.nbytes)
            self.dev.append(p)
            L().rd_upload(p, buf.ctypes.data, buf.nbytes)
        else:
            p = L().rd_host_alloc(buf.nbytes)
            self.pin.append(p)
            ctypes.memmove(p, buf.ctypes.data, buf.nbytes)
        return p

    def get(self, kind, p, shape):
        n = int(np.prod(shape))
        a = np.zeros(n + GUARD, np.uint8)
        if kind == "device":
            L().rd_download(a.ctypes.data, p, a.nbytes)
        else:
            ctypes.memmove(a.ctypes.data, p, a.nbytes)
        assert (a[n:] == 0xA5).all(), "bytes behind a buffer were written"
        return a[:n].reshape(shape)

    def place(self, kind, planes, pad=0):
        """planes as a `kind` frame with rows pad bytes longer than they need be: (what a service's enqueue takes as planes, pitches, keyword arguments)"""
        args, pitches = [], []
        for p in planes:
            p = np.ascontiguousarray(p)
            rows, row = p.shape[0], p.size // p.shape[0]
            img = np.full((rows, row + pad), PAD, np.uint8)
            img[:, :row] = p.reshape(rows, row)
            pitches.append(row + pad)
            args.append(img[:, :row] if kind == "host" else self.put(kind, img))
        return args, pitches, {"on_device": kind == "device", "pinned": kind == "pinned"}

    def out(self, kind, nbytes):
        """an output buffer of nbytes (and its guard) filled with 0xA5"""
        return self.put(kind, np.full(nbytes, 0xA5, np.uint8))

    def fetch(self, kind, p, nbytes):
        """the nbytes of an output buffer; its guard must be untouched"""
        return self.get(kind, p, (nbytes,))

    def close(self):
        for p in self.dev:
            L().rd_device_free(p)
        for p in self.pin:
            L().rd_host_free(p)
        self.dev, self.pin = [], []


class Pending:
    """one job on a frame, to be enqueued by the service's test (enqueue: theirs): where its frame will be, and what must not have changed"""

    def __init__(self, mem, fmt, src, iw, ih, mode, out_pad=3):
        self.mem, self.fmt, self.src, self.iw, self.ih = mem, fmt, src, iw, ih
        self.src_kind, self.out_kind = MODES[mode]
        self.rows = [row for _, row in shapes(fmt, iw, ih)]
        self.pitches = [p.shape[1] for p in src]
        if self.src_kind == "host":
            self.args, self.kw = [p[:, :row] for p, row in zip(src, self.rows)], {}
        else:
            self.args = [mem.put(self.src_kind, p) for p in src]
            self.kw = {"on_device": self.src_kind == "device", "pinned": self.src_kind == "pinned"}
        self.out_init = self.out = None
        self.patch_ptr = None      # (a job with patches in device or pinned memory: patch_ptr, patch_kind, patch_src)
        if self.out_kind:
            self.out_init = padded(fmt, iw, ih, out_pad, FILL)
            self.out = [mem.put(self.out_kind, p) for p in self.out_init]
            self.kw.update(out_planes=self.out, out_pitches=[p.shape[1] for p in self.out_init], out_pinned=self.out_kind == "pinned")

    def result(self):
        """the frame's planes, padding included; guards checked; an out-of-place job must have left its source alone, every job its patches"""
        if self.patch_ptr:
            assert np.array_equal(self.mem.get(self.patch_kind, self.patch_ptr, self.patch_src.shape), self.patch_src), "the job changed its patches"
        if self.out_kind:
            if self.src_kind != "host":
                for p, a in zip(self.src, self.args):
                    assert np.array_equal(self.mem.get(self.src_kind, a, p.shape), p), "an out-of-place job changed its source"
            return [self.mem.get(self.out_kind, o, p.shape) for o, p in zip(self.out, self.out_init)]
        return [self.mem.get("device", a, p.shape) for a, p in zip(self.args, self.src)]


def assert_one_job_too_many_is_fatal(make, enqueue, entry):
    """in a child process: `make` creates a service of njobs = 3, `enqueue` gives it one job on the 64 x 64 BGR device frame d; the fourth with nothing waited for
    ends the process with a message that names the entry point"""
    code = ("import numpy as np, rectdetect_amd as ra\n" + make + "\nd = ra.lib().rd_device_alloc(64 * 64 * 3)\nfor k in range(4):\n    " + enqueue + "\n    print('enqueued', k, flush=True)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=helpers.ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "enqueued 2" in r.stdout and "enqueued 3" not in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "3 jobs already in flight" in r.stderr and entry + ":" in r.stderr, r.stderr


def growing_jobs(service, jobs, enqueue, check):
    """the three jobs of a service of njobs = 2 whose second needs larger staging buffers than the first, enqueued while the first is in flight: enqueue(job) for
    the first two, the first waited for, the third enqueued, the others waited for; check(job, what service.wait() returned) for each, in order, at the end"""
    assert service.njobs == 2 and len(jobs) == 3
    waited = []
    for k, job in enumerate(jobs):
        if k == 2:
            waited.append(service.wait())
        assert enqueue(job) == k
    waited += [service.wait(), service.wait()]
    for job, w in zip(jobs, waited):
        check(job, w)
