#!/usr/bin/env python3
"""Generate tests/golden/polystream_*.npz from THE REFERENCE ITSELF (oracle/_ref/librdref.so: its kernels and host C on the serial OpenCL
shim).  Only runs where the reference build exists; the fixtures are data: inputs are re-created from seeds by rectdetect_amd/synth.py.

Per stream and frame: all records 0..n of the segment list exactly as poly.cpp's sequence leaves it (rdref_poly_run: fresh buffers per
frame), the CRC32 of the per-pixel id plane, and the parameters.

It also answers one question about vidpoly.cpp, which keeps its buffers across frames: the plane whose 2-px frame ring the polyline
stage's bridging step reads but never writes is the caller's tmp3 - mem6 in vidpoly (oclpolyline.c:297) - so a stream could carry ring
values from one frame into the next.  vidpoly.cpp:160-190 is restated here with persistent buffers by calling the reference's compiled
functions through ctypes, and its lists are compared with the per-frame lists on every frame.  Where they differ, the persistent-buffer
lists are stored as well (vid_*); the detector's contract stays the per-frame one.

    python tools/make_golden_polystreams.py [name ...]      (default: every stream)
"""
import ctypes
import json
import multiprocessing
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers

VID = (2000, 1.0, 10)      # vidpoly.cpp:180, 183
POLY = (500, 1.0, 20)      # poly.cpp:120, 123
HARD = ("tiles", "bars", "waves", "noise")
# name -> (iw, ih, list of (kind, seed, t) frames, parameters)
STREAMS = {
    "polystream_1920x1080_s0_vid": (1920, 1080, [("frame", synth.SEED0, t) for t in range(64)], VID),
    "polystream_1280x720_s1": (1280, 720, [("frame", synth.SEED0 + 1, t) for t in range(64)], POLY),
    "polystream_3840x2160_s4_vid": (3840, 2160, [("frame", synth.SEED0 + 4, t) for t in range(8)], VID),
    "polystream_1920x1080_hard_vid": (1920, 1080, [(k, 31, 0) for k in HARD], VID),
    "polystream_1920x1080_hard": (1920, 1080, [(k, 31, 0) for k in HARD], POLY),
}


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def make_frame(kind, seed, t, iw, ih):
    return synth.frame(seed, iw, ih, t) if kind == "frame" else synth.hard_frame(kind, seed, iw, ih)


class VidPoly:
    """vidpoly.cpp:109-190 on the reference's compiled code: buffers created once, kept for the whole stream."""

    def __init__(self, R, iw, ih, params):
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        for name, res, args in [("simpleGetDevice", vp, [ci]), ("simpleCreateContext", vp, [vp]), ("clCreateCommandQueue", vp, [vp, vp, ctypes.c_ulong, vp]),
                                ("clCreateBuffer", vp, [vp, ctypes.c_ulong, ctypes.c_size_t, vp, vp]), ("clFinish", ci, [vp]),
                                ("clEnqueueWriteBuffer", ci, [vp, vp, ctypes.c_uint, ctypes.c_size_t, ctypes.c_size_t, vp, ctypes.c_uint, vp, vp]),
                                ("clEnqueueReadBuffer", ci, [vp, vp, ctypes.c_uint, ctypes.c_size_t, ctypes.c_size_t, vp, ctypes.c_uint, vp, vp]),
                                ("clReleaseMemObject", ci, [vp]), ("init_oclimgutil", vp, [vp, vp]), ("init_oclpolyline", vp, [vp, vp]),
                                ("dispose_oclimgutil", None, [vp]), ("dispose_oclpolyline", None, [vp])]:
            fn = getattr(R, name)
            fn.restype, fn.argtypes = res, args
        sig = {"oclimgutil_convert_plab_bgr": [vp, vp, vp, ci, ci, ci, vp, vp], "oclimgutil_unpack_f_f_f_plab": [vp, vp, vp, vp, vp, ci, ci, vp, vp],
               "oclimgutil_iirblur_f_f": [vp, vp, vp, vp, vp, ci, ci, ci, vp, vp], "oclimgutil_pack_plab_f_f_f": [vp, vp, vp, vp, vp, ci, ci, vp, vp],
               "oclimgutil_edgevec_f2_f": [vp, vp, vp, ci, ci, vp, vp], "oclimgutil_edge_f_plab": [vp, vp, vp, ci, ci, vp, vp],
               "oclimgutil_thinthres_f_f_f2": [vp, vp, vp, vp, ci, ci, vp, vp], "oclimgutil_threshold_f_f": [vp, vp, vp, cf, cf, cf, ci, vp, vp],
               "oclimgutil_cast_i_f": [vp, vp, vp, cf, ci, vp, vp], "oclimgutil_label8x_int_int": [vp, vp, vp, vp, ci, ci, ci, vp, vp],
               "oclimgutil_clear": [vp, vp, ci, vp, vp], "oclimgutil_calcStrength": [vp, vp, vp, vp, ci, ci, vp, vp],
               "oclimgutil_filterStrength": [vp, vp, vp, ci, ci, ci, vp, vp], "oclimgutil_threshold_i_i": [vp, vp, vp, ci, ci, ci, ci, vp, vp],
               "oclpolyline_execute": [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, cf, ci, ci, ci, vp, vp]}
        for name, args in sig.items():
            fn = getattr(R, name)
            fn.restype, fn.argtypes = vp, args
        R.rdref_init()
        self.R, self.iw, self.ih, self.params = R, iw, ih, params
        self.device = R.simpleGetDevice(0)
        self.context = R.simpleCreateContext(self.device)
        self.queue = R.clCreateCommandQueue(self.context, self.device, 0, None)
        self.iu = R.init_oclimgutil(self.device, self.context)
        self.pl = R.init_oclpolyline(self.device, self.context)
        N = iw * ih
        zero = np.zeros(N * 4, np.int32)
        # (vidpoly.cpp:127-152: every buffer zero-filled once, CL_MEM_READ_WRITE | CL_MEM_COPY_HOST_PTR)
        self.mem = [R.clCreateBuffer(self.context, ra.CL_MEM_READ_WRITE | ra.CL_MEM_COPY_HOST_PTR, N * 4, zero.ctypes.data, None) for _ in range(10)]
        self.big = R.clCreateBuffer(self.context, ra.CL_MEM_READ_WRITE | ra.CL_MEM_COPY_HOST_PTR, N * 16, zero.ctypes.data, None)
        self.ls = R.clCreateBuffer(self.context, ra.CL_MEM_READ_WRITE | ra.CL_MEM_COPY_HOST_PTR, N * 16, zero.ctypes.data, None)
        self.buf0 = np.zeros(N, np.int32)

    def frame(self, bgr):
        R, iw, ih, q = self.R, self.iw, self.ih, self.queue
        m, N = self.mem, self.iw * self.ih
        sthr, minerr, sizethr = self.params
        ws = bgr.strides[0]
        self.buf0.view(np.uint8)[: ws * ih] = np.ascontiguousarray(bgr).reshape(-1)[: ws * ih]      # vidpoly.cpp:163: memcpy(buf0, data, ws * ih)
        R.clEnqueueWriteBuffer(q, m[0], 0, 0, N * 4, self.buf0.ctypes.data, 0, None, None)
        R.oclimgutil_convert_plab_bgr(self.iu, m[4], m[0], iw, ih, ws, q, None)
        R.oclimgutil_unpack_f_f_f_plab(self.iu, m[1], m[2], m[3], m[4], iw, ih, q, None)
        R.oclimgutil_iirblur_f_f(self.iu, m[0], m[1], m[4], m[5], 2, iw, ih, q, None)
        R.oclimgutil_iirblur_f_f(self.iu, m[1], m[2], m[4], m[5], 2, iw, ih, q, None)
        R.oclimgutil_iirblur_f_f(self.iu, m[2], m[3], m[4], m[5], 2, iw, ih, q, None)
        R.oclimgutil_pack_plab_f_f_f(self.iu, m[4], m[0], m[1], m[2], iw, ih, q, None)
        R.oclimgutil_edgevec_f2_f(self.iu, self.big, m[0], iw, ih, q, None)
        R.oclimgutil_edge_f_plab(self.iu, m[5], m[4], iw, ih, q, None)
        R.oclimgutil_thinthres_f_f_f2(self.iu, m[2], m[5], self.big, iw, ih, q, None)
        R.oclimgutil_threshold_f_f(self.iu, m[9], m[2], 0.0, 0.0, 1.0, N, q, None)
        R.oclimgutil_cast_i_f(self.iu, m[8], m[9], 1.0, N, q, None)
        R.oclimgutil_label8x_int_int(self.iu, m[3], m[8], m[9], 0, iw, ih, q, None)
        R.oclimgutil_clear(self.iu, m[4], N * 4, q, None)
        R.oclimgutil_calcStrength(self.iu, m[4], m[2], m[3], iw, ih, q, None)
        R.oclimgutil_filterStrength(self.iu, m[3], m[4], sthr, iw, ih, q, None)
        R.oclimgutil_threshold_i_i(self.iu, m[3], m[3], 0, 0, 1, N, q, None)
        R.oclpolyline_execute(self.pl, self.ls, N * 16, m[0], m[3], self.big, m[4], m[5], m[6], m[7], m[8], m[9], minerr, sizethr, iw, ih, q, None)
        ids = np.zeros(N, np.int32)
        R.clEnqueueReadBuffer(q, m[0], 1, 0, N * 4, ids.ctypes.data, 0, None, None)
        R.clEnqueueReadBuffer(q, m[0], 1, 0, N * 4, self.buf0.ctypes.data, 0, None, None)      # (vidpoly.cpp:188: buf0 <- mem0; the next frame overwrites ws * ih bytes of it)
        ls = np.zeros(N * 4, np.int32)
        R.clEnqueueReadBuffer(q, self.ls, 1, 0, N * 16, ls.ctypes.data, 0, None, None)
        R.clFinish(q)
        n = int(ls[0])
        return ls[: 14 * (n + 1)].view(ra.LS_DTYPE).copy(), ids

    def close(self):
        for b in self.mem + [self.big, self.ls]:
            self.R.clReleaseMemObject(b)
        self.R.dispose_oclpolyline(self.pl)
        self.R.dispose_oclimgutil(self.iu)


def per_frame(args):
    """poly.cpp's sequence on one frame (rdref_poly_run: fresh buffers).  In a worker process that is replaced every few frames: every call initialises
    oclimgutil / oclpolyline anew, and the reference never hands a kernel id back (oclhelper.c: KERNELIDMAX)."""
    name, i = args
    iw, ih, frames, (sthr, minerr, sizethr) = STREAMS[name]
    kind, seed, t = frames[i]
    img = make_frame(kind, seed, t, iw, ih)
    N = iw * ih
    ls = np.zeros(N * 4, np.int32)
    ids = np.zeros(N, np.int32)
    n = helpers.ref().rdref_poly_run(img.ctypes.data, iw, ih, img.strides[0], sthr, minerr, sizethr, helpers.P(ls), helpers.P(ids), None)
    return ls[: 14 * (n + 1)].tobytes(), ids.tobytes()


def main(names):
    R = helpers.ref()
    report = {}
    for name in names:
        iw, ih, frames, (sthr, minerr, sizethr) = STREAMS[name]
        vid = VidPoly(R, iw, ih, (sthr, minerr, sizethr))
        segs, offs, ids_crc, input_crc, vsegs, voffs, vids_crc, differ = [], [0], [], [], [], [0], [], []
        pool = multiprocessing.get_context("spawn").Pool(1, maxtasksperchild=8)
        pending = [pool.apply_async(per_frame, ((name, i),)) for i in range(len(frames))]
        for i, (kind, seed, t) in enumerate(frames):
            img = make_frame(kind, seed, t, iw, ih)
            vs, vids = vid.frame(img)
            lsb, idsb = pending[i].get()
            s = np.frombuffer(lsb, ra.LS_DTYPE).copy()
            ids = np.frombuffer(idsb, np.int32)
            n = int(s.view("i4")[0])
            same = vs.tobytes() == s.tobytes() and np.array_equal(vids, ids)
            if not same:
                differ.append(i)
            segs.append(s); offs.append(offs[-1] + len(s)); ids_crc.append(crc(ids)); input_crc.append(crc(img))
            vsegs.append(vs); voffs.append(voffs[-1] + len(vs)); vids_crc.append(crc(vids))
            print(name, i, kind, t, "segments", n, "vidpoly identical" if same else "VIDPOLY DIFFERS", flush=True)
        vid.close()
        pool.close()
        pool.join()
        out = dict(iw=iw, ih=ih, strength_thre=sthr, minerror=minerr, size_thre=sizethr, kinds=np.array([f[0] for f in frames]),
                   seeds=np.array([f[1] for f in frames], np.int64), ts=np.array([f[2] for f in frames], np.int32),
                   segments=np.concatenate(segs), offsets=np.array(offs, np.int64), ids_crc=np.array(ids_crc, np.uint32), input_crc=np.array(input_crc, np.uint32),
                   vid_differs=np.array(differ, np.int32))
        if differ:      # (the persistent-buffer lists, where they are not the per-frame ones)
            out.update(vid_segments=np.concatenate(vsegs), vid_offsets=np.array(voffs, np.int64), vid_ids_crc=np.array(vids_crc, np.uint32))
        path = os.path.join(helpers.GOLDEN, name + ".npz")
        np.savez_compressed(path, **out)
        report[name] = {"frames": len(frames), "vidpoly_persistent_buffers_differ": differ, "bytes": os.path.getsize(path)}
        print(json.dumps({name: report[name]}), flush=True)
    return report


if __name__ == "__main__":
    main(sys.argv[1:] or list(STREAMS))
