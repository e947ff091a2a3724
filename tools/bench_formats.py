#!/usr/bin/env python3
"""Frame rate of the rectangle detector per pixel format (rd_detector_enqueue_planes) and frame kind: one JSON line per size, format and kind, with the bytes
handed over per frame and the group launches (rd_detector_counter 16 + 17).  64 slots, tan 36 deg, the synthetic stream.  The formats run alternating within
one call (--repeat rounds of BGR, NV12, I420, RGBA, ...), so that each is compared against BGR on the same machine state.  bench.py is not involved.

Every format shows the detector the SAME images: the synthetic frames after their 4:2:0 round trip (the BGR frames the conversion contract gives for their NV12 /
I420 planes), so that the later stages, whose work depends on the content, do the same work for every format.  Each line carries the number of rectangles found,
which is therefore the same for every format of a size.  --align A: rows of device / pinned planes padded to a multiple of A bytes (pinned frames then travel by
2D copies).

    python tools/bench_formats.py [--sizes 1920x1080,3840x2160] [--formats BGR,NV12,I420,RGBA] [--kinds device,pinned,host] [--frames K] [--warmup W] [--repeat R] [--align A]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rectdetect_amd as ra
from tools.benchlib import synth_frames
from tests import pixfmt

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
FMT = {v: k for k, v in ra.PIX_NAMES.items()}


def same_content(img, fmt):
    """the planes of `img` in format fmt such that the detector sees the contract BGR frame of img's I420 planes whatever the format: YUV formats take img's own
    planes, the others that BGR frame"""
    if fmt in (ra.PIX_NV12, ra.PIX_I420):
        return pixfmt.convert(img, fmt)[0]
    return pixfmt.convert(pixfmt.convert(img, ra.PIX_I420)[1], fmt)[0]


class Frames:
    """the planes of the distinct frames in device / pinned memory (never written while frames are in flight: several slots may read one), or as numpy arrays
    for host frames"""

    def __init__(self, imgs, fmt, kind, align=0):
        L = ra.lib()
        self.kind, self.fmt, self.align = kind, fmt, align if kind != "host" else 0
        self.planes = [same_content(img, fmt) for img in imgs]
        self.bytes = sum(p.nbytes for p in self.planes[0])
        self.pitches = [p.strides[0] for p in self.planes[0]]
        self.ptrs = []
        if kind == "host":
            return
        if align:
            self.pitches = [(p + align - 1) // align * align for p in self.pitches]
        for planes in self.planes:
            ps = []
            for p, pitch in zip(planes, self.pitches):
                rows = p.shape[0]
                img = np.zeros((rows, pitch), np.uint8)
                img[:, :p.strides[0]] = p.reshape(rows, -1)
                q = L.rd_device_alloc(img.nbytes) if kind == "device" else L.rd_host_alloc(img.nbytes)
                if kind == "device":
                    L.rd_upload(q, img.ctypes.data, img.nbytes)
                else:
                    ctypes.memmove(q, img.ctypes.data, img.nbytes)
                ps.append(q)
            self.ptrs.append(ps)

    def enqueue(self, det, i):
        if self.kind == "host":
            return det.enqueue_planes(self.fmt, self.planes[i % len(self.planes)])
        return det.enqueue_planes(self.fmt, self.ptrs[i % len(self.ptrs)], self.pitches, on_device=self.kind == "device", pinned=self.kind == "pinned")

    def close(self):
        free = ra.lib().rd_device_free if self.kind == "device" else ra.lib().rd_host_free
        for ps in self.ptrs:
            for q in ps:
                free(q)


def measure(iw, ih, fr, nslots, frames, warmup):
    det = ra.Detector(iw, ih, nslots=nslots, aperture=TAN36)
    L = ra.lib()

    rects = 0

    def run(n):
        nonlocal rects
        inflight = 0
        for i in range(n):
            if inflight == nslots:
                rects += len(det.poll(TAN36))
                inflight -= 1
            fr.enqueue(det, i)
            inflight += 1
        while inflight:
            rects += len(det.poll(TAN36))
            inflight -= 1

    run(warmup)
    rects = 0
    g0 = L.rd_detector_counter(det.h, 16) + L.rd_detector_counter(det.h, 17)
    t = time.perf_counter()
    run(frames)
    dt = time.perf_counter() - t
    groups = L.rd_detector_counter(det.h, 16) + L.rd_detector_counter(det.h, 17) - g0
    det.close()
    return {"size": "%dx%d" % (iw, ih), "format": ra.PIX_NAMES[fr.fmt], "kind": fr.kind, "nslots": nslots, "frames": frames,
            "frames_per_s": round(frames / dt, 1), "bytes_per_frame": fr.bytes, "group_launches": int(groups), "rectangles": rects, "align": fr.align}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--formats", default="BGR,NV12,I420,RGBA")
    ap.add_argument("--kinds", default="device,pinned,host")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--frames", type=int, default=0, help="timed frames per run (default: 1024 at 1080p and below, 256 above)")
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--align", type=int, default=0, help="device / pinned plane rows padded to a multiple of this many bytes (0: rows back to back)")
    a = ap.parse_args()
    for size in a.sizes.split(","):
        iw, ih = (int(v) for v in size.split("x"))
        frames = a.frames or (1024 if iw * ih <= 1920 * 1080 else 256)
        imgs = synth_frames(iw, ih, 16)
        for kind in a.kinds.split(","):
            sets = [Frames(imgs, FMT[f], kind, a.align) for f in a.formats.split(",")]
            try:
                for r in range(a.repeat):
                    for fr in sets:
                        rec = measure(iw, ih, fr, a.nslots, frames, a.warmup)
                        rec["round"] = r
                        print(json.dumps(rec), flush=True)
            finally:
                for fr in sets:
                    fr.close()


if __name__ == "__main__":
    main()
