#!/usr/bin/env python3
"""Frame rate of half-size detection (rd_detector_enqueue_scaled, scale 2) against its two alternatives: one JSON line per configuration, format and round, with
the source bytes handed over per frame, the group launches (rd_detector_counter 16 + 17) and the rectangles found.  64 slots, tan 36 deg, device frames, the
synthetic stream after its 4:2:0 round trip (as tools/bench_formats.py prepares it).  bench.py is not involved.

    a   the full-size source (default 3840x2160) at scale 2 into a detector of half its size: the feature
    b   half() of those frames - the contract's 2x2 box average, made on the host - as frames of the detector's own size at scale 1: the same detector work
        as (a), so that (a) against (b) is the cost of the wider read in the front kernel
    c   the full-size frames at scale 1 into a full-size detector: what a caller had to do until now

The three run alternating within one call (--repeat rounds of a, b, c per format), so that they are compared on the same machine state.  BGR and BGRA show the
detector of (a) and of (b) the same image in every byte, and the tool fails unless both find the same number of rectangles; an NV12 frame of (b) is the 4:2:0
round trip of the half-size image - the nearest an NV12 frame of that size can come - so its image, and possibly its count, differs a little ("same_image":
false on those lines).  Then one line each for pinned and pageable host frames of (a), NV12.

    python tools/bench_scaled.py [--size 3840x2160] [--formats NV12,BGR,BGRA] [--repeat R] [--frames K] [--warmup W] [--distinct D] [--no-host]
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
from tools import benchlib
from tests import pixfmt

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
FMT = {v: k for k, v in ra.PIX_NAMES.items()}


def half(a):
    """the contract of rd_detector_enqueue_scaled, scale 2"""
    a = a.astype(np.int32)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def synth_frames(iw, ih, n):
    """n distinct frames of the synthetic stream (C generator), seed 0x5EED0000, and for each the BGR frame the conversion contract gives for its I420 planes"""
    return [(a, pixfmt.convert(a, ra.PIX_I420)[1]) for a in benchlib.synth_frames(iw, ih, n)]


class Frames:
    """planes of the distinct frames in device / pinned memory (never written while frames are in flight), or as numpy arrays for host frames"""

    def __init__(self, planes, fmt, kind, scale):
        L = ra.lib()
        self.kind, self.fmt, self.scale, self.planes = kind, fmt, scale, planes
        self.bytes = sum(p.nbytes for p in planes[0])
        self.pitches = [p.strides[0] for p in planes[0]]
        self.ptrs = []
        if kind == "host":
            return
        for pl in planes:
            ps = []
            for p in pl:
                p = np.ascontiguousarray(p)
                q = L.rd_device_alloc(p.nbytes) if kind == "device" else L.rd_host_alloc(p.nbytes)
                if kind == "device":
                    L.rd_upload(q, p.ctypes.data, p.nbytes)
                else:
                    ctypes.memmove(q, p.ctypes.data, p.nbytes)
                ps.append(q)
            self.ptrs.append(ps)

    def enqueue(self, det, i):
        if self.kind == "host":
            return det.enqueue_scaled(self.fmt, self.planes[i % len(self.planes)], scale=self.scale)
        return det.enqueue_scaled(self.fmt, self.ptrs[i % len(self.ptrs)], self.pitches, on_device=self.kind == "device", pinned=self.kind == "pinned", scale=self.scale)

    def close(self):
        free = ra.lib().rd_device_free if self.kind == "device" else ra.lib().rd_host_free
        for ps in self.ptrs:
            for q in ps:
                free(q)
        self.ptrs = []


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
    staging = L.rd_detector_counter(det.h, 33)
    det.close()
    return {"detector": "%dx%d" % (iw, ih), "format": ra.PIX_NAMES[fr.fmt], "scale": fr.scale, "kind": fr.kind, "nslots": nslots, "frames": frames,
            "frames_per_s": round(frames / dt, 1), "source_bytes_per_frame": fr.bytes, "group_launches": int(groups), "rectangles": rects, "scaled_staging_bytes": int(staging)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="3840x2160", help="the source's size (the detector of a and b is half of it)")
    ap.add_argument("--formats", default="NV12,BGR,BGRA")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--frames", type=int, default=0, help="timed frames per run of a and b (default 1024; c takes a quarter)")
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=8, help="distinct frames of the stream")
    ap.add_argument("--no-host", action="store_true", help="skip the pinned / pageable lines of (a)")
    a = ap.parse_args()
    sw, sh = (int(v) for v in a.size.split("x"))
    iw, ih = sw // 2, sh // 2
    frames = a.frames or 1024
    imgs = synth_frames(sw, sh, a.distinct)
    for name in a.formats.split(","):
        fmt = FMT[name]
        yuv = fmt >= ra.PIX_NV12
        # (a), (c): the source in format fmt whose contract frame is the stream's 4:2:0 round trip; (b): half() of that frame in format fmt
        full = [pixfmt.convert(img, fmt)[0] if yuv else pixfmt.convert(rt, fmt)[0] for img, rt in imgs]
        small = [pixfmt.convert(half(rt), fmt)[0] for _, rt in imgs]
        sets = {"a": (Frames(full, fmt, "device", 2), iw, ih, frames), "b": (Frames(small, fmt, "device", 1), iw, ih, frames)}
        sets["c"] = (Frames(full, fmt, "device", 1), sw, sh, max(frames // 4, a.nslots))
        sets["c"][0].ptrs, sets["c"][0].pitches = sets["a"][0].ptrs, sets["a"][0].pitches      # (the same planes on the device)
        try:
            for r in range(a.repeat):
                found = {}
                for label in ("a", "b", "c"):
                    fr, w, h, n = sets[label]
                    rec = measure(w, h, fr, a.nslots, n, min(a.warmup, n))
                    rec.update({"config": label, "round": r, "same_image": not yuv or label != "b"})
                    found[label] = rec["rectangles"]
                    print(json.dumps(rec), flush=True)
                if not yuv and found["a"] != found["b"]:
                    raise SystemExit("bench_scaled: (a) found %d rectangles and (b) %d on the same images (%s)" % (found["a"], found["b"], name))
        finally:
            sets["c"][0].ptrs = []
            for fr, _, _, _ in sets.values():
                fr.close()
        if yuv and not a.no_host:
            for kind in ("pinned", "host"):
                fr = Frames(full, fmt, kind, 2)
                try:
                    rec = measure(iw, ih, fr, a.nslots, frames, a.warmup)
                    rec.update({"config": "a", "round": 0, "same_image": True})
                    print(json.dumps(rec), flush=True)
                finally:
                    fr.close()


if __name__ == "__main__":
    main()
