#!/usr/bin/env python3
"""Frame rate of the polyline kind of rd_detector (rd_polyline_detector_create, vidpoly.cpp's parameters 2000 / 1 / 10) on synthetic streams: one JSON
line per configuration - 1280x720, 1920x1080, 3840x2160 with 64 frames in flight, frames resident in HBM and in pinned host memory - with the counters
(multi-launch repeats, long lists, frames per group launch) and the device bytes of one slot.  bench.py (the rectangle kind) is not involved.

    python tools/bench_polyline.py [--frames K] [--warmup W] [--nslots S] [--sizes 1280x720,1920x1080,3840x2160]
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


def measure(iw, ih, where, nslots, frames, warmup, distinct=16):
    L = ra.lib()
    nb = iw * ih * 3
    imgs = synth_frames(iw, ih, distinct)
    alloc, free = (L.rd_device_alloc, L.rd_device_free) if where == "device" else (L.rd_host_alloc, L.rd_host_free)
    # one buffer per slot (a buffer stays unchanged until its frame's poll), filled from the distinct frames
    bufs = [alloc(nb) for _ in range(nslots)]
    for k, p in enumerate(bufs):
        if where == "device":
            L.rd_upload(p, imgs[k % distinct].ctypes.data, nb)
        else:
            ctypes.memmove(p, imgs[k % distinct].ctypes.data, nb)
    det = ra.PolylineDetector(iw, ih, nslots=nslots, strength_thre=2000, minerror=1.0, size_thre=10)
    segs = 0

    def run(n):
        nonlocal segs
        inflight = 0
        for i in range(n):
            if inflight == nslots:
                s, _ = det.poll()
                segs += int(s.view("i4")[0])
                inflight -= 1
            det.enqueue(bufs[i % nslots], ws=iw * 3, on_device=where == "device", pinned=where == "pinned")
            inflight += 1
        while inflight:
            s, _ = det.poll()
            segs += int(s.view("i4")[0])
            inflight -= 1

    run(warmup)
    segs = 0
    t0 = time.perf_counter()
    run(frames)
    dt = time.perf_counter() - t0
    res = {"config": "polyline %dx%d %s frames, %d in flight" % (iw, ih, "resident" if where == "device" else "pinned host", nslots),
           "frames_per_s": round(frames / dt, 1), "frames": frames, "segments_per_frame": round(segs / frames, 1),
           "multilaunch_repeats": det.counter(0), "long_lists": det.counter(30), "frames_per_group_launch": det.counter(15),
           "handoff_records": det.counter(32), "slot_bytes": det.counter(31), "device_us_per_frame": round(det.counter(1) / max(det.counter(2), 1), 1)}
    det.close()
    for p in bufs:
        free(p)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--sizes", default="1280x720,1920x1080,3840x2160")
    a = ap.parse_args()
    if not ra.gpu_available():
        raise SystemExit("bench_polyline: no HIP device - the product has no CPU path")
    for size in a.sizes.split(","):
        iw, ih = (int(v) for v in size.split("x"))
        big = iw * ih > 1920 * 1088
        for where in ("device", "pinned"):
            print(json.dumps(measure(iw, ih, where, a.nslots, a.frames // 4 if big else a.frames, a.warmup // 4 if big else a.warmup)), flush=True)


if __name__ == "__main__":
    main()
