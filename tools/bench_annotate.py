#!/usr/bin/env python3
"""Rates of the annotator (rd_annotator, rd_detector_annotate_polled) at 1920x1080: JSON lines, appended to profiles/annotate_bench.jsonl (--out).

  * "jobs":  microseconds per job - the latency of one job (enqueue to wait, nothing else on the device) and the time per job with the annotator's jobs kept in flight -
             for (a) the rectangle primitives of a frame of the synthetic stream, in place in a BGR frame; (b) the segments of the same frame from the polyline
             detector with vidpoly.cpp's parameters, RD_ANNOT_CLEAR, in place in a BGR frame; (c) job (b) from one NV12 frame into another;
  * "loop":  the rectangle detector's frames/s (64 slots, post-process on worker threads, frames resident in HBM - the loop bench.py times) four ways in one process:
             nothing behind the poll, rectify_polled of 32 quads into 128x128 patches, annotate_polled of the frame's own rectangles in place, and the same into another
             frame.  The runs alternate --repeat times, a new detector per run, so each is the others' baseline on the same machine state (the first detector of a
             process runs faster than every later one: DESIGN.md, "Rectified patches").  Every frame of a run has a device buffer of its own, so a frame drawn into in place
             is never detected again and the detector's work is the same in all four ("rectangles" shows it); the pool is uploaded afresh after every in-place run.
Every GPU step is a child process under a time limit of its own; the tool stops at the first one that fails.  bench.py is not involved.

    python tools/bench_annotate.py [--steps jobs,loop] [--repeat R] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tools import benchlib as bl
from tools.benchlib import TAN36

NJOBS = 4
IW, IH = 1920, 1080
LOOP_MODES = ("none", "rectify", "annotate", "annotate_out")


def timed_jobs(an, job, label, extra):
    n = 4000
    lat, dt = bl.timed_jobs(job, lambda k: an.wait(), NJOBS, 64, 300, n)
    print(json.dumps(dict({"step": "jobs", "job": label, "size": "%dx%d" % (IW, IH), "jobs_in_flight": NJOBS, "jobs": n, "us_per_job_in_flight": round(dt / n * 1e6, 2),
                           **bl.latency_fields(lat)}, **extra)), flush=True)


def child_jobs():
    import rectdetect_amd as ra
    from tests import pixfmt
    L = ra.lib()
    frame = bl.synth_frames(IW, IH, 1)[0]
    det = ra.Detector(IW, IH, nslots=1, aperture=TAN36)
    det.enqueue(frame)
    rect_prims = ra.annot_rects(det.poll(TAN36))
    det.close()
    pdet = ra.PolylineDetector(IW, IH, nslots=1, strength_thre=2000, minerror=1.0, size_thre=10)
    pdet.enqueue(frame)
    seg_prims = ra.annot_segments(pdet.poll()[0], ra.ANNOT_SEG_ALL)
    pdet.close()
    an = ra.Annotator(max_prims=max(len(rect_prims), len(seg_prims), 1), njobs=NJOBS)
    dframe = bl.upload([frame])[0]
    timed_jobs(an, lambda k: an.enqueue(ra.PIX_BGR, (dframe,), (IW * 3,), IW, IH, rect_prims, on_device=True), "a: rectangles, BGR in place",
               {"primitives": len(rect_prims), "format": "BGR", "frames": "device, in place", "clear": False})
    timed_jobs(an, lambda k: an.enqueue(ra.PIX_BGR, (dframe,), (IW * 3,), IW, IH, seg_prims, ra.ANNOT_CLEAR, on_device=True), "b: segments on black, BGR in place",
               {"primitives": len(seg_prims), "format": "BGR", "frames": "device, in place", "clear": True})
    (y, uv), _ = pixfmt.convert(frame, ra.PIX_NV12)
    y, uv = np.ascontiguousarray(y), np.ascontiguousarray(uv)
    src = bl.upload([y, uv])
    dst = [L.rd_device_alloc(y.nbytes), L.rd_device_alloc(uv.nbytes)]
    timed_jobs(an, lambda k: an.enqueue(ra.PIX_NV12, src, (IW, IW), IW, IH, seg_prims, ra.ANNOT_CLEAR, out_planes=dst, out_pitches=(IW, IW), on_device=True),
               "c: segments on black, NV12 device to device", {"primitives": len(seg_prims), "format": "NV12", "frames": "device to device", "clear": True})
    timed_jobs(an, lambda k: an.enqueue(ra.PIX_NV12, src, (IW, IW), IW, IH, rect_prims, out_planes=dst, out_pitches=(IW, IW), on_device=True),
               "rectangles, NV12 device to device", {"primitives": len(rect_prims), "format": "NV12", "frames": "device to device", "clear": False})
    an.close()
    bl.free([dframe] + src + dst)


def child_loop(nslots, pattern):
    import rectdetect_amd as ra
    L = ra.lib()
    # a pool with a device frame of its own for EVERY frame of a run (16 images in turn, 7 GB): in place each frame is drawn into once, after its detection, and never
    # detected again, so the detector's work is the same in all four modes; and no frame in flight is ever drawn into
    frames, warmup, p = 1024, 128, 128
    base = bl.synth_frames(IW, IH, 16)
    imgs = [base[k % 16] for k in range(frames + warmup)]
    dptrs = bl.upload(imgs)
    quads = bl.random_quads(IW, IH, 32)
    outs = [L.rd_device_alloc(32 * p * p * 3) for _ in range(NJOBS)]
    oframes = [L.rd_device_alloc(IW * IH * 3) for _ in range(NJOBS)]
    rect = ra.Rectifier(p, p, max_quads=32, njobs=NJOBS)
    an = ra.Annotator(max_prims=1024, njobs=NJOBS)

    def enqueue(det, i):
        det.enqueue(dptrs[i], IW * 3, on_device=True)

    def run(det, mode, timed, tally):
        def behind(det, worker, rects, i, k):
            if mode == "rectify":
                det.rectify_polled(rect, quads, outs[k % NJOBS])
                return 0
            prims = ra.annot_rects(rects[:170])
            if mode == "annotate":
                det.annotate_polled(an, prims)
            else:
                det.annotate_polled(an, prims, out_planes=(oframes[k % NJOBS],), out_pitches=(IW * 3,))
            return len(prims)

        worker = None if mode == "none" else (rect if mode == "rectify" else an)
        bl.detector_loop(det, frames if timed else warmup, nslots, enqueue, tally, first=warmup if timed else 0, worker=worker, njobs=NJOBS, behind=behind)

    for r, mode, dt, tally in bl.detector_runs(pattern, lambda: ra.Detector(IW, IH, nslots=nslots, nworkers=1, aperture=TAN36), run):
        if mode == "annotate":      # (the next run starts from the pool as it was uploaded)
            for q, a in zip(dptrs, imgs):
                L.rd_upload(q, a.ctypes.data, a.nbytes)
        print(json.dumps({"step": "loop", "size": "%dx%d" % (IW, IH), "nslots": nslots, "behind_the_poll": mode, "run": r, "first_detector_of_process": r == 0, "frames": frames,
                          "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "primitives_per_frame": round(tally[2] / frames, 1), "frames_kind": "device"}), flush=True)
    rect.close()
    an.close()
    bl.free(outs + oframes + dptrs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", default="jobs,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3, help="rounds of (none, rectify, annotate, annotate_out) in the loop step")
    ap.add_argument("--pattern", default=None, help="the loop step's runs in one process, e.g. none,none,annotate (default: all four --repeat times)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "annotate_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    pattern = a.pattern or ",".join([",".join(LOOP_MODES)] * a.repeat)
    if a.child:
        bl.require_gpu("bench_annotate")
        if a.child == "jobs":
            child_jobs()
        else:
            modes = pattern.split(",")
            if any(m not in LOOP_MODES for m in modes):
                raise SystemExit("bench_annotate: --pattern takes %s" % ", ".join(LOOP_MODES))
            child_loop(a.nslots, modes)
        return 0
    cmd = lambda step: [sys.executable, os.path.abspath(__file__), "--child", step, "--nslots", str(a.nslots), "--pattern", pattern]
    return bl.drive("bench_annotate", a.steps.split(","), cmd, a.out, a.timeout)


if __name__ == "__main__":
    sys.exit(main())
