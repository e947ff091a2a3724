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
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.bench_rectify import random_quads, synth_frames

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
NJOBS = 4
IW, IH = 1920, 1080
LOOP_MODES = ("none", "rectify", "annotate", "annotate_out")


def timed_jobs(an, job, label, extra):
    for k in range(64):      # warm-up
        job(k)
        an.wait()
    lat = []
    for k in range(300):
        t = time.perf_counter()
        job(k)
        an.wait()
        lat.append(time.perf_counter() - t)
    n = 4000
    t = time.perf_counter()
    inflight = 0
    for k in range(n):
        if inflight == NJOBS:
            an.wait()
            inflight -= 1
        job(k)
        inflight += 1
    while inflight:
        an.wait()
        inflight -= 1
    dt = time.perf_counter() - t
    lat = np.sort(np.array(lat)) * 1e6
    print(json.dumps(dict({"step": "jobs", "job": label, "size": "%dx%d" % (IW, IH), "jobs_in_flight": NJOBS, "jobs": n, "us_per_job_in_flight": round(dt / n * 1e6, 2),
                           "job_latency_us_median": round(float(lat[len(lat) // 2]), 1), "job_latency_us_p10": round(float(lat[len(lat) // 10]), 1),
                           "job_latency_us_p90": round(float(lat[len(lat) * 9 // 10]), 1)}, **extra)), flush=True)


def child_jobs():
    import rectdetect_amd as ra
    from tests import pixfmt
    L = ra.lib()
    frame = synth_frames(IW, IH, 1)[0]
    det = ra.Detector(IW, IH, nslots=1, aperture=TAN36)
    det.enqueue(frame)
    rect_prims = ra.annot_rects(det.poll(TAN36))
    det.close()
    pdet = ra.PolylineDetector(IW, IH, nslots=1, strength_thre=2000, minerror=1.0, size_thre=10)
    pdet.enqueue(frame)
    seg_prims = ra.annot_segments(pdet.poll()[0], ra.ANNOT_SEG_ALL)
    pdet.close()
    an = ra.Annotator(max_prims=max(len(rect_prims), len(seg_prims), 1), njobs=NJOBS)
    dframe = L.rd_device_alloc(frame.nbytes)
    L.rd_upload(dframe, frame.ctypes.data, frame.nbytes)
    timed_jobs(an, lambda k: an.enqueue(ra.PIX_BGR, (dframe,), (IW * 3,), IW, IH, rect_prims, on_device=True), "a: rectangles, BGR in place",
               {"primitives": len(rect_prims), "format": "BGR", "frames": "device, in place", "clear": False})
    timed_jobs(an, lambda k: an.enqueue(ra.PIX_BGR, (dframe,), (IW * 3,), IW, IH, seg_prims, ra.ANNOT_CLEAR, on_device=True), "b: segments on black, BGR in place",
               {"primitives": len(seg_prims), "format": "BGR", "frames": "device, in place", "clear": True})
    (y, uv), _ = pixfmt.convert(frame, ra.PIX_NV12)
    y, uv = np.ascontiguousarray(y), np.ascontiguousarray(uv)
    src = [L.rd_device_alloc(y.nbytes), L.rd_device_alloc(uv.nbytes)]
    dst = [L.rd_device_alloc(y.nbytes), L.rd_device_alloc(uv.nbytes)]
    L.rd_upload(src[0], y.ctypes.data, y.nbytes)
    L.rd_upload(src[1], uv.ctypes.data, uv.nbytes)
    timed_jobs(an, lambda k: an.enqueue(ra.PIX_NV12, src, (IW, IW), IW, IH, seg_prims, ra.ANNOT_CLEAR, out_planes=dst, out_pitches=(IW, IW), on_device=True),
               "c: segments on black, NV12 device to device", {"primitives": len(seg_prims), "format": "NV12", "frames": "device to device", "clear": True})
    timed_jobs(an, lambda k: an.enqueue(ra.PIX_NV12, src, (IW, IW), IW, IH, rect_prims, out_planes=dst, out_pitches=(IW, IW), on_device=True),
               "rectangles, NV12 device to device", {"primitives": len(rect_prims), "format": "NV12", "frames": "device to device", "clear": False})
    an.close()
    for q in [dframe] + src + dst:
        L.rd_device_free(q)


def child_loop(nslots, pattern):
    import rectdetect_amd as ra
    L = ra.lib()
    # a pool with a device frame of its own for EVERY frame of a run (16 images in turn, 7 GB): in place each frame is drawn into once, after its detection, and never
    # detected again, so the detector's work is the same in all four modes; and no frame in flight is ever drawn into
    frames, warmup, p = 1024, 128, 128
    base = synth_frames(IW, IH, 16)
    imgs = [base[k % 16] for k in range(frames + warmup)]
    dptrs = []
    for a in imgs:
        q = L.rd_device_alloc(a.nbytes)
        L.rd_upload(q, a.ctypes.data, a.nbytes)
        dptrs.append(q)
    quads = random_quads(IW, IH, 32)
    outs = [L.rd_device_alloc(32 * p * p * 3) for _ in range(NJOBS)]
    oframes = [L.rd_device_alloc(IW * IH * 3) for _ in range(NJOBS)]
    rect = ra.Rectifier(p, p, max_quads=32, njobs=NJOBS)
    an = ra.Annotator(max_prims=1024, njobs=NJOBS)

    def run(det, first, n, mode, tally):
        inflight = jobs = 0
        worker = rect if mode == "rectify" else an

        def poll():
            nonlocal jobs
            rects = det.poll(TAN36)
            tally[0] += len(rects)
            if mode == "none":
                return
            if jobs == NJOBS:
                worker.wait()
                jobs -= 1
            if mode == "rectify":
                det.rectify_polled(rect, quads, outs[tally[1] % NJOBS])
            else:
                prims = ra.annot_rects(rects[:170])
                tally[2] += len(prims)
                if mode == "annotate":
                    det.annotate_polled(an, prims)
                else:
                    det.annotate_polled(an, prims, out_planes=(oframes[tally[1] % NJOBS],), out_pitches=(IW * 3,))
            tally[1] += 1
            jobs += 1

        for i in range(n):
            if inflight == nslots:
                poll()
                inflight -= 1
            det.enqueue(dptrs[first + i], IW * 3, on_device=True)
            inflight += 1
        while inflight:
            poll()
            inflight -= 1
        while jobs:
            worker.wait()
            jobs -= 1

    for r, mode in enumerate(pattern):
        det = ra.Detector(IW, IH, nslots=nslots, nworkers=1, aperture=TAN36)
        run(det, 0, warmup, mode, [0, 0, 0])
        tally = [0, 0, 0]
        t = time.perf_counter()
        run(det, warmup, frames, mode, tally)      # (ends with every frame polled and every job waited for)
        dt = time.perf_counter() - t
        det.close()
        if mode == "annotate":      # (the next run starts from the pool as it was uploaded)
            for q, a in zip(dptrs, imgs):
                L.rd_upload(q, a.ctypes.data, a.nbytes)
        print(json.dumps({"step": "loop", "size": "%dx%d" % (IW, IH), "nslots": nslots, "behind_the_poll": mode, "run": r, "first_detector_of_process": r == 0, "frames": frames,
                          "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "primitives_per_frame": round(tally[2] / frames, 1), "frames_kind": "device"}), flush=True)
    rect.close()
    an.close()
    for q in outs + oframes + dptrs:
        L.rd_device_free(q)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", default="jobs,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3, help="rounds of (none, rectify, annotate, annotate_out) in the loop step")
    ap.add_argument("--pattern", default=None, help="the loop step's runs in one process, e.g. none,none,annotate (default: all four --repeat times)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annotate_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    pattern = a.pattern or ",".join([",".join(LOOP_MODES)] * a.repeat)
    if a.child:
        import rectdetect_amd as ra
        if not ra.gpu_available():
            raise SystemExit("bench_annotate: no HIP device - nothing is measured without one")
        if a.child == "jobs":
            child_jobs()
        else:
            modes = pattern.split(",")
            if any(m not in LOOP_MODES for m in modes):
                raise SystemExit("bench_annotate: --pattern takes %s" % ", ".join(LOOP_MODES))
            child_loop(a.nslots, modes)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--nslots", str(a.nslots), "--pattern", pattern]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print("bench_annotate: step %s ran into its time limit of %d s - stopping" % (step, a.timeout), file=sys.stderr)
            return 124
        text = res.stdout.decode()
        sys.stdout.write(text)
        sys.stdout.flush()
        if res.returncode != 0:
            print("bench_annotate: step %s failed with status %d - stopping" % (step, res.returncode), file=sys.stderr)
            return res.returncode if res.returncode > 0 else 1
        with open(a.out, "a") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
