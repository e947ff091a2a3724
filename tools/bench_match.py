#!/usr/bin/env python3
"""Rates of the matcher (rd_matcher, rd_detector_match_polled) at 1920x1080: JSON lines, appended to profiles/match_bench.jsonl (--out).

  * "jobs":  microseconds per job - the latency of one job (enqueue to wait, nothing else on the device) and the time per job with four jobs kept in flight - on the
             rectangles of a frame of the synthetic stream (about ten quads), a BGR frame resident in HBM: the matcher at G = 32, m = 4 against T = 16 and against
             T = 1024 templates (noise images), and the rectifier's 128x128 job on the same quads into device memory - the same sampling work without the
             signature, the dots and the choice.  The three alternate --repeat times in one process.
  * "loop":  the rectangle detector's frames/s (64 slots, post-process on a worker thread, frames resident in HBM - the loop bench.py times) three ways in one
             process: nothing behind the poll, rectify_polled of the frame's own rectangles into 128x128 patches, match_polled of the frame's own rectangles against
             16 templates.  The runs alternate --repeat times, a new detector per run, so each is the others' baseline on the same machine state (the first detector
             of a process runs faster than every later one: DESIGN.md, "Rectified patches"; every line says whether it was).  Nothing is written into a frame, so
             the 16 images of the stream have one device buffer each.
Every GPU step is a child process under a time limit of its own; the tool stops at the first one that fails.  bench.py is not involved.

    python tools/bench_match.py [--steps jobs,loop] [--repeat R] [--out FILE]
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

from tools.bench_rectify import synth_frames

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
NJOBS = 4
IW, IH = 1920, 1080
G, M = 32, 4
P = G * M
LOOP_MODES = ("none", "rectify", "match")


def library(matcher, T):
    rng = np.random.default_rng(7)
    for _ in range(T):
        matcher.add_image(rng.integers(0, 256, (P, P, 3), dtype=np.uint8))


def timed_jobs(service, job, label, extra, rep):
    for k in range(64):      # warm-up
        job(k)
        service.wait()
    lat = []
    for k in range(300):
        t = time.perf_counter()
        job(k)
        service.wait()
        lat.append(time.perf_counter() - t)
    n = 2000
    t = time.perf_counter()
    inflight = 0
    for k in range(n):
        if inflight == NJOBS:
            service.wait()
            inflight -= 1
        job(k)
        inflight += 1
    while inflight:
        service.wait()
        inflight -= 1
    dt = time.perf_counter() - t
    lat = np.sort(np.array(lat)) * 1e6
    print(json.dumps(dict({"step": "jobs", "job": label, "repeat": rep, "size": "%dx%d" % (IW, IH), "jobs_in_flight": NJOBS, "jobs": n, "us_per_job_in_flight": round(dt / n * 1e6, 2),
                           "job_latency_us_median": round(float(lat[len(lat) // 2]), 1), "job_latency_us_p10": round(float(lat[len(lat) // 10]), 1),
                           "job_latency_us_p90": round(float(lat[len(lat) * 9 // 10]), 1)}, **extra)), flush=True)


def child_jobs(repeat):
    import rectdetect_amd as ra
    L = ra.lib()
    frame = synth_frames(IW, IH, 1)[0]
    det = ra.Detector(IW, IH, nslots=1, aperture=TAN36)
    det.enqueue(frame)
    quads = ra.rect_quads(det.poll(TAN36))
    det.close()
    if len(quads) == 0:
        raise SystemExit("bench_match: the synthetic frame has no rectangle")
    n = len(quads)
    dframe = L.rd_device_alloc(frame.nbytes)
    L.rd_upload(dframe, frame.ctypes.data, frame.nbytes)
    dout = L.rd_device_alloc(n * P * P * 3)
    matchers = {}
    for T in (16, 1024):
        matchers[T] = ra.Matcher(G, M, max_templates=T, max_quads=n, njobs=NJOBS)
        library(matchers[T], T)
    rect = ra.Rectifier(P, P, max_quads=n, njobs=NJOBS)
    for rep in range(repeat):
        for T in (16, 1024):
            mt = matchers[T]
            timed_jobs(mt, lambda k: mt.enqueue(ra.PIX_BGR, (dframe,), (IW * 3,), IW, IH, quads, on_device=True), "match, G = %d, m = %d, T = %d" % (G, M, T),
                       {"quads": n, "templates": T, "grid": G, "oversample": M, "format": "BGR", "frames": "device"}, rep)
        timed_jobs(rect, lambda k: rect.enqueue(ra.PIX_BGR, (dframe,), (IW * 3,), IW, IH, quads, dout, on_device=True), "rectify, %dx%d patches to device memory" % (P, P),
                   {"quads": n, "format": "BGR", "frames": "device"}, rep)
    for mt in matchers.values():
        mt.close()
    rect.close()
    L.rd_device_free(dframe)
    L.rd_device_free(dout)


def child_loop(nslots, pattern):
    import rectdetect_amd as ra
    L = ra.lib()
    frames, warmup = 1024, 128
    base = synth_frames(IW, IH, 16)
    dptrs = []
    for a in base:
        q = L.rd_device_alloc(a.nbytes)
        L.rd_upload(q, a.ctypes.data, a.nbytes)
        dptrs.append(q)
    outs = [L.rd_device_alloc(64 * P * P * 3) for _ in range(NJOBS)]
    rect = ra.Rectifier(P, P, max_quads=64, njobs=NJOBS)
    mt = ra.Matcher(G, M, max_templates=16, max_quads=64, njobs=NJOBS)
    library(mt, 16)
    workers = {"rectify": rect, "match": mt}

    def run(det, first, n, mode, tally):
        inflight = jobs = 0
        worker = workers.get(mode)

        def poll():
            nonlocal jobs
            rects = det.poll(TAN36)
            tally[0] += len(rects)
            if mode == "none":
                return
            if jobs == NJOBS:
                worker.wait()
                jobs -= 1
            quads = ra.rect_quads(rects[:64])
            tally[2] += len(quads)
            if mode == "rectify":
                det.rectify_polled(rect, quads, outs[tally[1] % NJOBS])
            else:
                det.match_polled(mt, quads)
            tally[1] += 1
            jobs += 1

        for i in range(n):
            if inflight == nslots:
                poll()
                inflight -= 1
            det.enqueue(dptrs[(first + i) % 16], IW * 3, on_device=True)
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
        print(json.dumps({"step": "loop", "size": "%dx%d" % (IW, IH), "nslots": nslots, "behind_the_poll": mode, "run": r, "first_detector_of_process": r == 0, "frames": frames,
                          "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "quads_per_frame": round(tally[2] / frames, 1), "templates": 16, "grid": G, "oversample": M,
                          "frames_kind": "device"}), flush=True)
    rect.close()
    mt.close()
    for q in outs + dptrs:
        L.rd_device_free(q)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", default="jobs,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=2, help="rounds of the alternating runs in either step")
    ap.add_argument("--timeout", type=int, default=300, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        import rectdetect_amd as ra
        if not ra.gpu_available():
            raise SystemExit("bench_match: no HIP device - nothing is measured without one")
        if a.child == "jobs":
            child_jobs(a.repeat)
        else:
            child_loop(a.nslots, list(LOOP_MODES) * a.repeat)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--nslots", str(a.nslots), "--repeat", str(a.repeat)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print("bench_match: step %s ran into its time limit of %d s - stopping" % (step, a.timeout), file=sys.stderr)
            return 124
        text = res.stdout.decode()
        sys.stdout.write(text)
        sys.stdout.flush()
        if res.returncode != 0:
            print("bench_match: step %s failed with status %d - stopping" % (step, res.returncode), file=sys.stderr)
            return res.returncode if res.returncode > 0 else 1
        with open(a.out, "a") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
