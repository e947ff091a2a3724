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
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tools import benchlib as bl
from tools.benchlib import TAN36

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
    n = 2000
    lat, dt = bl.timed_jobs(job, lambda k: service.wait(), NJOBS, 64, 300, n)
    print(json.dumps(dict({"step": "jobs", "job": label, "repeat": rep, "size": "%dx%d" % (IW, IH), "jobs_in_flight": NJOBS, "jobs": n, "us_per_job_in_flight": round(dt / n * 1e6, 2),
                           **bl.latency_fields(lat)}, **extra)), flush=True)


def child_jobs(repeat):
    import rectdetect_amd as ra
    L = ra.lib()
    frame = bl.synth_frames(IW, IH, 1)[0]
    quads = bl.own_quads(frame)
    if len(quads) == 0:
        raise SystemExit("bench_match: the synthetic frame has no rectangle")
    n = len(quads)
    dframe = bl.upload([frame])[0]
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
    bl.free([dframe, dout])


def child_loop(nslots, pattern):
    import rectdetect_amd as ra
    L = ra.lib()
    frames, warmup = 1024, 128
    dptrs = bl.upload(bl.synth_frames(IW, IH, 16))
    outs = [L.rd_device_alloc(64 * P * P * 3) for _ in range(NJOBS)]
    rect = ra.Rectifier(P, P, max_quads=64, njobs=NJOBS)
    mt = ra.Matcher(G, M, max_templates=16, max_quads=64, njobs=NJOBS)
    library(mt, 16)
    workers = {"rectify": rect, "match": mt}

    def enqueue(det, i):
        det.enqueue(dptrs[i % 16], IW * 3, on_device=True)

    def run(det, mode, timed, tally):
        def behind(det, worker, rects, i, k):
            quads = ra.rect_quads(rects[:64])
            if mode == "rectify":
                det.rectify_polled(rect, quads, outs[k % NJOBS])
            else:
                det.match_polled(mt, quads)
            return len(quads)

        bl.detector_loop(det, frames if timed else warmup, nslots, enqueue, tally, first=warmup if timed else 0, worker=workers.get(mode), njobs=NJOBS, behind=behind)

    for r, mode, dt, tally in bl.detector_runs(pattern, lambda: ra.Detector(IW, IH, nslots=nslots, nworkers=1, aperture=TAN36), run):
        print(json.dumps({"step": "loop", "size": "%dx%d" % (IW, IH), "nslots": nslots, "behind_the_poll": mode, "run": r, "first_detector_of_process": r == 0, "frames": frames,
                          "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "quads_per_frame": round(tally[2] / frames, 1), "templates": 16, "grid": G, "oversample": M,
                          "frames_kind": "device"}), flush=True)
    rect.close()
    mt.close()
    bl.free(outs + dptrs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", default="jobs,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=2, help="rounds of the alternating runs in either step")
    ap.add_argument("--timeout", type=int, default=300, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "match_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        bl.require_gpu("bench_match")
        if a.child == "jobs":
            child_jobs(a.repeat)
        else:
            child_loop(a.nslots, list(LOOP_MODES) * a.repeat)
        return 0
    cmd = lambda step: [sys.executable, os.path.abspath(__file__), "--child", step, "--nslots", str(a.nslots), "--repeat", str(a.repeat)]
    return bl.drive("bench_match", a.steps.split(","), cmd, a.out, a.timeout)


if __name__ == "__main__":
    sys.exit(main())
