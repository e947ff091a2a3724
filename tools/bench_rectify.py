#!/usr/bin/env python3
"""Rates of the rectifier (rd_rectifier, rd_detector_rectify_polled): one JSON line per configuration, appended to profiles/rectify_bench.jsonl (--out).

For each frame size (1280x720, 1920x1080, 3840x2160) and patch size (64x64, 128x128, 256x256), device frames and a device output:
  * "rates":  patches/s with the rectifier's jobs kept in flight, and the latency of one job (enqueue to wait, nothing else on the device), for 1, 8 and 32 quads
              per job - convex quads from a seeded generator, about a sixth of the frame wide, any rotation, some reaching outside the frame;
  * "loop":   the rectangle detector's frames/s (64 slots, post-process on worker threads, frames resident in HBM - the loop bench.py times) with
              rectify_polled of the frame's own rectangles behind every poll, next to the same loop without it; the two alternate --repeat times in one
              process (--pattern: any other order), a new detector per run, so each is the other's baseline on the same machine state.  The FIRST detector of a
              process runs some 8 % faster than every later one, with or without the rectifier ("Rectified patches"): compare runs 1 and later,
              or two processes that start differently (--pattern 0 and --pattern 1).
Every GPU step is a child process under a time limit of its own; the tool stops at the first one that fails.  bench.py is not involved.

    python tools/bench_rectify.py [--sizes 1280x720,1920x1080,3840x2160] [--patches 64,128,256] [--steps rates,loop] [--repeat R] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import benchlib as bl

NJOBS = 4


def child_rates(iw, ih, p):
    import rectdetect_amd as ra
    dframe = bl.upload(bl.synth_frames(iw, ih, 1))[0]
    outs = [ra.lib().rd_device_alloc(32 * p * p * 3) for _ in range(NJOBS)]
    rect = ra.Rectifier(p, p, max_quads=32, njobs=NJOBS)
    allq = bl.random_quads(iw, ih, 32)
    for nq in (1, 8, 32):
        quads = allq[:nq]
        assert all(ra.rectify_coefficients(q)[1] == 1 for q in quads)
        njobs_timed = 4000
        lat, dt = bl.timed_jobs(lambda k: rect.enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, outs[k % NJOBS], on_device=True), lambda k: rect.wait(), NJOBS, 64, 300, njobs_timed)
        print(json.dumps({"step": "rates", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "quads_per_job": nq, "jobs_in_flight": NJOBS, "jobs": njobs_timed,
                          "patches_per_s": round(njobs_timed * nq / dt, 1), "jobs_per_s": round(njobs_timed / dt, 1), "megapixels_per_s": round(njobs_timed * nq * p * p / dt / 1e6, 1),
                          **bl.latency_fields(lat), "frames": "device", "output": "device"}), flush=True)
    rect.close()
    bl.free(outs + [dframe])


def child_loop(iw, ih, p, nslots, pattern):
    import rectdetect_amd as ra
    rects = {True: ra.Rectifier(p, p, max_quads=64, njobs=NJOBS)}
    for r, rectify, frames, dt, tally in bl.rectify_polled_runs(iw, ih, nslots, pattern, rects):
        print(json.dumps({"step": "loop", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "nslots": nslots, "rectify_polled": rectify, "run": r, "first_detector_of_process": r == 0, "frames": frames,
                          "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "patches_per_s": round(tally[2] / dt, 1),
                          "frames_kind": "device", "output": "device"}), flush=True)
    rects[True].close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default="1280x720,1920x1080,3840x2160")
    ap.add_argument("--patches", default="64,128,256")
    ap.add_argument("--steps", default="rates,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3, help="rounds of (without, with) in the loop step")
    ap.add_argument("--pattern", default=None, help="the loop step's runs in one process as 0 (without) / 1 (with rectify_polled), e.g. 0,0,1,0 (default: 0,1 --repeat times)")
    ap.add_argument("--timeout", type=int, default=150, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "rectify_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    pattern = a.pattern or ",".join(["0,1"] * a.repeat)
    if a.child:
        iw, ih = (int(v) for v in a.sizes.split("x"))
        bl.require_gpu("bench_rectify")
        if a.child == "rates":
            child_rates(iw, ih, int(a.patches))
        else:
            child_loop(iw, ih, int(a.patches), a.nslots, [v == "1" for v in pattern.split(",")])
        return 0
    steps = [(step, size, p) for step in a.steps.split(",") for size in a.sizes.split(",") for p in a.patches.split(",")]
    cmd = lambda s: [sys.executable, os.path.abspath(__file__), "--child", s[0], "--sizes", s[1], "--patches", s[2], "--nslots", str(a.nslots), "--pattern", pattern]
    return bl.drive("bench_rectify", steps, cmd, a.out, a.timeout)


if __name__ == "__main__":
    sys.exit(main())
