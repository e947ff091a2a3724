#!/usr/bin/env python3
"""Rates of the scan rectifier (rd_rectifier_create_scan): one JSON line per configuration, appended to profiles/scan_bench.jsonl (--out).

On a synthetic frame's own rectangles (the rectangle detector's list for frame 0 of the stream, device frames, device output), --patch x --patch pages at
oversampling --oversample:
  * "rates":   the latency of one job (enqueue to wait, nothing else on the device) and jobs/s with the jobs kept in flight, for
                 gray               the tensor job { U8, NHWC, GRAY, m }: the scan job's first launch on its own, the figure to judge the others by;
                 flat/bilevel/bits-rR   the scan job in each mode at radius 8, 15 and 63;
               the configurations ALTERNATE within one process, --rounds times, and a line holds the median over the rounds of each round's median latency and
               the difference from "gray" of the same run: what the second launch and the new kernel cost.
  * "kernels": the two launches apart: the rates child's jobs once more under rocprofv3 --kernel-trace (csv), one run per radius, and per kernel the median
               of its durations in the trace.  Left out, with a message, where rocprofv3 is not installed.
  * "loop":    the rectangle detector's frames/s (64 slots, post-process on a worker thread, frames resident in HBM - the loop bench.py times) without a
               rectifier and with the scan rectifier { BITS, radius 15 } behind every poll; the two alternate --repeat times in one process, a new detector
               per run.  The FIRST detector of a process runs faster than every later one ("Rectified patches"): compare runs 1 and later.
Every GPU step is a child process in a process group of its own under a time limit of its own, at which the whole group is killed (the tracer's child too); the tool
stops at the first step that fails.  bench.py is not involved.

    python tools/bench_scan.py [--size 1920x1080] [--patch 128] [--oversample 1] [--steps rates,kernels,loop] [--rounds R] [--repeat R] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tools import benchlib as bl

NJOBS = 4
RADII = (8, 15, 63)
MODE_NAMES = ("flat", "bilevel", "bits")


def child_rates(iw, ih, p, m, rounds, radii, trace_only):
    ra = bl.require_gpu("bench_scan")
    frame, quads, dframe = bl.own_frame("bench_scan", iw, ih, 64)
    n = len(quads)
    configs = {"gray": ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, m))}
    for r in radii:
        for mode, mname in enumerate(MODE_NAMES):
            configs["%s-r%d" % (mname, r)] = ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, scan=ra.scan_spec(mode, r, oversample=m))
    ptrs = [ra.lib().rd_device_alloc(n * p * p) for _ in range(NJOBS)]

    def job(name, k):
        configs[name].enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, ptrs[k % NJOBS], on_device=True)

    def done(name, k):
        configs[name].wait()

    # (under the tracer the warm-up is all there is)
    lat, rate = bl.alternating_rounds(configs, job, done, 0 if trace_only else rounds, NJOBS, (100 if trace_only else 32, 100, 400))
    if not trace_only:
        gray = float(np.median(lat["gray"]))
        for name in configs:
            print(json.dumps({"step": "rates", "config": name, "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "oversample": m, "quads_per_job": n, "jobs_in_flight": NJOBS, "rounds": rounds,
                              **bl.round_fields(lat[name]), "over_the_gray_job_us": round(float(np.median(lat[name])) - gray, 1), "jobs_per_s_median": round(float(np.median(rate[name])), 1),
                              "pages_per_s_median": round(float(np.median(rate[name])) * n, 1), "frames": "device", "output": "device"}), flush=True)
    for rect in configs.values():
        rect.close()
    bl.free(ptrs + [dframe])


def step_kernels(a, timeout):
    """the rates child under the tracer, one run per radius: the JSON lines as text, or None where there is no tracer"""
    lines = []
    for r in RADII:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "trace", "--radius", str(r), "--size", a.size, "--patch", str(a.patch), "--oversample", str(a.oversample)]
        durations = bl.kernel_trace("bench_scan", cmd, timeout, lambda name: "k_scan" in name or "k_rectify_tensor" in name)
        if durations is None:
            return None
        for short in sorted(durations):
            lines.append(json.dumps({"step": "kernels", "kernel": short, "radius": r, "size": a.size, "patch": "%dx%d" % (a.patch, a.patch), "oversample": a.oversample,
                                     **bl.kernel_fields(durations[short])}))
    return "".join(line + "\n" for line in lines)


def child_loop(iw, ih, p, m, nslots, pattern):
    ra = bl.require_gpu("bench_scan")
    rects = {"bits-r15": ra.Rectifier(p, p, max_quads=64, njobs=NJOBS, scan=ra.scan_spec(ra.SCAN_BITS, 15, oversample=m))}
    for r, which, frames, dt, tally in bl.rectify_polled_runs(iw, ih, nslots, pattern, rects):
        print(json.dumps({"step": "loop", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "oversample": m, "nslots": nslots, "rectify_polled": which, "run": r, "first_detector_of_process": r == 0,
                          "frames": frames, "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "pages_per_s": round(tally[2] / dt, 1), "frames_kind": "device", "output": "device"}), flush=True)
    rects["bits-r15"].close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--oversample", type=int, default=1)
    ap.add_argument("--steps", default="rates,kernels,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating configurations in the rates step")
    ap.add_argument("--repeat", type=int, default=2, help="rounds of (none, bits-r15) in the loop step")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "scan_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--radius", type=int, default=15, help=argparse.SUPPRESS)
    a = ap.parse_args()
    iw, ih = (int(v) for v in a.size.split("x"))
    if a.child:
        if a.child == "rates":
            child_rates(iw, ih, a.patch, a.oversample, a.rounds, RADII, False)
        elif a.child == "trace":
            child_rates(iw, ih, a.patch, a.oversample, 0, (a.radius,), True)
        else:
            child_loop(iw, ih, a.patch, a.oversample, a.nslots, ["none", "bits-r15"] * a.repeat)
        return 0
    cmd = lambda step: [sys.executable, os.path.abspath(__file__), "--child", step, "--size", a.size, "--patch", str(a.patch), "--oversample", str(a.oversample), "--nslots", str(a.nslots),
                        "--rounds", str(a.rounds), "--repeat", str(a.repeat)]
    return bl.drive("bench_scan", a.steps.split(","), cmd, a.out, a.timeout, traced={"kernels": lambda timeout: step_kernels(a, timeout)})


if __name__ == "__main__":
    sys.exit(main())
