#!/usr/bin/env python3
"""Rates of the code rectifier (rd_rectifier_create_code): one JSON line per configuration, appended to profiles/code_bench.jsonl (--out).

On a synthetic frame's own rectangles (the rectangle detector's list for frame 0 of the stream, device frames), --patch x --patch patches at oversampling
--oversample, a 6 x 6 payload in one ring, inset 2:
  * "rates":   the latency of one job (enqueue to wait, nothing else on the device) and jobs/s with the jobs kept in flight, for
                 gray               the tensor job { U8, NHWC, GRAY, m } into device memory: the code job's first launch on its own, the figure to judge the others by;
                 code-dN            the code job with a dictionary of N = 0, 64, 1024 and 4096 codes;
                 grade-c4-hist      the grade job: the other record-writing two-launch job;
                 gray-pinned-host   the gray job read back to pinned host memory and decoded there by the restatement of the contract (tests/code.py: numpy and
                                    Python integers, dictionary of 64) - what a caller pays who decodes on the host with the tools at hand; its job count is lower,
                                    because it takes milliseconds;
                 gray-pinned        the same without the decoding: the read-back alone;
               the configurations ALTERNATE within one process, --rounds times, and a line holds the median over the rounds of each round's median latency and
               the difference from "gray" of the same run: what the second launch and the new kernel cost.
  * "kernels": the launches apart: the rates child's jobs once more under rocprofv3 --kernel-trace (csv) and per kernel and configuration the median of its
               durations in the trace.  Left out, with a message, where rocprofv3 is not installed.
  * "loop":    the rectangle detector's frames/s (64 slots, post-process on a worker thread, frames resident in HBM - the loop bench.py times) without a
               rectifier and with the code rectifier { dictionary of 1024 } behind every poll; the two alternate --repeat times in one process, a new detector
               per run.  The FIRST detector of a process runs faster than every later one ("Rectified patches"): compare runs 1 and later.
Every GPU step is a child process in a process group of its own under a time limit of its own, at which the whole group is killed (the tracer's child too); the tool
stops at the first step that fails.  bench.py is not involved.

    python tools/bench_code.py [--size 1920x1080] [--patch 128] [--oversample 1] [--steps rates,kernels,loop] [--rounds R] [--repeat R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tools import benchlib as bl

NJOBS = 4
NDICTS = (0, 64, 1024, 4096)
SLOW = ("gray-pinned-host",)      # configurations timed over fewer jobs


def code_spec(m):
    import rectdetect_amd as ra
    return ra.code_spec(6, 1, 2, oversample=m, contrast=16, max_border=2, max_hamming=4)


def dictionary(nd):
    """nd codes; what they are does not change the work (min_dist 0 accepts every candidate)"""
    import rectdetect_amd as ra
    return ra.code_dictionary(6, nd, 0, seed=11, tries=nd) if nd else None


def child_rates(iw, ih, p, m, rounds, trace_only):
    from tests import code as restated
    ra = bl.require_gpu("bench_code")
    L = ra.lib()
    frame, quads, dframe = bl.own_frame("bench_code", iw, ih, 64)
    n = len(quads)
    spec = code_spec(m)
    gray = lambda: ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, m))
    rects = {"gray": gray()}
    for nd in NDICTS:
        rects["code-d%d" % nd] = ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, code=spec, dictionary=dictionary(nd))
    rects["grade-c4-hist"] = ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, grade=ra.grade_spec(4, oversample=m, hist=True))
    rects["gray-pinned"] = gray()
    if not trace_only:
        rects["gray-pinned-host"] = gray()
    most = max(r.patch_bytes for r in rects.values())
    ptrs = [L.rd_device_alloc(n * most) for _ in range(NJOBS)]
    pins = [L.rd_host_alloc(n * p * p) for _ in range(NJOBS)]
    d64 = dictionary(64)
    pinned = lambda name: name.startswith("gray-pinned")

    def job(name, k):
        rects[name].enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, pins[k % NJOBS] if pinned(name) else ptrs[k % NJOBS], on_device=True, out_pinned=pinned(name))

    def done(name, k):
        status = rects[name].wait()
        if name == "gray-pinned-host":
            planes = np.ctypeslib.as_array((ctypes.c_uint8 * (n * p * p)).from_address(pins[k % NJOBS])).reshape(n, p, p)
            return restated.from_planes(planes, status, spec, d64)

    if not trace_only:      # the host's decoder computes what the job computes: compare once
        job("gray-pinned-host", 0)
        host = done("gray-pinned-host", 0)
        check = ra.Rectifier(p, p, max_quads=n, njobs=1, code=spec, dictionary=d64)
        mine = check.rectify(frame, quads)
        check.close()
        if not np.array_equal(host, mine):
            raise SystemExit("bench_code: the host's decoder and the code job disagree")

    # (under the tracer the warm-up is all there is)
    lat, rate = bl.alternating_rounds(rects, job, done, 0 if trace_only else rounds, NJOBS, (100 if trace_only else 32, 100, 400), slow=SLOW, slow_counts=(3, 5, 8))
    if not trace_only:
        base = float(np.median(lat["gray"]))
        for name in rects:
            print(json.dumps({"step": "rates", "config": name, "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "oversample": m, "quads_per_job": n, "jobs_in_flight": NJOBS, "rounds": rounds,
                              "bytes_per_quad": rects[name].patch_bytes, **bl.round_fields(lat[name]), "over_the_gray_job_us": round(float(np.median(lat[name])) - base, 1),
                              "jobs_per_s_median": round(float(np.median(rate[name])), 1), "quads_per_s_median": round(float(np.median(rate[name])) * n, 1), "frames": "device",
                              "output": "pinned" if pinned(name) else "device"}), flush=True)
    for rect in rects.values():
        rect.close()
    bl.free(ptrs + [dframe])
    for q in pins:
        L.rd_host_free(q)


def step_kernels(a, timeout):
    """the rates child under the tracer: the JSON lines as text, or None where there is no tracer.  The code kernel's launches come in the order of the
    configurations, 100 each: the trace is cut into those runs"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "trace", "--size", a.size, "--patch", str(a.patch), "--oversample", str(a.oversample)]
    durations = bl.kernel_trace("bench_code", cmd, timeout, lambda name: "k_code" in name or "k_grade" in name or "k_rectify_tensor" in name)
    if durations is None:
        return None
    code = [v for short in list(durations) if "k_code" in short for v in durations.pop(short)]
    if len(code) != 100 * len(NDICTS):
        print("bench_code: %d launches of the code kernel in the trace, expected %d - not cut into configurations" % (len(code), 100 * len(NDICTS)), file=sys.stderr)
        return None
    for i, nd in enumerate(NDICTS):
        durations["k_code ndict %d" % nd] = code[100 * i:100 * (i + 1)]
    lines = []
    for key in sorted(durations):
        lines.append(json.dumps({"step": "kernels", "kernel": key, "size": a.size, "patch": "%dx%d" % (a.patch, a.patch), "oversample": a.oversample, **bl.kernel_fields(durations[key])}))
    return "".join(line + "\n" for line in lines)


def child_loop(iw, ih, p, m, nslots, pattern):
    ra = bl.require_gpu("bench_code")
    rects = {"code-d1024": ra.Rectifier(p, p, max_quads=64, njobs=NJOBS, code=code_spec(m), dictionary=dictionary(1024))}
    for r, which, frames, dt, tally in bl.rectify_polled_runs(iw, ih, nslots, pattern, rects):
        print(json.dumps({"step": "loop", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "oversample": m, "nslots": nslots, "rectify_polled": which, "run": r, "first_detector_of_process": r == 0,
                          "frames": frames, "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "quads_per_s": round(tally[2] / dt, 1), "frames_kind": "device", "output": "device"}), flush=True)
    rects["code-d1024"].close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--oversample", type=int, default=1)
    ap.add_argument("--steps", default="rates,kernels,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating configurations in the rates step")
    ap.add_argument("--repeat", type=int, default=2, help="rounds of (none, code-d1024) in the loop step")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "code_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    iw, ih = (int(v) for v in a.size.split("x"))
    if a.child:
        if a.child == "rates":
            child_rates(iw, ih, a.patch, a.oversample, a.rounds, False)
        elif a.child == "trace":
            child_rates(iw, ih, a.patch, a.oversample, 0, True)
        else:
            child_loop(iw, ih, a.patch, a.oversample, a.nslots, ["none", "code-d1024"] * a.repeat)
        return 0
    cmd = lambda step: [sys.executable, os.path.abspath(__file__), "--child", step, "--size", a.size, "--patch", str(a.patch), "--oversample", str(a.oversample), "--nslots", str(a.nslots),
                        "--rounds", str(a.rounds), "--repeat", str(a.repeat)]
    return bl.drive("bench_code", a.steps.split(","), cmd, a.out, a.timeout, traced={"kernels": lambda timeout: step_kernels(a, timeout)})


if __name__ == "__main__":
    sys.exit(main())
