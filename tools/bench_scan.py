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
Every GPU step is a child process under a time limit of its own; the tool stops at the first one that fails.  bench.py is not involved.

    python tools/bench_scan.py [--size 1920x1080] [--patch 128] [--oversample 1] [--steps rates,kernels,loop] [--rounds R] [--repeat R] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
NJOBS = 4
RADII = (8, 15, 63)
MODE_NAMES = ("flat", "bilevel", "bits")


def synth_frames(iw, ih, n):
    import rectdetect_amd as ra
    out = []
    for t in range(n):
        a = np.empty((ih, iw, 3), np.uint8)
        ra.lib().rd_synth_frame(a.ctypes.data, iw, ih, iw * 3, 0x5EED0000, t, 1)
        out.append(a)
    return out


def own_quads(frame):
    """the quads of the frame's own rectangles"""
    import rectdetect_amd as ra
    ih, iw = frame.shape[:2]
    det = ra.Detector(iw, ih, nslots=1, aperture=TAN36)
    det.enqueue(frame)
    rects = det.poll(TAN36)
    det.close()
    return ra.rect_quads(rects)


def child_rates(iw, ih, p, m, rounds, radii, trace_only):
    import rectdetect_amd as ra
    if not ra.gpu_available():
        raise SystemExit("bench_scan: no HIP device - nothing is measured without one")
    L = ra.lib()
    frame = synth_frames(iw, ih, 1)[0]
    quads = own_quads(frame)[:64]
    n = len(quads)
    if n == 0:
        raise SystemExit("bench_scan: the synthetic frame holds no rectangle")
    dframe = L.rd_device_alloc(frame.nbytes)
    L.rd_upload(dframe, frame.ctypes.data, frame.nbytes)
    configs = {"gray": ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, m))}
    for r in radii:
        for mode, mname in enumerate(MODE_NAMES):
            configs["%s-r%d" % (mname, r)] = ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, scan=ra.scan_spec(mode, r, oversample=m))
    ptrs = [L.rd_device_alloc(n * p * p) for _ in range(NJOBS)]

    def job(name, k):
        configs[name].enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, ptrs[k % NJOBS], on_device=True)

    lat = {name: [] for name in configs}
    rate = {name: [] for name in configs}
    for name in configs:      # warm-up (under the tracer: all there is)
        for k in range(100 if trace_only else 32):
            job(name, k)
            configs[name].wait()
    for r in range(0 if trace_only else rounds):
        for name in configs:
            one = []
            for k in range(100):
                t = time.perf_counter()
                job(name, k)
                configs[name].wait()
                one.append(time.perf_counter() - t)
            lat[name].append(float(np.median(one)) * 1e6)
        for name in configs:
            njobs_timed, inflight = 400, 0
            t = time.perf_counter()
            for k in range(njobs_timed):
                if inflight == NJOBS:
                    configs[name].wait()
                    inflight -= 1
                job(name, k)
                inflight += 1
            while inflight:
                configs[name].wait()
                inflight -= 1
            rate[name].append(njobs_timed / (time.perf_counter() - t))
    if not trace_only:
        gray = float(np.median(lat["gray"]))
        for name in configs:
            med = float(np.median(lat[name]))
            print(json.dumps({"step": "rates", "config": name, "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "oversample": m, "quads_per_job": n, "jobs_in_flight": NJOBS, "rounds": rounds,
                              "job_latency_us_median": round(med, 1), "job_latency_us_min_round": round(min(lat[name]), 1), "job_latency_us_max_round": round(max(lat[name]), 1),
                              "over_the_gray_job_us": round(med - gray, 1), "jobs_per_s_median": round(float(np.median(rate[name])), 1),
                              "pages_per_s_median": round(float(np.median(rate[name])) * n, 1), "frames": "device", "output": "device"}), flush=True)
    for rect in configs.values():
        rect.close()
    for q in ptrs + [dframe]:
        L.rd_device_free(q)


def step_kernels(a, timeout):
    """the rates child under the tracer, one run per radius: the JSON lines as text, or None where there is no tracer"""
    if not shutil.which("rocprofv3"):
        print("bench_scan: rocprofv3 is not installed - the kernels step is left out", file=sys.stderr)
        return None
    lines = []
    for r in RADII:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "-o", "k", "--", sys.executable, os.path.abspath(__file__), "--child", "trace", "--radius", str(r), "--size", a.size, "--patch", str(a.patch),
                   "--oversample", str(a.oversample)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
            if res.returncode != 0:
                sys.stderr.write(res.stderr.decode()[-2000:])
                raise subprocess.CalledProcessError(res.returncode, cmd)
            durations = {}
            for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    name = row["Kernel_Name"]
                    if "k_scan" in name or "k_rectify_tensor" in name:
                        durations.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
            for name in sorted(durations):
                v = durations[name]
                short = name[name.index("k_"):].split("(")[0]
                lines.append(json.dumps({"step": "kernels", "kernel": short, "radius": r, "size": a.size, "patch": "%dx%d" % (a.patch, a.patch), "oversample": a.oversample, "launches": len(v),
                                         "kernel_us_median": round(float(np.median(v)), 2), "kernel_us_min": round(min(v), 2), "kernel_us_max": round(max(v), 2)}))
    return "".join(line + "\n" for line in lines)


def child_loop(iw, ih, p, m, nslots, pattern):
    import rectdetect_amd as ra
    if not ra.gpu_available():
        raise SystemExit("bench_scan: no HIP device - nothing is measured without one")
    L = ra.lib()
    imgs = synth_frames(iw, ih, 16)
    dptrs = []
    for a in imgs:
        q = L.rd_device_alloc(a.nbytes)
        L.rd_upload(q, a.ctypes.data, a.nbytes)
        dptrs.append(q)
    frames, warmup, maxq = 1024 if iw * ih <= 1920 * 1080 else 256, 128, 64
    rects = {"bits-r15": ra.Rectifier(p, p, max_quads=maxq, njobs=NJOBS, scan=ra.scan_spec(ra.SCAN_BITS, 15, oversample=m))}
    outs = [L.rd_device_alloc(maxq * max(r.patch_bytes for r in rects.values())) for _ in range(NJOBS)]

    def run(det, n, which, tally):
        inflight = jobs = 0
        rect = rects.get(which)

        def poll():
            nonlocal jobs
            found = det.poll(TAN36)
            tally[0] += len(found)
            if rect is not None:
                if jobs == NJOBS:
                    rect.wait()
                    jobs -= 1
                det.rectify_polled(rect, ra.rect_quads(found[:maxq]), outs[tally[1] % NJOBS])
                tally[1] += 1
                tally[2] += min(len(found), maxq)
                jobs += 1

        for i in range(n):
            if inflight == nslots:
                poll()
                inflight -= 1
            det.enqueue(dptrs[i % len(dptrs)], iw * 3, on_device=True)
            inflight += 1
        while inflight:
            poll()
            inflight -= 1
        while jobs:
            rect.wait()
            jobs -= 1

    for r, which in enumerate(pattern):
        det = ra.Detector(iw, ih, nslots=nslots, nworkers=1, aperture=TAN36)
        run(det, warmup, which, [0, 0, 0])
        tally = [0, 0, 0]
        t = time.perf_counter()
        run(det, frames, which, tally)      # (ends with every frame polled and every job waited for)
        dt = time.perf_counter() - t
        det.close()
        print(json.dumps({"step": "loop", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "oversample": m, "nslots": nslots, "rectify_polled": which, "run": r, "first_detector_of_process": r == 0,
                          "frames": frames, "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "pages_per_s": round(tally[2] / dt, 1), "frames_kind": "device", "output": "device"}), flush=True)
    for rect in rects.values():
        rect.close()
    for q in outs + dptrs:
        L.rd_device_free(q)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_bench.jsonl"))
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--size", a.size, "--patch", str(a.patch), "--oversample", str(a.oversample), "--nslots", str(a.nslots), "--rounds", str(a.rounds),
               "--repeat", str(a.repeat)]
        try:
            if step == "kernels":
                text = step_kernels(a, a.timeout)
                if text is None:
                    continue
            else:
                res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
                text = res.stdout.decode()
                if res.returncode != 0:
                    sys.stdout.write(text)
                    print("bench_scan: step %s failed with status %d - stopping" % (step, res.returncode), file=sys.stderr)
                    return res.returncode if res.returncode > 0 else 1
        except subprocess.TimeoutExpired:
            print("bench_scan: step %s ran into its time limit of %d s - stopping" % (step, a.timeout), file=sys.stderr)
            return 124
        except subprocess.CalledProcessError as e:
            print("bench_scan: step %s failed with status %d - stopping" % (step, e.returncode), file=sys.stderr)
            return e.returncode if e.returncode > 0 else 1
        sys.stdout.write(text)
        sys.stdout.flush()
        with open(a.out, "a") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
