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
import csv
import ctypes
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
NJOBS = 4
NDICTS = (0, 64, 1024, 4096)
SLOW = ("gray-pinned-host",)      # configurations timed over fewer jobs


def run_step(cmd, timeout, capture_stderr=False):
    """cmd in a process group of its own, the whole group killed at the time limit - under the tracer the GPU is open in a grandchild, which the death of its parent
    would not end: (return code, stdout, stderr or None); subprocess.TimeoutExpired once every process of the step is gone"""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE if capture_stderr else None, start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        p.communicate()
        raise
    return p.returncode, out, err


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


def code_spec(m):
    import rectdetect_amd as ra
    return ra.code_spec(6, 1, 2, oversample=m, contrast=16, max_border=2, max_hamming=4)


def dictionary(nd):
    """nd codes; what they are does not change the work (min_dist 0 accepts every candidate)"""
    import rectdetect_amd as ra
    return ra.code_dictionary(6, nd, 0, seed=11, tries=nd) if nd else None


def child_rates(iw, ih, p, m, rounds, trace_only):
    import rectdetect_amd as ra
    from tests import code as restated
    if not ra.gpu_available():
        raise SystemExit("bench_code: no HIP device - nothing is measured without one")
    L = ra.lib()
    frame = synth_frames(iw, ih, 1)[0]
    quads = own_quads(frame)[:64]
    n = len(quads)
    if n == 0:
        raise SystemExit("bench_code: the synthetic frame holds no rectangle")
    dframe = L.rd_device_alloc(frame.nbytes)
    L.rd_upload(dframe, frame.ctypes.data, frame.nbytes)
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

    lat = {name: [] for name in rects}
    rate = {name: [] for name in rects}
    for name in rects:      # warm-up (under the tracer: all there is)
        for k in range(3 if name in SLOW else (100 if trace_only else 32)):
            job(name, k)
            done(name, k)
    for r in range(0 if trace_only else rounds):
        for name in rects:
            one = []
            for k in range(5 if name in SLOW else 100):
                t = time.perf_counter()
                job(name, k)
                done(name, k)
                one.append(time.perf_counter() - t)
            lat[name].append(float(np.median(one)) * 1e6)
        for name in rects:
            njobs_timed, inflight = 8 if name in SLOW else 400, 0
            t = time.perf_counter()
            for k in range(njobs_timed):
                if inflight == NJOBS:
                    done(name, k - NJOBS)
                    inflight -= 1
                job(name, k)
                inflight += 1
            while inflight:
                done(name, njobs_timed - inflight)
                inflight -= 1
            rate[name].append(njobs_timed / (time.perf_counter() - t))
    if not trace_only:
        base = float(np.median(lat["gray"]))
        for name in rects:
            med = float(np.median(lat[name]))
            print(json.dumps({"step": "rates", "config": name, "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "oversample": m, "quads_per_job": n, "jobs_in_flight": NJOBS, "rounds": rounds,
                              "bytes_per_quad": rects[name].patch_bytes, "job_latency_us_median": round(med, 1), "job_latency_us_min_round": round(min(lat[name]), 1),
                              "job_latency_us_max_round": round(max(lat[name]), 1), "over_the_gray_job_us": round(med - base, 1), "jobs_per_s_median": round(float(np.median(rate[name])), 1),
                              "quads_per_s_median": round(float(np.median(rate[name])) * n, 1), "frames": "device", "output": "pinned" if pinned(name) else "device"}), flush=True)
    for rect in rects.values():
        rect.close()
    for q in ptrs + [dframe]:
        L.rd_device_free(q)
    for q in pins:
        L.rd_host_free(q)


def step_kernels(a, timeout):
    """the rates child under the tracer: the JSON lines as text, or None where there is no tracer.  The code kernel's launches come in the order of the
    configurations, 100 each: the trace is cut into those runs"""
    if not shutil.which("rocprofv3"):
        print("bench_code: rocprofv3 is not installed - the kernels step is left out", file=sys.stderr)
        return None
    lines = []
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "-o", "k", "--", sys.executable, os.path.abspath(__file__), "--child", "trace", "--size", a.size, "--patch", str(a.patch),
               "--oversample", str(a.oversample)]
        rc, _, err = run_step(cmd, timeout, capture_stderr=True)
        if rc != 0:
            sys.stderr.write(err.decode()[-2000:])
            raise subprocess.CalledProcessError(rc, cmd)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
        rows.sort(key=lambda row: int(row["Start_Timestamp"]))
        durations = {}
        ncode = 0
        for row in rows:
            name = row["Kernel_Name"]
            if "k_code" in name:
                key = "k_code ndict %d" % NDICTS[min(ncode // 100, len(NDICTS) - 1)]
                ncode += 1
            elif "k_grade" in name or "k_rectify_tensor" in name:
                key = name[name.index("k_"):].split("(")[0]
            else:
                continue
            durations.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
        if ncode != 100 * len(NDICTS):
            print("bench_code: %d launches of the code kernel in the trace, expected %d - not cut into configurations" % (ncode, 100 * len(NDICTS)), file=sys.stderr)
            return None
        for key in sorted(durations):
            v = durations[key]
            lines.append(json.dumps({"step": "kernels", "kernel": key, "size": a.size, "patch": "%dx%d" % (a.patch, a.patch), "oversample": a.oversample, "launches": len(v),
                                     "kernel_us_median": round(float(np.median(v)), 2), "kernel_us_min": round(min(v), 2), "kernel_us_max": round(max(v), 2)}))
    return "".join(line + "\n" for line in lines)


def child_loop(iw, ih, p, m, nslots, pattern):
    import rectdetect_amd as ra
    if not ra.gpu_available():
        raise SystemExit("bench_code: no HIP device - nothing is measured without one")
    L = ra.lib()
    imgs = synth_frames(iw, ih, 16)
    dptrs = []
    for a in imgs:
        q = L.rd_device_alloc(a.nbytes)
        L.rd_upload(q, a.ctypes.data, a.nbytes)
        dptrs.append(q)
    frames, warmup, maxq = 1024 if iw * ih <= 1920 * 1080 else 256, 128, 64
    rects = {"code-d1024": ra.Rectifier(p, p, max_quads=maxq, njobs=NJOBS, code=code_spec(m), dictionary=dictionary(1024))}
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
                          "frames": frames, "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "quads_per_s": round(tally[2] / dt, 1), "frames_kind": "device", "output": "device"}), flush=True)
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
    ap.add_argument("--repeat", type=int, default=2, help="rounds of (none, code-d1024) in the loop step")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "code_bench.jsonl"))
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
                rc, out, _ = run_step(cmd, a.timeout)
                text = out.decode()
                if rc != 0:
                    sys.stdout.write(text)
                    print("bench_code: step %s failed with status %d - stopping" % (step, rc), file=sys.stderr)
                    return rc if rc > 0 else 1
        except subprocess.TimeoutExpired:
            print("bench_code: step %s ran into its time limit of %d s - stopping" % (step, a.timeout), file=sys.stderr)
            return 124
        except subprocess.CalledProcessError as e:
            print("bench_code: step %s failed with status %d - stopping" % (step, e.returncode), file=sys.stderr)
            return e.returncode if e.returncode > 0 else 1
        sys.stdout.write(text)
        sys.stdout.flush()
        with open(a.out, "a") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
