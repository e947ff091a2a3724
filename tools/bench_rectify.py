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
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
NJOBS = 4


def synth_frames(iw, ih, n):
    import rectdetect_amd as ra
    out = []
    for t in range(n):
        a = np.empty((ih, iw, 3), np.uint8)
        ra.lib().rd_synth_frame(a.ctypes.data, iw, ih, iw * 3, 0x5EED0000, t, 1)
        out.append(a)
    return out


def random_quads(iw, ih, n, seed=1):
    """n strictly convex quads: a rectangle of about iw / 6 by iw / 8 with jittered corners, rotated by any angle, its centre anywhere in the frame"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 4, 2))
    for k in range(n):
        w, h = iw / 6.0 * rng.uniform(0.7, 1.3), iw / 8.0 * rng.uniform(0.7, 1.3)
        base = np.array([(-w, -h), (w, -h), (w, h), (-w, h)]) / 2 + rng.uniform(-0.08, 0.08, (4, 2)) * w
        th = rng.uniform(0, 2 * np.pi)
        rot = np.array([(np.cos(th), -np.sin(th)), (np.sin(th), np.cos(th))])
        out[k] = base @ rot.T + (rng.uniform(0, iw), rng.uniform(0, ih))
    return out


def child_rates(iw, ih, p):
    import rectdetect_amd as ra
    L = ra.lib()
    frame = synth_frames(iw, ih, 1)[0]
    dframe = L.rd_device_alloc(frame.nbytes)
    L.rd_upload(dframe, frame.ctypes.data, frame.nbytes)
    outs = [L.rd_device_alloc(32 * p * p * 3) for _ in range(NJOBS)]
    rect = ra.Rectifier(p, p, max_quads=32, njobs=NJOBS)
    allq = random_quads(iw, ih, 32)
    for nq in (1, 8, 32):
        quads = allq[:nq]
        assert all(ra.rectify_coefficients(q)[1] == 1 for q in quads)

        def job(k):
            rect.enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, outs[k % NJOBS], on_device=True)

        for k in range(64):      # warm-up
            job(k)
            rect.wait()
        lat = []
        for k in range(300):
            t = time.perf_counter()
            job(k)
            rect.wait()
            lat.append(time.perf_counter() - t)
        njobs_timed = 4000
        t = time.perf_counter()
        inflight = 0
        for k in range(njobs_timed):
            if inflight == NJOBS:
                rect.wait()
                inflight -= 1
            job(k)
            inflight += 1
        while inflight:
            rect.wait()
            inflight -= 1
        dt = time.perf_counter() - t
        lat = np.sort(np.array(lat)) * 1e6
        print(json.dumps({"step": "rates", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "quads_per_job": nq, "jobs_in_flight": NJOBS, "jobs": njobs_timed,
                          "patches_per_s": round(njobs_timed * nq / dt, 1), "jobs_per_s": round(njobs_timed / dt, 1), "megapixels_per_s": round(njobs_timed * nq * p * p / dt / 1e6, 1),
                          "job_latency_us_median": round(float(lat[len(lat) // 2]), 1), "job_latency_us_p10": round(float(lat[len(lat) // 10]), 1),
                          "job_latency_us_p90": round(float(lat[len(lat) * 9 // 10]), 1), "frames": "device", "output": "device"}), flush=True)
    rect.close()
    for q in outs + [dframe]:
        L.rd_device_free(q)


def child_loop(iw, ih, p, nslots, pattern):
    import rectdetect_amd as ra
    L = ra.lib()
    imgs = synth_frames(iw, ih, 16)
    dptrs = []
    for a in imgs:
        q = L.rd_device_alloc(a.nbytes)
        L.rd_upload(q, a.ctypes.data, a.nbytes)
        dptrs.append(q)
    frames = 1024 if iw * ih <= 1920 * 1080 else 256
    warmup = 128
    maxq = 64
    outs = [L.rd_device_alloc(maxq * p * p * 3) for _ in range(NJOBS)]
    rect = ra.Rectifier(p, p, max_quads=maxq, njobs=NJOBS)

    def run(det, n, rectify, tally):
        inflight = jobs = 0

        def poll():
            nonlocal jobs
            rects = det.poll(TAN36)
            tally[0] += len(rects)
            if rectify:
                if jobs == NJOBS:
                    rect.wait()
                    jobs -= 1
                det.rectify_polled(rect, ra.rect_quads(rects[:maxq]), outs[tally[1] % NJOBS])
                tally[1] += 1
                tally[2] += min(len(rects), maxq)      # (the quads handed over)
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

    for r, rectify in enumerate(pattern):
        det = ra.Detector(iw, ih, nslots=nslots, nworkers=1, aperture=TAN36)
        run(det, warmup, rectify, [0, 0, 0])
        tally = [0, 0, 0]
        t = time.perf_counter()
        run(det, frames, rectify, tally)      # (ends with every frame polled and every job waited for)
        dt = time.perf_counter() - t
        det.close()
        print(json.dumps({"step": "loop", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "nslots": nslots, "rectify_polled": rectify, "run": r, "first_detector_of_process": r == 0, "frames": frames,
                          "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "patches_per_s": round(tally[2] / dt, 1),
                          "frames_kind": "device", "output": "device"}), flush=True)
    rect.close()
    for q in outs + dptrs:
        L.rd_device_free(q)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default="1280x720,1920x1080,3840x2160")
    ap.add_argument("--patches", default="64,128,256")
    ap.add_argument("--steps", default="rates,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3, help="rounds of (without, with) in the loop step")
    ap.add_argument("--pattern", default=None, help="the loop step's runs in one process as 0 (without) / 1 (with rectify_polled), e.g. 0,0,1,0 (default: 0,1 --repeat times)")
    ap.add_argument("--timeout", type=int, default=150, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    pattern = a.pattern or ",".join(["0,1"] * a.repeat)
    if a.child:
        iw, ih = (int(v) for v in a.sizes.split("x"))
        import rectdetect_amd as ra
        if not ra.gpu_available():
            raise SystemExit("bench_rectify: no HIP device - nothing is measured without one")
        if a.child == "rates":
            child_rates(iw, ih, int(a.patches))
        else:
            child_loop(iw, ih, int(a.patches), a.nslots, [v == "1" for v in pattern.split(",")])
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for step in a.steps.split(","):
        for size in a.sizes.split(","):
            for p in a.patches.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--sizes", size, "--patches", p, "--nslots", str(a.nslots), "--pattern", pattern]
                try:
                    res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print("bench_rectify: step %s %s %s ran into its time limit of %d s - stopping" % (step, size, p, a.timeout), file=sys.stderr)
                    return 124
                text = res.stdout.decode()
                sys.stdout.write(text)
                sys.stdout.flush()
                if res.returncode != 0:
                    print("bench_rectify: step %s %s %s failed with status %d - stopping" % (step, size, p, res.returncode), file=sys.stderr)
                    return res.returncode if res.returncode > 0 else 1
                with open(a.out, "a") as f:
                    f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
