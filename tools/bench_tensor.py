#!/usr/bin/env python3
"""Rates of the tensor rectifier (rd_rectifier_create_tensor): one JSON line per configuration, appended to profiles/tensor_bench.jsonl (--out).

On a synthetic frame's own rectangles (the rectangle detector's list for frame 0 of the stream, device frames, device output), --patch x --patch outputs:
  * "rates":  the latency of one job (enqueue to wait, nothing else on the device) and jobs/s with the jobs kept in flight, for
                classic      the u8 rectifier (rd_rectifier_create), today's figure;
                f16-m1/2/4   the tensor job { F16, NCHW, RGB, m } with a mean and a deviation per channel;
                torch        what a user does without it: the classic job into a torch uint8 tensor, then permute, float, sub, div and half in torch on the
                             device, synchronised;
              the configurations ALTERNATE within one process, --rounds times, and a line holds the median over the rounds of each round's median latency.
              torch is imported before the library is loaded, so that the process holds one HIP runtime.
  * "loop":   the rectangle detector's frames/s (64 slots, post-process on a worker thread, frames resident in HBM - the loop bench.py times) without a
              rectifier, with the u8 rectifier and with the tensor rectifier { F16, NCHW, RGB, 1 } behind every poll; the three alternate --repeat times in one
              process, a new detector per run.  The FIRST detector of a process runs faster than every later one ("Rectified patches"): compare runs
              1 and later.
Every GPU step is a child process under a time limit of its own; the tool stops at the first one that fails.  bench.py is not involved.

    python tools/bench_tensor.py [--size 1920x1080] [--patch 128] [--steps rates,loop] [--rounds R] [--repeat R] [--out FILE]
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
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)      # per OUTPUT channel (R, G, B), in 0 .. 255 units


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


def spec_f16(m):
    import rectdetect_amd as ra
    return ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, m, scale=[1.0 / s for s in STD], bias=[-a / s for a, s in zip(MEAN, STD)])


def child_rates(iw, ih, p, rounds):
    import torch      # before the library: one HIP runtime in the process
    import rectdetect_amd as ra
    L = ra.lib()
    frame = synth_frames(iw, ih, 1)[0]
    quads = own_quads(frame)[:64]
    n = len(quads)
    if n == 0:
        raise SystemExit("bench_tensor: the synthetic frame holds no rectangle")
    dframe = L.rd_device_alloc(frame.nbytes)
    L.rd_upload(dframe, frame.ctypes.data, frame.nbytes)
    mean = torch.tensor(MEAN, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    configs = {}
    for name, spec in (("classic", None), ("f16-m1", spec_f16(1)), ("f16-m2", spec_f16(2)), ("f16-m4", spec_f16(4)), ("torch", None)):
        rect = ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, tensor=spec)
        if name == "torch":
            outs = [torch.empty((n, p, p, 3), dtype=torch.uint8, device="cuda") for _ in range(NJOBS)]
            ptrs = [t.data_ptr() for t in outs]
        else:
            outs = None
            ptrs = [L.rd_device_alloc(n * rect.patch_bytes) for _ in range(NJOBS)]
        configs[name] = (rect, outs, ptrs)
    torch.cuda.synchronize()

    def job(name, k):
        rect, outs, ptrs = configs[name]
        rect.enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, ptrs[k % NJOBS], on_device=True)

    def finish(name, k):
        """the job's wait and, for "torch", the second pass over the patches: BGR -> RGB, HWC -> CHW, float, mean, deviation, half"""
        rect, outs, _ = configs[name]
        rect.wait()
        if outs is not None:
            t = outs[k % NJOBS].permute(0, 3, 1, 2).flip(1).float().sub(mean).div(std).half()
            torch.cuda.synchronize()
            return t

    lat = {name: [] for name in configs}
    rate = {name: [] for name in configs}
    for name in configs:      # warm-up
        for k in range(32):
            job(name, k)
            finish(name, k)
    for r in range(rounds):
        for name in configs:
            one = []
            for k in range(100):
                t = time.perf_counter()
                job(name, k)
                finish(name, k)
                one.append(time.perf_counter() - t)
            lat[name].append(float(np.median(one)) * 1e6)
        for name in configs:
            njobs_timed, inflight, first = 400, 0, 0
            t = time.perf_counter()
            for k in range(njobs_timed):
                if inflight == NJOBS:
                    finish(name, first)
                    first += 1
                    inflight -= 1
                job(name, k)
                inflight += 1
            while inflight:
                finish(name, first)
                first += 1
                inflight -= 1
            rate[name].append(njobs_timed / (time.perf_counter() - t))
    for name in configs:
        print(json.dumps({"step": "rates", "config": name, "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "quads_per_job": n, "jobs_in_flight": NJOBS, "rounds": rounds,
                          "job_latency_us_median": round(float(np.median(lat[name])), 1), "job_latency_us_min_round": round(min(lat[name]), 1), "job_latency_us_max_round": round(max(lat[name]), 1),
                          "jobs_per_s_median": round(float(np.median(rate[name])), 1), "patches_per_s_median": round(float(np.median(rate[name])) * n, 1),
                          "frames": "device", "output": "device"}), flush=True)
    for name, (rect, outs, ptrs) in configs.items():
        rect.close()
        if outs is None:
            for q in ptrs:
                L.rd_device_free(q)
    L.rd_device_free(dframe)


def child_loop(iw, ih, p, nslots, pattern):
    import rectdetect_amd as ra
    L = ra.lib()
    imgs = synth_frames(iw, ih, 16)
    dptrs = []
    for a in imgs:
        q = L.rd_device_alloc(a.nbytes)
        L.rd_upload(q, a.ctypes.data, a.nbytes)
        dptrs.append(q)
    frames, warmup, maxq = 1024 if iw * ih <= 1920 * 1080 else 256, 128, 64
    rects = {"u8": ra.Rectifier(p, p, max_quads=maxq, njobs=NJOBS), "f16": ra.Rectifier(p, p, max_quads=maxq, njobs=NJOBS, tensor=spec_f16(1))}
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
        print(json.dumps({"step": "loop", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "nslots": nslots, "rectify_polled": which, "run": r, "first_detector_of_process": r == 0,
                          "frames": frames, "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "patches_per_s": round(tally[2] / dt, 1), "frames_kind": "device", "output": "device"}), flush=True)
    for rect in rects.values():
        rect.close()
    for q in outs + dptrs:
        L.rd_device_free(q)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--steps", default="rates,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating configurations in the rates step")
    ap.add_argument("--repeat", type=int, default=2, help="rounds of (none, u8, f16) in the loop step")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    iw, ih = (int(v) for v in a.size.split("x"))
    if a.child:
        if a.child == "rates":
            child_rates(iw, ih, a.patch, a.rounds)
        else:
            import rectdetect_amd as ra
            if not ra.gpu_available():
                raise SystemExit("bench_tensor: no HIP device - nothing is measured without one")
            child_loop(iw, ih, a.patch, a.nslots, ["none", "u8", "f16"] * a.repeat)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--size", a.size, "--patch", str(a.patch), "--nslots", str(a.nslots), "--rounds", str(a.rounds), "--repeat", str(a.repeat)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print("bench_tensor: step %s ran into its time limit of %d s - stopping" % (step, a.timeout), file=sys.stderr)
            return 124
        text = res.stdout.decode()
        sys.stdout.write(text)
        sys.stdout.flush()
        if res.returncode != 0:
            print("bench_tensor: step %s failed with status %d - stopping" % (step, res.returncode), file=sys.stderr)
            return res.returncode if res.returncode > 0 else 1
        with open(a.out, "a") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
