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
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tools import benchlib as bl

NJOBS = 4
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)      # per OUTPUT channel (R, G, B), in 0 .. 255 units


def spec_f16(m):
    import rectdetect_amd as ra
    return ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, m, scale=[1.0 / s for s in STD], bias=[-a / s for a, s in zip(MEAN, STD)])


def child_rates(iw, ih, p, rounds):
    import torch      # (bl.require_gpu imported it before the library: one HIP runtime in the process)
    import rectdetect_amd as ra
    L = ra.lib()
    frame, quads, dframe = bl.own_frame("bench_tensor", iw, ih, 64)
    n = len(quads)
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

    lat, rate = bl.alternating_rounds(configs, job, finish, rounds, NJOBS, (32, 100, 400))
    for name in configs:
        print(json.dumps({"step": "rates", "config": name, "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "quads_per_job": n, "jobs_in_flight": NJOBS, "rounds": rounds,
                          **bl.round_fields(lat[name]), "jobs_per_s_median": round(float(np.median(rate[name])), 1), "patches_per_s_median": round(float(np.median(rate[name])) * n, 1),
                          "frames": "device", "output": "device"}), flush=True)
    for name, (rect, outs, ptrs) in configs.items():
        rect.close()
        if outs is None:
            bl.free(ptrs)
    bl.free([dframe])


def child_loop(iw, ih, p, nslots, pattern):
    import rectdetect_amd as ra
    rects = {"u8": ra.Rectifier(p, p, max_quads=64, njobs=NJOBS), "f16": ra.Rectifier(p, p, max_quads=64, njobs=NJOBS, tensor=spec_f16(1))}
    for r, which, frames, dt, tally in bl.rectify_polled_runs(iw, ih, nslots, pattern, rects):
        print(json.dumps({"step": "loop", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "nslots": nslots, "rectify_polled": which, "run": r, "first_detector_of_process": r == 0,
                          "frames": frames, "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "patches_per_s": round(tally[2] / dt, 1), "frames_kind": "device", "output": "device"}), flush=True)
    for rect in rects.values():
        rect.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--steps", default="rates,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating configurations in the rates step")
    ap.add_argument("--repeat", type=int, default=2, help="rounds of (none, u8, f16) in the loop step")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "tensor_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    iw, ih = (int(v) for v in a.size.split("x"))
    if a.child:
        bl.require_gpu("bench_tensor", torch_first=a.child == "rates")
        if a.child == "rates":
            child_rates(iw, ih, a.patch, a.rounds)
        else:
            child_loop(iw, ih, a.patch, a.nslots, ["none", "u8", "f16"] * a.repeat)
        return 0
    cmd = lambda step: [sys.executable, os.path.abspath(__file__), "--child", step, "--size", a.size, "--patch", str(a.patch), "--nslots", str(a.nslots), "--rounds", str(a.rounds), "--repeat", str(a.repeat)]
    return bl.drive("bench_tensor", a.steps.split(","), cmd, a.out, a.timeout)


if __name__ == "__main__":
    sys.exit(main())
