#!/usr/bin/env python3
"""What the remapper (rd_remapper) costs: one JSON line per measurement, appended to profiles/remap_bench.jsonl (--out).

At 1920x1080 -> 1920x1080 with k1 = -0.1 (fx = fy = 1000, the principal point at the centre; the view takes the lens's fx, fy, cx, cy), device frames, device output:
  * "latency": the latency of one job (enqueue to wait, a host clock around work that ends in a synchronise, nothing else on the device) from a BGR and from an NV12
               frame, and - measured the same way, in the same process, in alternating rounds - of a device-to-device copy of as many bytes as the kernel's
               traffic names (the table's bytes + 2 frames' bytes) and of half as many (a copy READS and WRITES its bytes, so this one moves the kernel's
               traffic); the copies' device time from events as well.  The yardstick for "bound by its traffic".
  * "kernel":  the same three kinds of work alternating under `rocprofv3 --kernel-trace` (a run of its own: tracing slows the host), and from its database the
               duration of every launch of k_remap<BGR>, k_remap<NV12> and the copy's kernel: median, 10th and 90th percentile.
  * "loop":    the rectangle detector's frames/s (64 slots, post-process on worker threads - the loop bench.py times) with a remap job ahead of every enqueue
               (--njobs jobs in flight, the remap of the frames ahead running while the host polls), next to the same loop fed the SAME remapped frames made
               beforehand; the two alternate --repeat times in one process, a new detector per run.  The first detector of a process runs faster than every
               later one ("Rectified patches"): compare runs 1 and later.
Every GPU step is a child process in a process group of its own under a time limit of its own, at which the whole group is killed (the tracer's child too); the tool
stops at the first step that fails.  bench.py is not involved.

    python tools/bench_remap.py [--steps latency,kernel,loop] [--repeat R] [--njobs J] [--out FILE] [--trace-dir DIR]
"""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tools import benchlib as bl

IW, IH = 1920, 1080
PITCH = IW * 3
K1, F = -0.1, 1000.0
FORMATS = ("BGR", "NV12")


def cameras():
    import rectdetect_amd as ra
    lens = ra.lens(F, F, (IW - 1) / 2, (IH - 1) / 2, k1=K1)
    return lens, ra.view(F, F, (IW - 1) / 2, (IH - 1) / 2)


def nv12_of(bgr):
    """any NV12 frame of the picture will do for a timing: BT.601 luma, chroma of the top left pixel of each 2x2"""
    b, g, r = (bgr[..., k].astype(np.int32) for k in range(3))
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    uv = np.stack([u[0::2, 0::2], v[0::2, 0::2]], axis=-1).reshape(IH // 2, IW)
    return np.clip(y, 0, 255).astype(np.uint8), np.clip(uv, 0, 255).astype(np.uint8)


def traffic_bytes():
    """what one job moves by the count of the kernel's design: 8 bytes of table per output pixel, the BGR source frame once, the output frame"""
    return IW * IH * 8 + 2 * IW * IH * 3


def pct(us):
    a = np.sort(np.asarray(us, np.float64))
    return {"median_us": round(float(a[len(a) // 2]), 2), "p10_us": round(float(a[len(a) // 10]), 2), "p90_us": round(float(a[len(a) * 9 // 10]), 2), "n": len(a)}


class Work:
    """the three kinds of work on one device: a remap job from a BGR frame, one from an NV12 frame, a device-to-device copy"""

    def __init__(self, njobs):
        import torch
        import rectdetect_amd as ra
        self.ra, self.torch = ra, torch
        frame = bl.synth_frames(IW, IH, 1)[0]
        y, uv = nv12_of(frame)
        dev = torch.device("cuda:0")
        self.bgr, self.y, self.uv = (torch.from_numpy(a).to(dev) for a in (frame, y, uv))
        self.out = torch.empty((IH, IW, 3), dtype=torch.uint8, device=dev)
        n = traffic_bytes()
        self.src_full, self.dst_full = torch.zeros(n // 4, dtype=torch.int32, device=dev), torch.empty(n // 4, dtype=torch.int32, device=dev)
        self.src_half, self.dst_half = self.src_full[:n // 8], self.dst_full[:n // 8]
        lens, view = cameras()
        self.remapper = ra.Remapper(IW, IH, IW, IH, lens=lens, view=view, njobs=njobs)
        torch.cuda.synchronize()

    def job(self, fmt):
        ra = self.ra
        if fmt == "BGR":
            self.remapper.enqueue(ra.PIX_BGR, (self.bgr.data_ptr(),), (PITCH,), True, self.out.data_ptr(), PITCH)
        else:
            self.remapper.enqueue(ra.PIX_NV12, (self.y.data_ptr(), self.uv.data_ptr()), (IW, IW), True, self.out.data_ptr(), PITCH)
        self.remapper.wait()

    def copy(self, half):
        (self.dst_half if half else self.dst_full).copy_(self.src_half if half else self.src_full)
        self.torch.cuda.synchronize()

    def copy_kernel(self, half):
        """the same bytes through an element-wise kernel, which a kernel trace names (a plain copy_ may run on a copy engine or as a blit the trace files elsewhere)"""
        self.torch.add(self.src_half if half else self.src_full, 0, out=self.dst_half if half else self.dst_full)
        self.torch.cuda.synchronize()


def child_latency(njobs):
    w = Work(njobs)
    torch = w.torch
    kinds = [("remap", f) for f in FORMATS] + [("copy", False), ("copy", True), ("copy_kernel", False), ("copy_kernel", True)]
    run = lambda k, a: w.job(a) if k == "remap" else (w.copy(a) if k == "copy" else w.copy_kernel(a))
    for k, a in kinds:      # warm-up of every shape the timed window uses
        for _ in range(50):
            run(k, a)
    lat = {ka: [] for ka in kinds}
    dev = {ka: [] for ka in kinds if ka[0] != "remap"}
    for _ in range(8):      # alternating rounds
        for ka in kinds:
            for _ in range(50):
                t = time.perf_counter()
                run(*ka)
                lat[ka].append((time.perf_counter() - t) * 1e6)
            if ka in dev:      # device time of 50 back to back, from events
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                src, dst = (w.src_half, w.dst_half) if ka[1] else (w.src_full, w.dst_full)
                e0.record()
                for _ in range(50):
                    if ka[0] == "copy":
                        dst.copy_(src)
                    else:
                        torch.add(src, 0, out=dst)
                e1.record()
                torch.cuda.synchronize()
                dev[ka].append(e0.elapsed_time(e1) * 1e3 / 50)
    n = traffic_bytes()
    for (k, a), v in lat.items():
        rec = {"step": "latency", "size": "%dx%d" % (IW, IH), "k1": K1, "work": k}
        if k == "remap":
            rec.update(format=a, frames="device", output="device", bytes_by_design=n, table_bytes=IW * IH * 8, inside=w.remapper.inside)
        else:
            rec.update(bytes_copied=n // 2 if a else n, bytes_moved=n if a else 2 * n, device_us_per_copy_back_to_back=pct(dev[(k, a)])["median_us"])
        rec["latency"] = pct(v)
        print(json.dumps(rec), flush=True)
    w.remapper.close()


def child_kernel(njobs):
    """the work a kernel trace is taken of: rounds of one BGR job, one NV12 job, one copy kernel of each size"""
    w = Work(njobs)
    for _ in range(300):
        w.job("BGR")
        w.job("NV12")
        w.copy_kernel(True)
        w.copy_kernel(False)
    w.remapper.close()


def kernel_stats(db_path):
    """per kernel of the trace: the durations of the later four fifths of its launches"""
    db = sqlite3.connect(db_path)
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table' or type='view'")]
    kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    by = {}
    for s, e, name in db.execute(f"select d.start, d.end, s.kernel_name from {kd} d join {ks} s on d.kernel_id = s.id order by d.start"):
        by.setdefault(name, []).append((e - s) / 1e3)
    return {name: v[len(v) // 5:] for name, v in by.items() if len(v) >= 100}


def child_loop(nslots, njobs, pattern):
    import rectdetect_amd as ra
    L = ra.lib()
    lens, view = cameras()
    tan_aov = ra.view_tan_aov(view, IW)
    srcs = bl.upload(bl.synth_frames(IW, IH, 16))
    remapper = ra.Remapper(IW, IH, IW, IH, lens=lens, view=view, njobs=njobs)
    nout = nslots + njobs + 1      # a remapped frame stays until its poll returned, and njobs more are being made
    outs = [L.rd_device_alloc(IH * PITCH) for _ in range(nout)]
    ready = []      # the same frames remapped beforehand: what the loop without the remapper is fed
    for q in srcs:
        o = L.rd_device_alloc(IH * PITCH)
        remapper.enqueue(ra.PIX_BGR, (q,), (PITCH,), True, o, PITCH)
        remapper.wait()
        ready.append(o)
    frames, warmup = 1024, 128

    def run(det, remap, timed, tally):
        n = frames if timed else warmup
        inflight = 0
        feed = lambda i: remapper.enqueue(ra.PIX_BGR, (srcs[i % len(srcs)],), (PITCH,), True, outs[i % nout], PITCH)
        if remap:
            for i in range(min(njobs, n)):
                feed(i)
        for i in range(n):
            if inflight == nslots:
                tally[0] += len(det.poll(tan_aov))
                inflight -= 1
            if remap:
                remapper.wait()      # frame i is undistorted; the frames ahead of it are on their way
                if i + njobs < n:
                    feed(i + njobs)
            det.enqueue(outs[i % nout] if remap else ready[i % len(ready)], PITCH, on_device=True)
            inflight += 1
        while inflight:
            tally[0] += len(det.poll(tan_aov))
            inflight -= 1

    for r, remap, dt, tally in bl.detector_runs(pattern, lambda: ra.Detector(IW, IH, nslots=nslots, nworkers=1, aperture=tan_aov), run):
        print(json.dumps({"step": "loop", "size": "%dx%d" % (IW, IH), "k1": K1, "nslots": nslots, "remap_ahead_of_every_enqueue": remap, "remap_jobs_in_flight": njobs if remap else 0, "run": r,
                          "first_detector_of_process": r == 0, "frames": frames, "frames_per_s": round(frames / dt, 1), "us_per_frame": round(dt / frames * 1e6, 2), "rectangles": tally[0],
                          "frames_kind": "device"}), flush=True)
    remapper.close()
    bl.free(outs + srcs + ready)


def step_kernel(a, cmd, timeout):
    """the kernel child under the tracer, and from the tracer's database the duration of every launch: the JSON lines as text"""
    if a.trace_dir is None:
        a.trace_dir = tempfile.mkdtemp(prefix="remap_trace_")
    os.makedirs(a.trace_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "-d", a.trace_dir, "-o", "remap", "--"] + cmd
    rc, out, _ = bl.run_step(cmd, timeout)
    if rc != 0:
        sys.stdout.write(out.decode())
        raise subprocess.CalledProcessError(rc, cmd)
    dbs = sorted(glob.glob(os.path.join(a.trace_dir, "**", "*.db"), recursive=True), key=os.path.getmtime)
    if not dbs:
        print("bench_remap: the kernel trace left no database under %s" % a.trace_dir, file=sys.stderr)
        raise subprocess.CalledProcessError(1, cmd)
    return "".join(json.dumps({"step": "kernel", "size": "%dx%d" % (IW, IH), "k1": K1, "kernel": name, "bytes_by_design": traffic_bytes() if "k_remap" in name else None,
                               "duration": pct(v)}) + "\n" for name, v in sorted(kernel_stats(dbs[-1]).items()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", default="latency,kernel,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--njobs", type=int, default=4, help="remap jobs in flight in the loop step")
    ap.add_argument("--repeat", type=int, default=3, help="rounds of (without, with) in the loop step")
    ap.add_argument("--pattern", default=None, help="the loop step's runs in one process as 0 (without) / 1 (with the remapper), e.g. 0,0,1,0 (default: 0,1 --repeat times)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "remap_bench.jsonl"))
    ap.add_argument("--trace-dir", default=None, help="where the kernel step's trace goes (default: a new temporary directory)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    pattern = a.pattern or ",".join(["0,1"] * a.repeat)
    if a.child:
        bl.require_gpu("bench_remap", torch_first=a.child in ("latency", "kernel"))      # (torch before the library: one HIP runtime in the process)
        if a.child == "latency":
            child_latency(a.njobs)
        elif a.child == "kernel":
            child_kernel(a.njobs)
        else:
            child_loop(a.nslots, a.njobs, [v == "1" for v in pattern.split(",")])
        return 0
    cmd = lambda step: [sys.executable, os.path.abspath(__file__), "--child", step, "--nslots", str(a.nslots), "--njobs", str(a.njobs), "--pattern", pattern]
    return bl.drive("bench_remap", a.steps.split(","), cmd, a.out, a.timeout, traced={"kernel": lambda timeout: step_kernel(a, cmd("kernel"), timeout)})


if __name__ == "__main__":
    sys.exit(main())
