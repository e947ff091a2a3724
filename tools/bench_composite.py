#!/usr/bin/env python3
"""Rates of the compositor (rd_compositor, rd_detector_composite_polled) at 1920x1080: JSON lines, appended to profiles/composite_bench.jsonl (--out).

  * "jobs":  microseconds per job - the latency of one job (enqueue to wait, nothing else on the device) and the time per job with four of the compositor's jobs kept
             in flight - for the rectangles of a frame of the synthetic stream (about ten quads) as fills and as pastes of 128x128 patches, in BGR and NV12,
             (a) in place and (b) into another device frame;
  * "loop":  (c) the rectangle detector's frames/s (64 slots, post-process on worker threads, frames resident in HBM - the loop bench.py times) four ways in one
             process: nothing behind the poll, rectify_polled of 32 quads into 128x128 patches, annotate_polled of the frame's own rectangles in place, and
             composite_polled of fills of the frame's own rectangles in place.  The runs alternate --repeat times, a new detector per run, so each is the others'
             baseline on the same machine state (the first detector of a process runs faster than every later one: DESIGN.md, "Rectified patches"; every line says
             whether it was).  Two more runs exist for --pattern, to tell the host's share of the loss from the device's: composite_empty builds the items and
             enqueues an EMPTY job (the host's work and the event, nothing on the device), composite_cached takes the items from a cache per image (no Python helper
             per frame; the device's work as in composite).  Every frame of a run has a device buffer of its own, so a frame written into in place is never detected again and the detector's work
             is the same in all four ("rectangles" shows it); the pool is uploaded afresh after every in-place run.
Every GPU step is a child process under a time limit of its own; the tool stops at the first one that fails.  bench.py is not involved.

    python tools/bench_composite.py [--steps jobs,loop] [--repeat R] [--out FILE]
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

from tools.bench_rectify import random_quads, synth_frames

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
NJOBS = 4
IW, IH = 1920, 1080
P = 128
LOOP_MODES = ("none", "rectify", "annotate", "composite")
PROBE_MODES = ("composite_empty", "composite_cached")      # --pattern only: where the loop's loss goes


def timed_jobs(comp, job, label, extra):
    for k in range(64):      # warm-up
        job(k)
        comp.wait()
    lat = []
    for k in range(300):
        t = time.perf_counter()
        job(k)
        comp.wait()
        lat.append(time.perf_counter() - t)
    n = 4000
    t = time.perf_counter()
    inflight = 0
    for k in range(n):
        if inflight == NJOBS:
            comp.wait()
            inflight -= 1
        job(k)
        inflight += 1
    while inflight:
        comp.wait()
        inflight -= 1
    dt = time.perf_counter() - t
    lat = np.sort(np.array(lat)) * 1e6
    print(json.dumps(dict({"step": "jobs", "job": label, "size": "%dx%d" % (IW, IH), "jobs_in_flight": NJOBS, "jobs": n, "us_per_job_in_flight": round(dt / n * 1e6, 2),
                           "job_latency_us_median": round(float(lat[len(lat) // 2]), 1), "job_latency_us_p10": round(float(lat[len(lat) // 10]), 1),
                           "job_latency_us_p90": round(float(lat[len(lat) * 9 // 10]), 1)}, **extra)), flush=True)


def child_jobs(kinds):
    import rectdetect_amd as ra
    from tests import pixfmt
    L = ra.lib()
    frame = synth_frames(IW, IH, 1)[0]
    det = ra.Detector(IW, IH, nslots=1, aperture=TAN36)
    det.enqueue(frame)
    quads = ra.rect_quads(det.poll(TAN36))
    det.close()
    if len(quads) == 0:
        raise SystemExit("bench_composite: the synthetic frame has no rectangle")
    n = len(quads)
    fills = ra.comp_items(quads, colour=(16, 16, 16))
    pastes = ra.comp_items(quads, patch=np.arange(n))
    tiles = len(ra.composite_tiles(fills, IW, IH))
    comp = ra.Compositor(P, P, max_items=n, njobs=NJOBS)
    patches = np.random.default_rng(1).integers(0, 256, (n, P, P, 3), dtype=np.uint8)
    dpatches = L.rd_device_alloc(patches.nbytes)
    L.rd_upload(dpatches, patches.ctypes.data, patches.nbytes)
    dframe, dout = L.rd_device_alloc(frame.nbytes), L.rd_device_alloc(frame.nbytes)
    L.rd_upload(dframe, frame.ctypes.data, frame.nbytes)
    (y, uv), _ = pixfmt.convert(frame, ra.PIX_NV12)
    y, uv = np.ascontiguousarray(y), np.ascontiguousarray(uv)
    src = [L.rd_device_alloc(y.nbytes), L.rd_device_alloc(uv.nbytes)]
    dst = [L.rd_device_alloc(y.nbytes), L.rd_device_alloc(uv.nbytes)]
    L.rd_upload(src[0], y.ctypes.data, y.nbytes)
    L.rd_upload(src[1], uv.ctypes.data, uv.nbytes)
    for what, items, pk in (("fills", fills, {}), ("pastes of 128x128 patches", pastes, {"patches": (dpatches, n), "patches_on_device": True})):
        if what.split()[0] not in kinds:
            continue
        extra = {"items": n, "tiles_launched": tiles, "kind": what}
        timed_jobs(comp, lambda k: comp.enqueue(ra.PIX_BGR, (dframe,), (IW * 3,), IW, IH, items, on_device=True, **pk), "a: %s, BGR in place" % what,
                   dict(extra, format="BGR", frames="device, in place"))
        timed_jobs(comp, lambda k: comp.enqueue(ra.PIX_NV12, src, (IW, IW), IW, IH, items, on_device=True, **pk), "a: %s, NV12 in place" % what,
                   dict(extra, format="NV12", frames="device, in place"))
        timed_jobs(comp, lambda k: comp.enqueue(ra.PIX_BGR, (dframe,), (IW * 3,), IW, IH, items, out_planes=(dout,), out_pitches=(IW * 3,), on_device=True, **pk),
                   "b: %s, BGR device to device" % what, dict(extra, format="BGR", frames="device to device"))
        timed_jobs(comp, lambda k: comp.enqueue(ra.PIX_NV12, src, (IW, IW), IW, IH, items, out_planes=dst, out_pitches=(IW, IW), on_device=True, **pk),
                   "b: %s, NV12 device to device" % what, dict(extra, format="NV12", frames="device to device"))
    comp.close()
    for q in [dframe, dout, dpatches] + src + dst:
        L.rd_device_free(q)


def child_loop(nslots, pattern):
    import rectdetect_amd as ra
    L = ra.lib()
    # a pool with a device frame of its own for EVERY frame of a run (16 images in turn, 7 GB): in place each frame is written into once, after its detection, and
    # never detected again, so the detector's work is the same in all four modes; and no frame in flight is ever written into
    frames, warmup = 1024, 128
    base = synth_frames(IW, IH, 16)
    imgs = [base[k % 16] for k in range(frames + warmup)]
    dptrs = []
    for a in imgs:
        q = L.rd_device_alloc(a.nbytes)
        L.rd_upload(q, a.ctypes.data, a.nbytes)
        dptrs.append(q)
    quads = random_quads(IW, IH, 32)
    outs = [L.rd_device_alloc(32 * P * P * 3) for _ in range(NJOBS)]
    rect = ra.Rectifier(P, P, max_quads=32, njobs=NJOBS)
    an = ra.Annotator(max_prims=1024, njobs=NJOBS)
    comp = ra.Compositor(P, P, max_items=256, njobs=NJOBS)
    workers = {"rectify": rect, "annotate": an, "composite": comp, "composite_empty": comp, "composite_cached": comp}
    cache = {}      # composite_cached: the items of image k % 16 (the stream is the same 16 images in turn, and their rectangles the same every time)

    def run(det, first, n, mode, tally):
        inflight = jobs = 0
        worker = workers.get(mode)
        polled = first

        def poll():
            nonlocal jobs, polled
            rects = det.poll(TAN36)
            tally[0] += len(rects)
            image = polled % 16
            polled += 1
            if mode == "none":
                return
            if jobs == NJOBS:
                worker.wait()
                jobs -= 1
            if mode == "rectify":
                det.rectify_polled(rect, quads, outs[tally[1] % NJOBS])
            elif mode == "annotate":
                prims = ra.annot_rects(rects[:170])
                tally[2] += len(prims)
                det.annotate_polled(an, prims)
            else:
                if mode == "composite_cached" and image in cache:
                    items = cache[image]
                else:
                    items = ra.comp_items(ra.rect_quads(rects[:256]), colour=(16, 16, 16))
                    cache.setdefault(image, items)
                tally[2] += len(items)
                det.composite_polled(comp, items[:0] if mode == "composite_empty" else items)
            tally[1] += 1
            jobs += 1

        for i in range(n):
            if inflight == nslots:
                poll()
                inflight -= 1
            det.enqueue(dptrs[first + i], IW * 3, on_device=True)
            inflight += 1
        while inflight:
            poll()
            inflight -= 1
        while jobs:
            worker.wait()
            jobs -= 1

    for r, mode in enumerate(pattern):
        det = ra.Detector(IW, IH, nslots=nslots, nworkers=1, aperture=TAN36)
        run(det, 0, warmup, mode, [0, 0, 0])
        tally = [0, 0, 0]
        t = time.perf_counter()
        run(det, warmup, frames, mode, tally)      # (ends with every frame polled and every job waited for)
        dt = time.perf_counter() - t
        det.close()
        if mode in ("annotate", "composite", "composite_cached"):      # (the next run starts from the pool as it was uploaded)
            for q, a in zip(dptrs, imgs):
                L.rd_upload(q, a.ctypes.data, a.nbytes)
        print(json.dumps({"step": "loop", "size": "%dx%d" % (IW, IH), "nslots": nslots, "behind_the_poll": mode, "run": r, "first_detector_of_process": r == 0, "frames": frames,
                          "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "items_or_primitives_per_frame": round(tally[2] / frames, 1), "frames_kind": "device"}), flush=True)
    rect.close()
    an.close()
    comp.close()
    for q in outs + dptrs:
        L.rd_device_free(q)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", default="jobs,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=2, help="rounds of (none, rectify, annotate, composite) in the loop step")
    ap.add_argument("--pattern", default=None, help="the loop step's runs in one process, e.g. none,none,composite (default: all four --repeat times)")
    ap.add_argument("--kinds", default="fills,pastes", help="the jobs step's item kinds (a kernel trace of one kind: --child jobs --kinds fills)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    pattern = a.pattern or ",".join([",".join(LOOP_MODES)] * a.repeat)
    if a.child:
        import rectdetect_amd as ra
        if not ra.gpu_available():
            raise SystemExit("bench_composite: no HIP device - nothing is measured without one")
        if a.child == "jobs":
            child_jobs(a.kinds.split(","))
        else:
            modes = pattern.split(",")
            if any(m not in LOOP_MODES + PROBE_MODES for m in modes):
                raise SystemExit("bench_composite: --pattern takes %s" % ", ".join(LOOP_MODES + PROBE_MODES))
            child_loop(a.nslots, modes)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--nslots", str(a.nslots), "--pattern", pattern, "--kinds", a.kinds]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print("bench_composite: step %s ran into its time limit of %d s - stopping" % (step, a.timeout), file=sys.stderr)
            return 124
        text = res.stdout.decode()
        sys.stdout.write(text)
        sys.stdout.flush()
        if res.returncode != 0:
            print("bench_composite: step %s failed with status %d - stopping" % (step, res.returncode), file=sys.stderr)
            return res.returncode if res.returncode > 0 else 1
        with open(a.out, "a") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
