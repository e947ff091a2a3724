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
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tools import benchlib as bl
from tools.benchlib import TAN36

NJOBS = 4
IW, IH = 1920, 1080
P = 128
LOOP_MODES = ("none", "rectify", "annotate", "composite")
PROBE_MODES = ("composite_empty", "composite_cached")      # --pattern only: where the loop's loss goes


def timed_jobs(comp, job, label, extra):
    n = 4000
    lat, dt = bl.timed_jobs(job, lambda k: comp.wait(), NJOBS, 64, 300, n)
    print(json.dumps(dict({"step": "jobs", "job": label, "size": "%dx%d" % (IW, IH), "jobs_in_flight": NJOBS, "jobs": n, "us_per_job_in_flight": round(dt / n * 1e6, 2),
                           **bl.latency_fields(lat)}, **extra)), flush=True)


def child_jobs(kinds):
    import rectdetect_amd as ra
    from tests import pixfmt
    L = ra.lib()
    frame = bl.synth_frames(IW, IH, 1)[0]
    quads = bl.own_quads(frame)
    if len(quads) == 0:
        raise SystemExit("bench_composite: the synthetic frame has no rectangle")
    n = len(quads)
    fills = ra.comp_items(quads, colour=(16, 16, 16))
    pastes = ra.comp_items(quads, patch=np.arange(n))
    tiles = len(ra.composite_tiles(fills, IW, IH))
    comp = ra.Compositor(P, P, max_items=n, njobs=NJOBS)
    patches = np.random.default_rng(1).integers(0, 256, (n, P, P, 3), dtype=np.uint8)
    dpatches, dframe = bl.upload([patches, frame])
    dout = L.rd_device_alloc(frame.nbytes)
    (y, uv), _ = pixfmt.convert(frame, ra.PIX_NV12)
    y, uv = np.ascontiguousarray(y), np.ascontiguousarray(uv)
    src = bl.upload([y, uv])
    dst = [L.rd_device_alloc(y.nbytes), L.rd_device_alloc(uv.nbytes)]
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
    bl.free([dframe, dout, dpatches] + src + dst)


def child_loop(nslots, pattern):
    import rectdetect_amd as ra
    L = ra.lib()
    # a pool with a device frame of its own for EVERY frame of a run (16 images in turn, 7 GB): in place each frame is written into once, after its detection, and
    # never detected again, so the detector's work is the same in all four modes; and no frame in flight is ever written into
    frames, warmup = 1024, 128
    base = bl.synth_frames(IW, IH, 16)
    imgs = [base[k % 16] for k in range(frames + warmup)]
    dptrs = bl.upload(imgs)
    quads = bl.random_quads(IW, IH, 32)
    outs = [L.rd_device_alloc(32 * P * P * 3) for _ in range(NJOBS)]
    rect = ra.Rectifier(P, P, max_quads=32, njobs=NJOBS)
    an = ra.Annotator(max_prims=1024, njobs=NJOBS)
    comp = ra.Compositor(P, P, max_items=256, njobs=NJOBS)
    workers = {"rectify": rect, "annotate": an, "composite": comp, "composite_empty": comp, "composite_cached": comp}
    cache = {}      # composite_cached: the items of image k % 16 (the stream is the same 16 images in turn, and their rectangles the same every time)

    def enqueue(det, i):
        det.enqueue(dptrs[i], IW * 3, on_device=True)

    def run(det, mode, timed, tally):
        def behind(det, worker, rects, i, k):
            if mode == "rectify":
                det.rectify_polled(rect, quads, outs[k % NJOBS])
                return 0
            if mode == "annotate":
                prims = ra.annot_rects(rects[:170])
                det.annotate_polled(an, prims)
                return len(prims)
            image = i % 16
            if mode == "composite_cached" and image in cache:
                items = cache[image]
            else:
                items = ra.comp_items(ra.rect_quads(rects[:256]), colour=(16, 16, 16))
                cache.setdefault(image, items)
            det.composite_polled(comp, items[:0] if mode == "composite_empty" else items)
            return len(items)

        bl.detector_loop(det, frames if timed else warmup, nslots, enqueue, tally, first=warmup if timed else 0, worker=workers.get(mode), njobs=NJOBS, behind=behind)

    for r, mode, dt, tally in bl.detector_runs(pattern, lambda: ra.Detector(IW, IH, nslots=nslots, nworkers=1, aperture=TAN36), run):
        if mode in ("annotate", "composite", "composite_cached"):      # (the next run starts from the pool as it was uploaded)
            for q, a in zip(dptrs, imgs):
                L.rd_upload(q, a.ctypes.data, a.nbytes)
        print(json.dumps({"step": "loop", "size": "%dx%d" % (IW, IH), "nslots": nslots, "behind_the_poll": mode, "run": r, "first_detector_of_process": r == 0, "frames": frames,
                          "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "items_or_primitives_per_frame": round(tally[2] / frames, 1), "frames_kind": "device"}), flush=True)
    rect.close()
    an.close()
    comp.close()
    bl.free(outs + dptrs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", default="jobs,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=2, help="rounds of (none, rectify, annotate, composite) in the loop step")
    ap.add_argument("--pattern", default=None, help="the loop step's runs in one process, e.g. none,none,composite (default: all four --repeat times)")
    ap.add_argument("--kinds", default="fills,pastes", help="the jobs step's item kinds (a kernel trace of one kind: --child jobs --kinds fills)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "composite_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    pattern = a.pattern or ",".join([",".join(LOOP_MODES)] * a.repeat)
    if a.child:
        bl.require_gpu("bench_composite")
        if a.child == "jobs":
            child_jobs(a.kinds.split(","))
        else:
            modes = pattern.split(",")
            if any(m not in LOOP_MODES + PROBE_MODES for m in modes):
                raise SystemExit("bench_composite: --pattern takes %s" % ", ".join(LOOP_MODES + PROBE_MODES))
            child_loop(a.nslots, modes)
        return 0
    cmd = lambda step: [sys.executable, os.path.abspath(__file__), "--child", step, "--nslots", str(a.nslots), "--pattern", pattern, "--kinds", a.kinds]
    return bl.drive("bench_composite", a.steps.split(","), cmd, a.out, a.timeout)


if __name__ == "__main__":
    sys.exit(main())
