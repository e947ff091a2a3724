#!/usr/bin/env python3
"""Rates of the grade rectifier (rd_rectifier_create_grade): one JSON line per configuration, appended to profiles/grade_bench.jsonl (--out).

On a synthetic frame's own rectangles (the rectangle detector's list for frame 0 of the stream, device frames), --patch x --patch patches at oversampling
--oversample:
  * "rates":   the latency of one job (enqueue to wait, nothing else on the device) and jobs/s with the jobs kept in flight, for
                 gray               the tensor job { U8, NHWC, GRAY, m } into device memory: the grade job's first launch on its own, the figure to judge the others by;
                 grade-cC[-hist]    the grade job at cells 1 and 8, without and with the histogram;
                 scan-bits-r8       the scan job { BITS, radius 8 }: the other two-launch job on the same grid;
                 gray-torch         the gray job into a torch tensor, then the same records and histogram by a chain of torch ops, synchronised (left out, with a
                                    message, where torch is not installed);
                 gray-pinned        the gray job read back to pinned host memory: what a caller pays who grades on the host (the host's arithmetic not included);
               the configurations ALTERNATE within one process, --rounds times, and a line holds the median over the rounds of each round's median latency and
               the difference from "gray" of the same run: what the second launch and the new kernel cost.
  * "kernels": the launches apart: the rates child's jobs once more under rocprofv3 --kernel-trace (csv) and per kernel the median of its durations in the
               trace; with --variant LIB the same run once more on that library (a timing-only build, tools/variants.sh: -DRD_GRADE_FLUSH=0 flushes from one tile
               per quad only - what the global atomics cost).  Left out, with a message, where rocprofv3 is not installed.
  * "loop":    the rectangle detector's frames/s (64 slots, post-process on a worker thread, frames resident in HBM - the loop bench.py times) without a
               rectifier and with the grade rectifier { cells 4, hist } behind every poll; the two alternate --repeat times in one process, a new detector
               per run.  The FIRST detector of a process runs faster than every later one ("Rectified patches"): compare runs 1 and later.
Every GPU step is a child process in a process group of its own under a time limit of its own, at which the whole group is killed (the tracer's child too); the tool
stops at the first step that fails.  bench.py is not involved.

    python tools/bench_grade.py [--size 1920x1080] [--patch 128] [--oversample 1] [--steps rates,kernels,loop] [--rounds R] [--repeat R] [--variant LIB] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tools import benchlib as bl

NJOBS = 4
GRADES = (("grade-c1", 1, False), ("grade-c8", 8, False), ("grade-c1-hist", 1, True), ("grade-c8-hist", 8, True))


def torch_records(torch, g, cells, dark, bright, edge):
    """the records and the histogram of (n, p, p) uint8 planes by torch ops: (an (n, cells, cells, 8) int64 tensor, an (n, 256) int64 tensor); p divisible by cells"""
    n, p = g.shape[0], g.shape[1]
    G = g.to(torch.int32)
    P = torch.nn.functional.pad(G.unsqueeze(1).float(), (1, 1, 1, 1), mode="replicate").squeeze(1).to(torch.int32)
    Lp = P[:, 1:-1, :-2] + P[:, 1:-1, 2:] + P[:, :-2, 1:-1] + P[:, 2:, 1:-1] - 4 * G
    G64, L64 = G.to(torch.int64), Lp.to(torch.int64)
    terms = torch.stack([torch.ones_like(G64), (G64 <= dark).to(torch.int64), (G64 >= bright).to(torch.int64), (L64.abs() >= edge).to(torch.int64), G64, G64 * G64, L64, L64 * L64], dim=-1)
    rec = terms.view(n, cells, p // cells, cells, p // cells, 8).sum(dim=(2, 4))
    hist = torch.bincount((G64.view(n, -1) + 256 * torch.arange(n, device=g.device).view(n, 1)).flatten(), minlength=256 * n).view(n, 256)
    return rec, hist


def child_rates(iw, ih, p, m, rounds, trace_only):
    torch = None
    if not trace_only:
        try:
            import torch      # first: the process then holds ONE HIP runtime, torch's
        except ImportError:
            print("bench_grade: torch is not installed - the gray-torch configuration is left out", file=sys.stderr)
    ra = bl.require_gpu("bench_grade", torch_first=torch is not None)
    L = ra.lib()
    frame, quads, dframe = bl.own_frame("bench_grade", iw, ih, 64)
    n = len(quads)
    gray = lambda: ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, m))
    rects = {"gray": gray()}
    for name, c, h in GRADES:
        rects[name] = ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, grade=ra.grade_spec(c, oversample=m, hist=h))
    rects["scan-bits-r8"] = ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, scan=ra.scan_spec(ra.SCAN_BITS, 8, oversample=m))
    rects["gray-pinned"] = gray()
    if torch is not None and p % 8 == 0:
        rects["gray-torch"] = gray()
        tens = [torch.empty((n, p, p), dtype=torch.uint8, device="cuda") for _ in range(NJOBS)]
        torch.cuda.synchronize()
    most = max(r.patch_bytes for r in rects.values())
    ptrs = [L.rd_device_alloc(n * most) for _ in range(NJOBS)]
    pins = [L.rd_host_alloc(n * p * p) for _ in range(NJOBS)]
    spec8 = ra.grade_spec(8)

    def job(name, k):
        out = pins[k % NJOBS] if name == "gray-pinned" else (tens[k % NJOBS].data_ptr() if name == "gray-torch" else ptrs[k % NJOBS])
        rects[name].enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, out, on_device=True, out_pinned=name == "gray-pinned")

    def done(name, k):
        rects[name].wait()
        if name == "gray-torch":      # (the job's wait made the plane visible to every stream)
            rec, hist = torch_records(torch, tens[k % NJOBS], 8, int(spec8["dark"]), int(spec8["bright"]), int(spec8["edge"]))
            torch.cuda.synchronize()

    if "gray-torch" in rects:      # the chain computes what the job computes: compare once
        job("gray-torch", 0)
        rects["gray-torch"].wait()
        rec, hist = torch_records(torch, tens[0], 8, int(spec8["dark"]), int(spec8["bright"]), int(spec8["edge"]))
        check = ra.Rectifier(p, p, max_quads=n, njobs=1, grade=ra.grade_spec(8, oversample=m, hist=True))
        cells, h = ra.grade_view(check.rectify(frame, quads), ra.grade_spec(8, hist=True))
        check.close()
        mine = np.stack([cells[f].astype(np.int64) for f in ("n", "lo", "hi", "ne", "sg", "sgg", "sl", "sll")], axis=-1)
        if not (np.array_equal(rec.cpu().numpy(), mine) and np.array_equal(hist.cpu().numpy(), h.astype(np.int64))):
            raise SystemExit("bench_grade: the torch chain and the grade job disagree")

    # (under the tracer the warm-up is all there is)
    lat, rate = bl.alternating_rounds(rects, job, done, 0 if trace_only else rounds, NJOBS, (100 if trace_only else 32, 100, 400))
    if not trace_only:
        base = float(np.median(lat["gray"]))
        for name in rects:
            print(json.dumps({"step": "rates", "config": name, "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "oversample": m, "quads_per_job": n, "jobs_in_flight": NJOBS, "rounds": rounds,
                              "bytes_per_quad": rects[name].patch_bytes, **bl.round_fields(lat[name]), "over_the_gray_job_us": round(float(np.median(lat[name])) - base, 1),
                              "jobs_per_s_median": round(float(np.median(rate[name])), 1), "quads_per_s_median": round(float(np.median(rate[name])) * n, 1), "frames": "device",
                              "output": "pinned" if name == "gray-pinned" else "device"}), flush=True)
    for rect in rects.values():
        rect.close()
    bl.free(ptrs + [dframe])
    for q in pins:
        L.rd_host_free(q)


def step_kernels(a, timeout):
    """the rates child under the tracer, on the product library and on --variant: the JSON lines as text, or None where there is no tracer"""
    lines = []
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "trace", "--size", a.size, "--patch", str(a.patch), "--oversample", str(a.oversample)]
    for lib in [None] + ([a.variant] if a.variant else []):
        env = None if lib is None else dict(os.environ, RD_LIB_PATH=os.path.abspath(lib))
        durations = bl.kernel_trace("bench_grade", cmd, timeout, lambda name: "k_grade" in name or "k_scan" in name or "k_rectify_tensor" in name, env=env)
        if durations is None:
            return None
        for short in sorted(durations):
            lines.append(json.dumps({"step": "kernels", "library": "product" if lib is None else os.path.basename(lib), "kernel": short, "size": a.size, "patch": "%dx%d" % (a.patch, a.patch),
                                     "oversample": a.oversample, **bl.kernel_fields(durations[short])}))
    return "".join(line + "\n" for line in lines)


def child_loop(iw, ih, p, m, nslots, pattern):
    ra = bl.require_gpu("bench_grade")
    rects = {"grade-c4-hist": ra.Rectifier(p, p, max_quads=64, njobs=NJOBS, grade=ra.grade_spec(4, oversample=m, hist=True))}
    for r, which, frames, dt, tally in bl.rectify_polled_runs(iw, ih, nslots, pattern, rects):
        print(json.dumps({"step": "loop", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "oversample": m, "nslots": nslots, "rectify_polled": which, "run": r, "first_detector_of_process": r == 0,
                          "frames": frames, "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "quads_per_s": round(tally[2] / dt, 1), "frames_kind": "device", "output": "device"}), flush=True)
    rects["grade-c4-hist"].close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--oversample", type=int, default=1)
    ap.add_argument("--steps", default="rates,kernels,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating configurations in the rates step")
    ap.add_argument("--repeat", type=int, default=2, help="rounds of (none, grade-c4-hist) in the loop step")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per GPU step")
    ap.add_argument("--variant", default=None, help="a timing-only build of the library (tools/variants.sh) to trace next to the product in the kernels step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "grade_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    iw, ih = (int(v) for v in a.size.split("x"))
    if a.child:
        if a.child == "rates":
            child_rates(iw, ih, a.patch, a.oversample, a.rounds, False)
        elif a.child == "trace":
            child_rates(iw, ih, a.patch, a.oversample, 0, True)
        else:
            child_loop(iw, ih, a.patch, a.oversample, a.nslots, ["none", "grade-c4-hist"] * a.repeat)
        return 0
    cmd = lambda step: [sys.executable, os.path.abspath(__file__), "--child", step, "--size", a.size, "--patch", str(a.patch), "--oversample", str(a.oversample), "--nslots", str(a.nslots),
                        "--rounds", str(a.rounds), "--repeat", str(a.repeat)]
    return bl.drive("bench_grade", a.steps.split(","), cmd, a.out, a.timeout, traced={"kernels": lambda timeout: step_kernels(a, timeout)})


if __name__ == "__main__":
    sys.exit(main())
