#!/usr/bin/env python3
"""Rates of the blobs rectifier (rd_rectifier_create_blobs): one JSON line per configuration, appended to profiles/blob_bench.jsonl (--out).

On a synthetic frame's own rectangles (the rectangle detector's list for frame 0 of the stream, the first --quads of them, device frames), --patch x --patch pages:
  * "rates":   the latency of one job (enqueue to wait, nothing else on the device) and jobs/s with the jobs kept in flight, for
                 blobs-rR[-page]    the blobs job at radius R = 15, 63 and 0 (the fixed level), without and with the cleaned page;
                 scan-bits-rR       the RD_SCAN_BITS scan job at the same radius: the blobs job's first two launches on their own, the figure to judge it by;
                 grade-c4           the grade job: the other job that adds into stream-zeroed records;
                 scan-pinned-host   the scan job's bits read back to pinned host memory and labelled there by rd_blob_page_host, page by page: what a caller
                                    pays today; scan-pinned the read-back alone;
               the configurations ALTERNATE within one process, --rounds times; a line holds the median over the rounds of each round's median latency, the
               rounds' extremes, and the difference from the scan job of the same radius and run: what the component stage costs.
  * "kernels": the launches apart: the rates child's jobs once more under rocprofv3 --kernel-trace (csv), per kernel the median of its durations in the trace -
               the component stage's per-launch split, for the --patch pages and (the "a4" child under the tracer) for one 1654 x 2339 page.  Left out, with a
               message, where rocprofv3 is not installed.
  * "a4":      one A4-sized page at 200 dpi, 1654 x 2339, a rendered page of text-like strokes, through rd_blobs_pages_device (uploads, scratch and the
               download included) against rd_blob_page_host on the same bits; the two must agree.
  * "loop":    the rectangle detector's frames/s (64 slots, post-process on a worker thread, frames resident in HBM - the loop bench.py times) without a
               rectifier and with the blobs rectifier { radius 15, page } behind every poll; the two alternate --repeat times in one process, a new detector per
               run.  The FIRST detector of a process runs faster than every later one ("Rectified patches"): compare runs 1 and later.
Every GPU step is a child process in a process group of its own under a time limit of its own, at which the whole group is killed (the tracer's child too); the tool
stops at the first step that fails.  bench.py is not involved.

    python tools/bench_blobs.py [--size 1920x1080] [--patch 128] [--quads 10] [--steps rates,kernels,a4,loop] [--rounds R] [--repeat R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tools import benchlib as bl

NJOBS = 4
RADII = (15, 63, 0)
SLOW = ("scan-pinned-host",)      # configurations timed over fewer jobs
A4 = (1654, 2339)


def blob_spec(radius, page):
    import rectdetect_amd as ra
    return ra.blob_spec(radius, 26 if radius else 96, 0, 1, False, 8, 4, 0, 256, page)


def child_rates(iw, ih, p, nq, rounds, trace_only):
    ra = bl.require_gpu("bench_blobs")
    L = ra.lib()
    frame, quads, dframe = bl.own_frame("bench_blobs", iw, ih, nq)
    n = len(quads)
    scan = lambda r: ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, scan=ra.scan_spec(ra.SCAN_BITS, r))
    rects = {}
    for r in RADII:
        if r:
            rects["scan-bits-r%d" % r] = scan(r)
        for page in (False, True):
            rects["blobs-r%d%s" % (r, "-page" if page else "")] = ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, blobs=blob_spec(r, page))
    rects["grade-c4"] = ra.Rectifier(p, p, max_quads=n, njobs=NJOBS, grade=ra.grade_spec(4))
    rects["scan-pinned"] = scan(15)
    if not trace_only:
        rects["scan-pinned-host"] = scan(15)
    most = max(r.patch_bytes for r in rects.values())
    ptrs = [L.rd_device_alloc(n * most) for _ in range(NJOBS)]
    rb = (p + 7) // 8
    pins = [L.rd_host_alloc(n * rb * p) for _ in range(NJOBS)]
    hspec = blob_spec(15, True)
    hbytes = ra.blob_bytes(hspec, p, p)
    hout = np.zeros((n, hbytes // 8), np.uint64)
    pinned = lambda name: name.startswith("scan-pinned")

    def job(name, k):
        rects[name].enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, pins[k % NJOBS] if pinned(name) else ptrs[k % NJOBS], on_device=True, out_pinned=pinned(name))

    def done(name, k):
        status = rects[name].wait()
        if name == "scan-pinned-host":
            hout[:] = 0
            for q in range(n):
                if status[q]:
                    L.rd_blob_page_host(pins[k % NJOBS] + q * rb * p, p, p, hspec.ctypes.data, hout[q].ctypes.data)
            return hout.view(np.uint8)

    if not trace_only:      # the host's labelling computes what the job computes: compare once
        job("scan-pinned-host", 0)
        host = done("scan-pinned-host", 0).copy()
        check = ra.Rectifier(p, p, max_quads=n, njobs=1, blobs=hspec)
        mine = check.rectify(frame, quads)
        check.close()
        if not np.array_equal(host, mine):
            raise SystemExit("bench_blobs: rd_blob_page_host on the scan job's bits and the blobs job disagree")
        heads = ra.blob_view(mine, hspec, p, p)[0]
        print(json.dumps({"step": "pages", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "quads": n, "ink_per_page_median": int(np.median(heads["ink"])),
                          "components_per_page_median": int(np.median(heads["all"])), "kept_per_page_median": int(np.median(heads["found"])), "largest_component": int(heads["largest"].max())}), flush=True)

    # (under the tracer the warm-up is all there is)
    lat, rate = bl.alternating_rounds(rects, job, done, 0 if trace_only else rounds, NJOBS, (100 if trace_only else 32, 100, 400), slow=SLOW, slow_counts=(3, 20, 40))
    if not trace_only:
        for name in rects:
            radius = name.split("-r")[1].split("-")[0] if name.startswith("blobs-r") else None
            base = "scan-bits-r%s" % radius if radius not in (None, "0") else None
            over = [a - b for a, b in zip(lat[name], lat[base])] if base else None
            print(json.dumps({"step": "rates", "config": name, "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "quads_per_job": n, "jobs_in_flight": NJOBS, "rounds": rounds,
                              "bytes_per_quad": rects[name].patch_bytes, **bl.round_fields(lat[name]),
                              "over_the_scan_job_us_median": None if over is None else round(float(np.median(over)), 1),
                              "over_the_scan_job_us_range": None if over is None else [round(min(over), 1), round(max(over), 1)],
                              "jobs_per_s_median": round(float(np.median(rate[name])), 1), "jobs_per_s_range": [round(min(rate[name]), 1), round(max(rate[name]), 1)],
                              "frames": "device", "output": "pinned" if pinned(name) else "device"}), flush=True)
    for rect in rects.values():
        rect.close()
    bl.free(ptrs + [dframe])
    for q in pins:
        L.rd_host_free(q)


def a4_page():
    """an A4 page at 200 dpi of text-like strokes: rows of small boxes of random width with gaps, speckle between them"""
    pw, ph = A4
    rng = np.random.default_rng(4)
    m = np.zeros((ph, pw), bool)
    for y in range(120, ph - 120, 34):
        x = 120
        while x < pw - 140:
            w, h = int(rng.integers(6, 18)), int(rng.integers(10, 22))
            m[y:y + h, x:x + 2] = m[y:y + h, x + w:x + w + 2] = True
            m[y:y + 2, x:x + w + 2] = m[y + h // 2:y + h // 2 + 2, x:x + w] = True
            x += w + int(rng.integers(4, 14))
    m |= rng.random((ph, pw)) < 0.002
    return m


def child_a4(repeat, trace_only):
    ra = bl.require_gpu("bench_blobs")
    pw, ph = A4
    bits = np.packbits(a4_page(), axis=1, bitorder="big")
    spec = ra.blob_spec(15, 26, 0, 1, False, 8, 4, 0, 4096, True)
    dev, host = [], []
    for k in range(2 + (3 if trace_only else repeat)):
        t = time.perf_counter()
        got, info = ra.blobs_pages(bits, pw, ph, spec)
        dev.append(time.perf_counter() - t)
        t = time.perf_counter()
        want = ra.blob_page_host(bits, pw, ph, spec)
        host.append(time.perf_counter() - t)
        if not np.array_equal(got[0], want):
            raise SystemExit("bench_blobs: the device and rd_blob_page_host disagree on the A4 page")
    if not trace_only:
        h = ra.blob_view(got, spec, pw, ph)[0][0]
        dev, host = dev[2:], host[2:]
        print(json.dumps({"step": "a4", "page": "%dx%d" % A4, "ink": int(h["ink"]), "components": int(h["all"]), "kept": int(h["found"]), "launches": info["launches"], "runs": len(dev),
                          "device_call_ms_median": round(float(np.median(dev)) * 1e3, 3), "device_call_ms_range": [round(min(dev) * 1e3, 3), round(max(dev) * 1e3, 3)],
                          "host_ms_median": round(float(np.median(host)) * 1e3, 3), "host_ms_range": [round(min(host) * 1e3, 3), round(max(host) * 1e3, 3)],
                          "device_call_includes": "scratch allocation, upload of the bits, the stage, download of the records and the page"}), flush=True)


def traced(a, child, timeout, label):
    """a child under the tracer: per kernel of the blobs job the median of its durations, as JSON lines; None where there is no tracer"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--size", a.size, "--patch", str(a.patch), "--quads", str(a.quads)]
    durations = bl.kernel_trace("bench_blobs", cmd, timeout, lambda name: "k_blob" in name or "k_scan" in name or "k_rectify_tensor" in name or "k_grade" in name)
    if durations is None:
        return None
    return "".join(json.dumps({"step": "kernels", "workload": label, "kernel": key, **bl.kernel_fields(durations[key])}) + "\n" for key in sorted(durations))


def step_kernels(a, timeout):
    pages = traced(a, "trace", timeout, "%d pages of %dx%d (all radii and both page settings together)" % (a.quads, a.patch, a.patch))
    return None if pages is None else pages + traced(a, "trace-a4", timeout, "one page of %dx%d" % A4)


def child_loop(iw, ih, p, nslots, pattern):
    ra = bl.require_gpu("bench_blobs")
    rects = {"blobs-r15-page": ra.Rectifier(p, p, max_quads=64, njobs=NJOBS, blobs=blob_spec(15, True))}
    for r, which, frames, dt, tally in bl.rectify_polled_runs(iw, ih, nslots, pattern, rects):
        print(json.dumps({"step": "loop", "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "nslots": nslots, "rectify_polled": which, "run": r, "first_detector_of_process": r == 0,
                          "frames": frames, "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "quads_per_s": round(tally[2] / dt, 1), "frames_kind": "device", "output": "device"}), flush=True)
    rects["blobs-r15-page"].close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--quads", type=int, default=10, help="quads per job: the first of the frame's own rectangles")
    ap.add_argument("--steps", default="rates,kernels,a4,loop")
    ap.add_argument("--nslots", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating configurations in the rates step")
    ap.add_argument("--repeat", type=int, default=2, help="rounds of (none, blobs) in the loop step; ten times as many runs of the a4 step")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed per GPU step")
    ap.add_argument("--out", default=os.path.join(bl.ROOT, "profiles", "blob_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    iw, ih = (int(v) for v in a.size.split("x"))
    if a.child:
        if a.child == "rates":
            child_rates(iw, ih, a.patch, a.quads, a.rounds, False)
        elif a.child == "trace":
            child_rates(iw, ih, a.patch, a.quads, 0, True)
        elif a.child == "a4":
            child_a4(10 * a.repeat, False)
        elif a.child == "trace-a4":
            child_a4(0, True)
        else:
            child_loop(iw, ih, a.patch, a.nslots, ["none", "blobs-r15-page"] * a.repeat)
        return 0
    cmd = lambda step: [sys.executable, os.path.abspath(__file__), "--child", step, "--size", a.size, "--patch", str(a.patch), "--quads", str(a.quads), "--nslots", str(a.nslots),
                        "--rounds", str(a.rounds), "--repeat", str(a.repeat)]
    return bl.drive("bench_blobs", a.steps.split(","), cmd, a.out, a.timeout, traced={"kernels": lambda timeout: step_kernels(a, timeout)})


if __name__ == "__main__":
    sys.exit(main())
