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
RADII = (15, 63, 0)
SLOW = ("scan-pinned-host",)      # configurations timed over fewer jobs
A4 = (1654, 2339)


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


def blob_spec(radius, page):
    import rectdetect_amd as ra
    return ra.blob_spec(radius, 26 if radius else 96, 0, 1, False, 8, 4, 0, 256, page)


def child_rates(iw, ih, p, nq, rounds, trace_only):
    import rectdetect_amd as ra
    if not ra.gpu_available():
        raise SystemExit("bench_blobs: no HIP device - nothing is measured without one")
    L = ra.lib()
    frame = synth_frames(iw, ih, 1)[0]
    quads = own_quads(frame)[:nq]
    n = len(quads)
    if n == 0:
        raise SystemExit("bench_blobs: the synthetic frame holds no rectangle")
    dframe = L.rd_device_alloc(frame.nbytes)
    L.rd_upload(dframe, frame.ctypes.data, frame.nbytes)
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

    lat = {name: [] for name in rects}
    rate = {name: [] for name in rects}
    for name in rects:      # warm-up (under the tracer: all there is)
        for k in range(3 if name in SLOW else (100 if trace_only else 32)):
            job(name, k)
            done(name, k)
    for r in range(0 if trace_only else rounds):
        for name in rects:
            one = []
            for k in range(20 if name in SLOW else 100):
                t = time.perf_counter()
                job(name, k)
                done(name, k)
                one.append(time.perf_counter() - t)
            lat[name].append(float(np.median(one)) * 1e6)
        for name in rects:
            njobs_timed, inflight = 40 if name in SLOW else 400, 0
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
        for name in rects:
            radius = name.split("-r")[1].split("-")[0] if name.startswith("blobs-r") else None
            base = "scan-bits-r%s" % radius if radius not in (None, "0") else None
            over = [a - b for a, b in zip(lat[name], lat[base])] if base else None
            med = float(np.median(lat[name]))
            print(json.dumps({"step": "rates", "config": name, "size": "%dx%d" % (iw, ih), "patch": "%dx%d" % (p, p), "quads_per_job": n, "jobs_in_flight": NJOBS, "rounds": rounds,
                              "bytes_per_quad": rects[name].patch_bytes, "job_latency_us_median": round(med, 1), "job_latency_us_min_round": round(min(lat[name]), 1),
                              "job_latency_us_max_round": round(max(lat[name]), 1),
                              "over_the_scan_job_us_median": None if over is None else round(float(np.median(over)), 1),
                              "over_the_scan_job_us_range": None if over is None else [round(min(over), 1), round(max(over), 1)],
                              "jobs_per_s_median": round(float(np.median(rate[name])), 1), "jobs_per_s_range": [round(min(rate[name]), 1), round(max(rate[name]), 1)],
                              "frames": "device", "output": "pinned" if pinned(name) else "device"}), flush=True)
    for rect in rects.values():
        rect.close()
    for q in ptrs + [dframe]:
        L.rd_device_free(q)
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
    import rectdetect_amd as ra
    if not ra.gpu_available():
        raise SystemExit("bench_blobs: no HIP device - nothing is measured without one")
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
    """a child under the tracer: per kernel of the blobs job the median of its durations, as JSON lines"""
    lines = []
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "-o", "k", "--", sys.executable, os.path.abspath(__file__), "--child", child, "--size", a.size, "--patch", str(a.patch),
               "--quads", str(a.quads)]
        rc, _, err = run_step(cmd, timeout, capture_stderr=True)
        if rc != 0:
            sys.stderr.write(err.decode()[-2000:])
            raise subprocess.CalledProcessError(rc, cmd)
        durations = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Kernel_Name"]
                if "k_blob" in name or "k_scan" in name or "k_rectify_tensor" in name or "k_grade" in name:
                    key = name[name.index("k_"):].split("(")[0]
                    durations.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
        for key in sorted(durations):
            v = durations[key]
            lines.append(json.dumps({"step": "kernels", "workload": label, "kernel": key, "launches": len(v), "kernel_us_median": round(float(np.median(v)), 2),
                                     "kernel_us_min": round(min(v), 2), "kernel_us_max": round(max(v), 2)}))
    return "".join(line + "\n" for line in lines)


def step_kernels(a, timeout):
    if not shutil.which("rocprofv3"):
        print("bench_blobs: rocprofv3 is not installed - the kernels step is left out", file=sys.stderr)
        return None
    return traced(a, "trace", timeout, "%d pages of %dx%d (all radii and both page settings together)" % (a.quads, a.patch, a.patch)) + traced(a, "trace-a4", timeout, "one page of %dx%d" % A4)


def child_loop(iw, ih, p, nslots, pattern):
    import rectdetect_amd as ra
    if not ra.gpu_available():
        raise SystemExit("bench_blobs: no HIP device - nothing is measured without one")
    L = ra.lib()
    imgs = synth_frames(iw, ih, 16)
    dptrs = []
    for a in imgs:
        q = L.rd_device_alloc(a.nbytes)
        L.rd_upload(q, a.ctypes.data, a.nbytes)
        dptrs.append(q)
    frames, warmup, maxq = 1024 if iw * ih <= 1920 * 1080 else 256, 128, 64
    rects = {"blobs-r15-page": ra.Rectifier(p, p, max_quads=maxq, njobs=NJOBS, blobs=blob_spec(15, True))}
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
                          "frames": frames, "frames_per_s": round(frames / dt, 1), "rectangles": tally[0], "quads_per_s": round(tally[2] / dt, 1), "frames_kind": "device", "output": "device"}), flush=True)
    for rect in rects.values():
        rect.close()
    for q in outs + dptrs:
        L.rd_device_free(q)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blob_bench.jsonl"))
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for step in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--size", a.size, "--patch", str(a.patch), "--quads", str(a.quads), "--nslots", str(a.nslots), "--rounds", str(a.rounds),
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
                    print("bench_blobs: step %s failed with status %d - stopping" % (step, rc), file=sys.stderr)
                    return rc if rc > 0 else 1
        except subprocess.TimeoutExpired:
            print("bench_blobs: step %s ran into its time limit of %d s - stopping" % (step, a.timeout), file=sys.stderr)
            return 124
        except subprocess.CalledProcessError as e:
            print("bench_blobs: step %s failed with status %d - stopping" % (step, e.returncode), file=sys.stderr)
            return e.returncode if e.returncode > 0 else 1
        sys.stdout.write(text)
        sys.stdout.flush()
        with open(a.out, "a") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
