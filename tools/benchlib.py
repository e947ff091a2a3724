"""What the bench_*.py tools share: synthetic inputs, device buffers, the two timed job loops, the detector loop with a service behind every poll, the kernel tracer and
the step driver.  Plain functions; a tool is its configurations and its JSON lines (profiles/README.md, "The bench tools")."""
import csv
import functools
import glob
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))


# ---- inputs and buffers

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


def own_quads(frame):
    """the quads of the frame's own rectangles"""
    import rectdetect_amd as ra
    ih, iw = frame.shape[:2]
    det = ra.Detector(iw, ih, nslots=1, aperture=TAN36)
    det.enqueue(frame)
    rects = det.poll(TAN36)
    det.close()
    return ra.rect_quads(rects)


def own_frame(tool, iw, ih, nq):
    """frame 0 of the synthetic stream, the first nq quads of its own rectangles, the frame in device memory"""
    frame = synth_frames(iw, ih, 1)[0]
    quads = own_quads(frame)[:nq]
    if len(quads) == 0:
        raise SystemExit("%s: the synthetic frame holds no rectangle" % tool)
    return frame, quads, upload([frame])[0]


def upload(arrays):
    """a device buffer per array, filled with it"""
    import rectdetect_amd as ra
    L = ra.lib()
    ptrs = []
    for a in arrays:
        q = L.rd_device_alloc(a.nbytes)
        L.rd_upload(q, a.ctypes.data, a.nbytes)
        ptrs.append(q)
    return ptrs


def free(ptrs):
    import rectdetect_amd as ra
    for q in ptrs:
        ra.lib().rd_device_free(q)


def require_gpu(tool, torch_first=False):
    """the library, or the end of the process where there is no device; torch_first: torch is imported before the library is loaded, so that the process holds ONE HIP
    runtime, torch's"""
    if torch_first:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("%s: torch sees no HIP device - nothing is measured without one" % tool)
    import rectdetect_amd as ra
    if not ra.gpu_available():
        raise SystemExit("%s: no HIP device - nothing is measured without one" % tool)
    return ra


# ---- the timed job loops

def in_flight(job, done, n, njobs):
    """n jobs with njobs kept in flight, every one waited for at the end: the seconds it took"""
    inflight = 0
    t = time.perf_counter()
    for k in range(n):
        if inflight == njobs:
            done(k - njobs)
            inflight -= 1
        job(k)
        inflight += 1
    while inflight:
        done(n - inflight)
        inflight -= 1
    return time.perf_counter() - t


def latencies(job, done, n):
    """n jobs one at a time, enqueue to wait: the seconds of each"""
    lat = []
    for k in range(n):
        t = time.perf_counter()
        job(k)
        done(k)
        lat.append(time.perf_counter() - t)
    return lat


def timed_jobs(job, done, njobs, warmup, nlat, ntimed):
    """one configuration, job(k) and done(k): warm-up, nlat single-job latencies, ntimed jobs with njobs in flight.
    (the latencies in microseconds, sorted; the seconds the jobs in flight took)"""
    for k in range(warmup):
        job(k)
        done(k)
    lat = latencies(job, done, nlat)
    dt = in_flight(job, done, ntimed, njobs)
    return np.sort(np.array(lat)) * 1e6, dt


def latency_fields(lat):
    """the median, 10th and 90th percentile of timed_jobs' sorted latencies as the tools' JSON fields"""
    return {"job_latency_us_median": round(float(lat[len(lat) // 2]), 1), "job_latency_us_p10": round(float(lat[len(lat) // 10]), 1),
            "job_latency_us_p90": round(float(lat[len(lat) * 9 // 10]), 1)}


def alternating_rounds(names, job, done, rounds, njobs, counts, slow=(), slow_counts=None):
    """configurations that alternate within one process, job(name, k) and done(name, k): a warm-up of every one, then in every round a latency pass over all of them
    and a pass with njobs in flight over all of them.  counts = (warm-up, latencies per round, jobs in flight per round); the names in slow take slow_counts.
    ({name: each round's median latency in microseconds}, {name: each round's jobs per second})"""
    names = list(names)
    count = {name: slow_counts if name in slow else counts for name in names}
    jobs = {name: functools.partial(job, name) for name in names}      # (bound outside the timed regions)
    dones = {name: functools.partial(done, name) for name in names}
    lat = {name: [] for name in names}
    rate = {name: [] for name in names}
    for name in names:
        for k in range(count[name][0]):
            job(name, k)
            done(name, k)
    for r in range(rounds):
        for name in names:
            lat[name].append(float(np.median(latencies(jobs[name], dones[name], count[name][1]))) * 1e6)
        for name in names:
            rate[name].append(count[name][2] / in_flight(jobs[name], dones[name], count[name][2], njobs))
    return lat, rate


def round_fields(lat):
    """the median and the extremes of alternating_rounds' latencies of one configuration as the tools' JSON fields"""
    return {"job_latency_us_median": round(float(np.median(lat)), 1), "job_latency_us_min_round": round(min(lat), 1), "job_latency_us_max_round": round(max(lat), 1)}


# ---- the detector loop

def detector_loop(det, n, nslots, enqueue, tally, tan=TAN36, first=0, worker=None, njobs=0, behind=None):
    """n frames through det with nslots in flight: enqueue(det, i) hands frame i over, i = first .. first + n - 1.  With a worker, behind(det, worker, found, i, k)
    starts the worker's job k on what the poll of frame i found, no more than njobs of them out, and returns what it handed over.  Ends with every frame polled and
    every job waited for.  tally += [what the polls found, the jobs, what they were handed]"""
    inflight = jobs = 0
    polled = first

    def poll():
        nonlocal jobs, polled
        found = det.poll(tan)
        tally[0] += len(found)
        if worker is not None:
            if jobs == njobs:
                worker.wait()
                jobs -= 1
            tally[2] += behind(det, worker, found, polled, tally[1])
            tally[1] += 1
            jobs += 1
        polled += 1

    for i in range(first, first + n):
        if inflight == nslots:
            poll()
            inflight -= 1
        enqueue(det, i)
        inflight += 1
    while inflight:
        poll()
        inflight -= 1
    while jobs:
        worker.wait()
        jobs -= 1


def detector_runs(pattern, new_detector, run):
    """the runs of a pattern in one process, a new detector per run: run(det, which, False, tally) warms it up, run(det, which, True, tally) is timed.
    Yields (run number, which, seconds, tally) after the detector is closed; the FIRST detector of a process runs faster than every later one ("Rectified
    patches"), so the tools' lines say "first_detector_of_process" for run 0"""
    for r, which in enumerate(pattern):
        det = new_detector()
        run(det, which, False, [0, 0, 0])
        tally = [0, 0, 0]
        t = time.perf_counter()
        run(det, which, True, tally)
        dt = time.perf_counter() - t
        det.close()
        yield r, which, dt, tally


def rectify_polled_runs(iw, ih, nslots, pattern, rects, maxq=64, njobs=4):
    """the loop bench.py times (frames resident in HBM, post-process on a worker thread) with rectify_polled of the frame's own rectangles, at most maxq, into the
    rectifier rects[which] behind every poll; a which that rects does not hold runs the loop alone.  Yields (run number, which, frames, seconds, tally)"""
    import rectdetect_amd as ra
    dptrs = upload(synth_frames(iw, ih, 16))
    frames, warmup = 1024 if iw * ih <= 1920 * 1080 else 256, 128
    outs = [ra.lib().rd_device_alloc(maxq * max(r.patch_bytes for r in rects.values())) for _ in range(njobs)]

    def enqueue(det, i):
        det.enqueue(dptrs[i % len(dptrs)], iw * 3, on_device=True)

    def behind(det, rect, found, i, k):
        det.rectify_polled(rect, ra.rect_quads(found[:maxq]), outs[k % njobs])
        return min(len(found), maxq)

    def run(det, which, timed, tally):
        detector_loop(det, frames if timed else warmup, nslots, enqueue, tally, worker=rects.get(which), njobs=njobs, behind=behind)

    for r, which, dt, tally in detector_runs(pattern, lambda: ra.Detector(iw, ih, nslots=nslots, nworkers=1, aperture=TAN36), run):
        yield r, which, frames, dt, tally
    free(outs + dptrs)


# ---- child processes

def run_step(cmd, timeout, capture_stderr=False, env=None):
    """cmd in a process group of its own, the whole group killed at the time limit - under the tracer the GPU is open in a grandchild, which the death of its parent
    would not end: (return code, stdout, stderr or None); subprocess.TimeoutExpired once every process of the step is gone"""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE if capture_stderr else None, start_new_session=True, env=env)
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


def kernel_trace(tool, cmd, timeout, keep, env=None):
    """cmd under rocprofv3 --kernel-trace: {short kernel name: its launches' durations in microseconds, in the order they started} for the kernels whose full name
    keep() accepts; None, with a message, where rocprofv3 is not installed"""
    if not shutil.which("rocprofv3"):
        print("%s: rocprofv3 is not installed - the kernels step is left out" % tool, file=sys.stderr)
        return None
    with tempfile.TemporaryDirectory() as d:
        full = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "-o", "k", "--"] + cmd
        rc, _, err = run_step(full, timeout, capture_stderr=True, env=env)
        if rc != 0:
            sys.stderr.write(err.decode()[-2000:])
            raise subprocess.CalledProcessError(rc, full)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                rows += [row for row in csv.DictReader(f) if keep(row["Kernel_Name"])]
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    durations = {}
    for row in rows:
        name = row["Kernel_Name"]
        durations.setdefault(name[name.index("k_"):].split("(")[0], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    return durations


def kernel_fields(v):
    """one kernel's durations as the tools' JSON fields"""
    return {"launches": len(v), "kernel_us_median": round(float(np.median(v)), 2), "kernel_us_min": round(min(v), 2), "kernel_us_max": round(max(v), 2)}


def drive(tool, steps, make_cmd, out, timeout, traced=None):
    """the tool's steps one after the other, make_cmd(step) each in a child under run_step; a step is a name or a tuple that starts with one.  traced[name](timeout)
    gives the text of a step that is not one plain child, or None where it is left out.  A step's lines are printed and appended to out when it succeeded; the first
    that fails ends the tool: its status, 124 for the time limit"""
    traced = traced or {}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for step in steps:
        name, label = (step, step) if isinstance(step, str) else (step[0], " ".join(step))
        try:
            if name in traced:
                text = traced[name](timeout)
                if text is None:
                    continue
            else:
                cmd = make_cmd(step)
                rc, stdout, _ = run_step(cmd, timeout)
                text = stdout.decode()
                if rc != 0:
                    sys.stdout.write(text)
                    sys.stdout.flush()
                    raise subprocess.CalledProcessError(rc, cmd)
        except subprocess.TimeoutExpired:
            print("%s: step %s ran into its time limit of %d s - stopping" % (tool, label, timeout), file=sys.stderr)
            return 124
        except subprocess.CalledProcessError as e:
            print("%s: step %s failed with status %d - stopping" % (tool, label, e.returncode), file=sys.stderr)
            return e.returncode if e.returncode > 0 else 1
        sys.stdout.write(text)
        sys.stdout.flush()
        with open(out, "a") as f:
            f.write(text)
    return 0
