"""tools/benchlib.py and the ten bench tools built on it, as far as they go without a GPU: command lines, the step driver, the process group killed at the time limit,
and the call sequences of the timed loops and of the detector loop, written out here from the tools' earlier private copies."""
import os
import subprocess
import sys
import time

import pytest

import rectdetect_amd as ra
from tools import benchlib as bl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every tool with its first step and the smallest options its command line has
TOOLS = {"bench_rectify": ["--steps", "rates", "--sizes", "1280x720", "--patches", "64"], "bench_tensor": ["--steps", "rates"], "bench_scan": ["--steps", "rates"],
         "bench_grade": ["--steps", "rates"], "bench_code": ["--steps", "rates"], "bench_blobs": ["--steps", "rates"], "bench_annotate": ["--steps", "jobs"],
         "bench_composite": ["--steps", "jobs"], "bench_match": ["--steps", "jobs"], "bench_remap": ["--steps", "latency"]}
PY = [sys.executable, "-c"]


def tool(name, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", name + ".py")] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("name", sorted(TOOLS))
def test_help(name):
    res = tool(name, "--help")
    assert res.returncode == 0 and b"--steps" in res.stdout


@pytest.mark.skipif(ra.gpu_available(), reason="a HIP device is present: the tools would measure")
@pytest.mark.parametrize("name", sorted(TOOLS))
def test_without_a_device_nothing_is_measured(name, tmp_path):
    out = tmp_path / "out.jsonl"
    res = tool(name, "--out", str(out), *TOOLS[name])
    assert res.returncode != 0
    assert ("%s: no HIP device - nothing is measured without one" % name).encode() in res.stderr or \
           ("%s: torch sees no HIP device - nothing is measured without one" % name).encode() in res.stderr
    assert ("%s: step %s" % (name, TOOLS[name][1])).encode() in res.stderr and b"failed with status 1 - stopping" in res.stderr
    assert not out.exists() or out.read_text() == ""


# ---- run_step

def test_run_step_kills_the_whole_group_at_the_limit(tmp_path):
    pidfile = tmp_path / "pid"
    t = time.perf_counter()
    with pytest.raises(subprocess.TimeoutExpired):
        bl.run_step(["sh", "-c", "sleep 60 & echo $! > %s; sleep 60" % pidfile], 1)
    assert time.perf_counter() - t < 8
    pid = int(pidfile.read_text())
    # the grandchild was killed, not waited for: it may be a zombie of init's for a moment, which kill(pid, 0) still finds
    for _ in range(200):
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            break
        try:
            if open("/proc/%d/stat" % pid).read().rsplit(")", 1)[1].split()[0] == "Z":
                break
        except OSError:
            break
        time.sleep(0.01)
    else:
        pytest.fail("the grandchild %d outlived run_step" % pid)


def test_run_step_returns_status_and_output():
    assert bl.run_step(PY + ["import sys; print('x'); sys.exit(3)"], 30) == (3, b"x\n", None)
    rc, out, err = bl.run_step(PY + ["import sys; print('e', file=sys.stderr)"], 30, capture_stderr=True, env=dict(os.environ, BENCHLIB_TEST="1"))
    assert (rc, out, err) == (0, b"", b"e\n")


# ---- drive

def drive(tmp_path, steps, timeout=30, traced=None):
    """drive() over steps {name: python source}: (status, what --out holds)"""
    out = tmp_path / "sub" / "out.jsonl"      # (a directory that drive() makes)
    rc = bl.drive("bench_fake", list(steps), lambda step: PY + [steps[step]], str(out), timeout, traced=traced)
    return rc, out.read_text() if out.exists() else ""


def test_drive_appends_good_steps_in_order(tmp_path, capfd):
    assert drive(tmp_path, {"a": "print('{\"step\": \"a\"}')", "b": "print('{\"step\": \"b\"}')"}) == (0, '{"step": "a"}\n{"step": "b"}\n')
    assert capfd.readouterr().out == '{"step": "a"}\n{"step": "b"}\n'
    assert drive(tmp_path, {"c": "print('c')"}) == (0, '{"step": "a"}\n{"step": "b"}\nc\n')      # appended, never truncated


def test_drive_stops_at_a_failing_step(tmp_path, capfd):
    marker = tmp_path / "ran"
    rc, text = drive(tmp_path, {"a": "print('a')", "b": "import sys; print('half'); sys.exit(5)", "c": "open(%r, 'w')" % str(marker)})
    assert (rc, text) == (5, "a\n") and not marker.exists()
    got = capfd.readouterr()
    assert got.out == "a\nhalf\n" and "bench_fake: step b failed with status 5 - stopping" in got.err


def test_drive_signal_is_status_1(tmp_path, capfd):
    rc, text = drive(tmp_path, {"a": "import os, signal; os.kill(os.getpid(), signal.SIGKILL)", "b": "print('b')"})
    assert (rc, text) == (1, "")
    assert "bench_fake: step a failed with status -9 - stopping" in capfd.readouterr().err


def test_drive_time_limit_is_status_124(tmp_path, capfd):
    marker = tmp_path / "ran"
    t = time.perf_counter()
    rc, text = drive(tmp_path, {"a": "print('a')", "b": "import time; print('b', flush=True); time.sleep(60)", "c": "open(%r, 'w')" % str(marker)}, timeout=1)
    assert (rc, text) == (124, "a\n") and not marker.exists() and time.perf_counter() - t < 8
    assert "bench_fake: step b ran into its time limit of 1 s - stopping" in capfd.readouterr().err


def test_drive_traced_steps_and_tuples(tmp_path, capfd):
    def failing(timeout):
        raise subprocess.CalledProcessError(7, ["tracer"])

    out = tmp_path / "out.jsonl"
    steps = [("rates", "1280x720", "64"), ("kernels", "1280x720", "64"), ("left-out", "1280x720", "64"), ("bad", "1280x720", "64"), ("never", "1280x720", "64")]
    rc = bl.drive("bench_fake", steps, lambda s: PY + ["print(%r)" % " ".join(s)], str(out), 30,
                  traced={"kernels": lambda timeout: "traced %d\n" % timeout, "left-out": lambda timeout: None, "bad": failing})
    assert rc == 7 and out.read_text() == "rates 1280x720 64\ntraced 30\n"
    assert "bench_fake: step bad 1280x720 64 failed with status 7 - stopping" in capfd.readouterr().err


# ---- the timed loops

def recorder():
    calls = []
    return calls, (lambda k: calls.append(("job", k))), (lambda k: calls.append(("done", k)))


def pairs(ks):
    return [c for k in ks for c in (("job", k), ("done", k))]


def in_flight_calls(n, njobs):
    """what the tools' own loops did: njobs jobs, then a wait for the oldest ahead of every further job, then the drain"""
    calls = [("job", k) for k in range(njobs)]
    for k in range(njobs, n):
        calls += [("done", k - njobs), ("job", k)]
    return calls + [("done", k) for k in range(n - njobs, n)]


def test_in_flight_sequence():
    calls, job, done = recorder()
    assert bl.in_flight(job, done, 10, 4) > 0
    assert calls == [("job", 0), ("job", 1), ("job", 2), ("job", 3), ("done", 0), ("job", 4), ("done", 1), ("job", 5), ("done", 2), ("job", 6), ("done", 3), ("job", 7),
                     ("done", 4), ("job", 8), ("done", 5), ("job", 9), ("done", 6), ("done", 7), ("done", 8), ("done", 9)]
    assert calls == in_flight_calls(10, 4)
    calls.clear()
    bl.in_flight(job, done, 3, 4)      # fewer jobs than fit in flight
    assert calls == [("job", 0), ("job", 1), ("job", 2), ("done", 0), ("done", 1), ("done", 2)]


def test_timed_jobs_counts_and_sequence():
    calls, job, done = recorder()
    lat, dt = bl.timed_jobs(job, done, 4, 6, 30, 10)
    assert calls == pairs(range(6)) + pairs(range(30)) + in_flight_calls(10, 4)
    assert len(lat) == 30 and all(lat[i] <= lat[i + 1] for i in range(29)) and lat[0] >= 0 and dt > 0
    assert list(bl.latency_fields(list(range(300)))) == ["job_latency_us_median", "job_latency_us_p10", "job_latency_us_p90"]
    assert list(bl.latency_fields(list(range(300))).values()) == [150.0, 30.0, 270.0]


def test_alternating_rounds_order_and_slow_counts():
    calls = []
    lat, rate = bl.alternating_rounds({"a": 0, "slow": 0, "b": 0}, lambda name, k: calls.append((name, "job", k)), lambda name, k: calls.append((name, "done", k)),
                                      2, 4, (5, 7, 9), slow=("slow",), slow_counts=(1, 2, 6))
    named = lambda name, seq: [(name,) + c for c in seq]
    one_round = (named("a", pairs(range(7))) + named("slow", pairs(range(2))) + named("b", pairs(range(7)))      # the latency pass over every configuration, then
                 + named("a", in_flight_calls(9, 4)) + named("slow", in_flight_calls(6, 4)) + named("b", in_flight_calls(9, 4)))      # the pass with the jobs in flight
    assert calls == named("a", pairs(range(5))) + named("slow", pairs(range(1))) + named("b", pairs(range(5))) + one_round + one_round
    assert list(lat) == list(rate) == ["a", "slow", "b"] and all(len(v) == 2 for v in list(lat.values()) + list(rate.values()))
    assert list(bl.round_fields([3.0, 1.0, 2.0]).items()) == [("job_latency_us_median", 2.0), ("job_latency_us_min_round", 1.0), ("job_latency_us_max_round", 3.0)]
    # under the tracer: no rounds, the warm-up is all there is
    calls.clear()
    lat, rate = bl.alternating_rounds(["a"], lambda name, k: calls.append((name, "job", k)), lambda name, k: calls.append((name, "done", k)), 0, 4, (3, 7, 9))
    assert calls == named("a", pairs(range(3))) and lat == {"a": []} and rate == {"a": []}


# ---- the detector loop

class FakeDetector:
    def __init__(self, log, per_poll=(5, 0, 2)):
        self.log, self.out, self.most, self.per_poll, self.polls, self.closed = log, 0, 0, per_poll, 0, False

    def enqueue(self, i):
        self.out += 1
        self.most = max(self.most, self.out)
        self.log.append(("enqueue", i))

    def poll(self, tan):
        assert tan == bl.TAN36 and self.out > 0
        self.out -= 1
        self.log.append(("poll",))
        self.polls += 1
        return ["rect"] * self.per_poll[(self.polls - 1) % len(self.per_poll)]

    def close(self):
        self.closed = True


class FakeService:
    def __init__(self, log):
        self.log, self.out, self.most = log, 0, 0

    def start(self, k):
        self.out += 1
        self.most = max(self.most, self.out)
        self.log.append(("job", k))

    def wait(self):
        assert self.out > 0
        self.out -= 1
        self.log.append(("wait",))


def test_detector_loop_bookkeeping():
    log = []
    det, svc = FakeDetector(log), FakeService(log)
    seen = []

    def behind(d, worker, found, i, k):
        assert d is det and worker is svc
        seen.append((i, k, len(found)))
        worker.start(k)
        return min(len(found), 4)      # (as the tools hand over at most so many)

    tally = [0, 0, 0]
    bl.detector_loop(det, 8, 3, lambda d, i: d.enqueue(i), tally, first=100, worker=svc, njobs=2, behind=behind)
    assert det.most == 3 and svc.most == 2 and det.out == 0 and svc.out == 0
    assert [c for c in log if c[0] == "enqueue"] == [("enqueue", i) for i in range(100, 108)] and log.count(("poll",)) == 8
    assert seen == [(100 + j, j, (5, 0, 2)[j % 3]) for j in range(8)]      # every frame polled once, in order, each with the job number behind it
    assert log.count(("wait",)) == 8 and [c for c in log if c[0] == "job"] == [("job", k) for k in range(8)]
    # the order of the earlier private loops: three frames go in; from then on a poll (with a wait ahead of the job once two are out) ahead of every enqueue; the
    # frames still out are polled; the jobs still out are waited for
    P, W = ("poll",), ("wait",)
    assert log == [("enqueue", 100), ("enqueue", 101), ("enqueue", 102), P, ("job", 0), ("enqueue", 103), P, ("job", 1), ("enqueue", 104), P, W, ("job", 2), ("enqueue", 105),
                   P, W, ("job", 3), ("enqueue", 106), P, W, ("job", 4), ("enqueue", 107), P, W, ("job", 5), P, W, ("job", 6), P, W, ("job", 7), W, W]
    assert tally == [5 + 0 + 2 + 5 + 0 + 2 + 5 + 0, 8, 4 + 0 + 2 + 4 + 0 + 2 + 4 + 0]


def test_detector_loop_without_a_service():
    log = []
    det = FakeDetector(log)
    tally = [0, 0, 0]
    bl.detector_loop(det, 5, 2, lambda d, i: d.enqueue(i), tally)
    P = ("poll",)
    assert log == [("enqueue", 0), ("enqueue", 1), P, ("enqueue", 2), P, ("enqueue", 3), P, ("enqueue", 4), P, P] and tally == [5 + 0 + 2 + 5 + 0, 0, 0]


def test_detector_runs_new_detector_warm_up_then_timed():
    made, runs = [], []

    def new_detector():
        made.append(FakeDetector([]))
        return made[-1]

    def run(det, which, timed, tally):
        assert det is made[-1] and not det.closed
        runs.append((which, timed))
        tally[0] += 10 if timed else 1000      # (the warm-up's tally is not the run's)

    got = []
    for r, which, dt, tally in bl.detector_runs(["none", "x", "none"], new_detector, run):
        assert made[-1].closed and len(made) == r + 1
        got.append((r, which, tally))
        assert dt >= 0
    assert got == [(0, "none", [10, 0, 0]), (1, "x", [10, 0, 0]), (2, "none", [10, 0, 0])]
    assert runs == [("none", False), ("none", True), ("x", False), ("x", True), ("none", False), ("none", True)]


# ---- what is left in the tools

def test_one_definition_of_what_the_tools_share():
    shared = ("def run_step", "def synth_frames", "def own_quads", "def random_quads", "subprocess.run", "rocprofv3\", \"--kernel-trace\", \"-f\"", "inflight == NJOBS")
    for name in TOOLS:
        text = open(os.path.join(ROOT, "tools", name + ".py")).read()
        assert "from tools import benchlib as bl" in text
        assert [s for s in shared if s in text] == [], name
