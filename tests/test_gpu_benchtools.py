"""The bench tools' untraced steps at the smallest options their command lines allow, line by line against what the parent of the benchlib refactor printed
(tests/golden/bench_tools_parent.json: recorded on an MI355X from two runs of the parent's tools; its header says how).  Per line: the keys in order, the value of every
field but the measured ones (names, sizes, counts of jobs, frames, quads, rectangles and launches), and the type of every measured field.  Measured are the fields whose
names the header lists: those that differed between the parent's two runs in any line of any tool, all of them times and rates - where two runs printed the same time
in some line, they agreed by accident."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--size", "1280x720", "--patch", "64"]
CASES = [
    ("bench_rectify", "rates", ["--sizes", "1280x720", "--patches", "64"]),
    ("bench_rectify", "loop", ["--sizes", "1280x720", "--patches", "64", "--pattern", "0,1"]),
    ("bench_tensor", "rates", SMALL + ["--rounds", "1"]),
    ("bench_tensor", "loop", SMALL + ["--repeat", "1"]),
    ("bench_scan", "rates", SMALL + ["--rounds", "1"]),
    ("bench_scan", "loop", SMALL + ["--repeat", "1"]),
    ("bench_grade", "rates", SMALL + ["--rounds", "1"]),
    ("bench_grade", "loop", SMALL + ["--repeat", "1"]),
    ("bench_code", "rates", SMALL + ["--rounds", "1"]),
    ("bench_code", "loop", SMALL + ["--repeat", "1"]),
    ("bench_blobs", "rates", SMALL + ["--rounds", "1"]),
    ("bench_blobs", "a4", SMALL + ["--repeat", "1"]),
    ("bench_blobs", "loop", SMALL + ["--repeat", "1"]),
    ("bench_annotate", "jobs", []),
    ("bench_annotate", "loop", ["--pattern", "none,rectify,annotate,annotate_out"]),      # (uploads its 7 GB frame pool: some 8 s)
    ("bench_composite", "jobs", []),
    ("bench_composite", "loop", ["--pattern", "none,rectify,annotate,composite"]),
    ("bench_match", "jobs", ["--repeat", "1"]),
    ("bench_match", "loop", ["--repeat", "1"]),
    ("bench_remap", "latency", []),
    ("bench_remap", "loop", ["--pattern", "0,1"]),
]


def signature(v):
    """the types in a value, through lists and dictionaries"""
    if isinstance(v, dict):
        return {k: signature(x) for k, x in v.items()}
    if isinstance(v, list):
        return [signature(x) for x in v]
    return type(v).__name__


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "bench_tools_parent.json")) as f:
        return json.load(f)["cases"]


def test_every_recorded_case_is_run(parent):
    assert sorted(parent) == sorted("%s-%s" % c[:2] for c in CASES)


@pytest.mark.parametrize("tool,step,options", CASES, ids=["%s-%s" % c[:2] for c in CASES])
def test_lines_as_the_parent_printed_them(tool, step, options, parent, tmp_path):
    want = parent["%s-%s" % (tool, step)]
    assert want["options"] == options
    out = tmp_path / "out.jsonl"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"), "--steps", step, "--out", str(out), "--timeout", "90"] + options,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    text = res.stdout.decode()
    assert out.read_text() == text
    lines = [json.loads(line) for line in text.splitlines()]
    assert len(lines) == len(want["lines"])
    for got, w in zip(lines, want["lines"]):
        assert list(got) == w["keys"]
        assert {k: got[k] for k in w["same"]} == w["same"]
        assert {k: signature(got[k]) for k in w["types"]} == w["types"]
