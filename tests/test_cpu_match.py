"""Matched quads without a GPU: rd_match_score against the restatement (tests/match.py) in every bit, rd_match_limits against the header, the restated selection
rule on crafted keys, and the host-only code under the sanitizers as a plain process.  No tolerance."""
import os
import re
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers
from tests import match

GRIDS = (8, 16, 32, 64)


def record(status=1, tmpl=0, rot=0, dot=0, tmpl2=-1, rot2=0, dot2=0, sa=0, saa=0):
    r = np.zeros((), ra.MATCH_DTYPE)
    r["status"], r["tmpl"], r["rot"], r["dot"], r["tmpl2"], r["rot2"], r["dot2"], r["sa"], r["saa"] = status, tmpl, rot, dot, tmpl2, rot2, dot2, sa, saa
    return r


def check(rec, G, sb, sbb, sb2, sbb2):
    got = ra.match_score(rec, G, sb, sbb, sb2, sbb2)
    want = match.complete(rec, G * G, sb, sbb, sb2, sbb2)
    assert got.tobytes() == want.tobytes(), (rec, G, sb, sbb, sb2, sbb2, got, want)
    return got


def sums(v):
    v = np.asarray(v, np.int64)
    return int(v.sum()), int((v * v).sum())


@pytest.mark.parametrize("G", GRIDS)
def test_score_equals_the_restatement_in_every_bit_on_random_signatures(G):
    rng = np.random.default_rng(100 + G)
    D = G * G
    for k in range(200):
        spread = (1, 3, 40, 128)[k % 4]
        a, b, c = (np.clip(rng.integers(-spread, spread + 1, D) + rng.integers(-100, 100), -128, 127) for _ in range(3))
        if match.flat(a) or match.flat(b) or match.flat(c):
            continue
        (sa, saa), (sb, sbb), (sc, scc) = sums(a), sums(b), sums(c)
        second = k % 3 != 0
        rec = record(1, k, k % 4, int(a @ b), k + 1 if second else -1, (k + 1) % 4 if second else 0, int(a @ c) if second else 0, sa, saa)
        got = check(rec, G, sb, sbb, sc, scc)
        assert -1.0 <= got["score"] <= 1.0 and (second or got["score2"] == 0.0)


@pytest.mark.parametrize("G", GRIDS)
def test_score_at_the_extreme_values(G):
    D = G * G
    for va in (-128, 127):
        for vb in (-128, 127):
            for odd_a in (-128, 127, 0):
                for odd_b in (-128, 127, 1):
                    a, b = np.full(D, va, np.int64), np.full(D, vb, np.int64)
                    a[0], b[-1] = odd_a, odd_b      # all cells but one
                    if match.flat(a) or match.flat(b):
                        continue
                    (sa, saa), (sb, sbb) = sums(a), sums(b)
                    check(record(1, 1, 3, int(a @ b), 0, 2, int(a @ a), sa, saa), G, sb, sbb, sa, saa)
    a = np.full(D, -128, np.int64)
    a[5] = 127
    sa, saa = sums(a)
    got = check(record(1, 0, 0, saa, -1, 0, 0, sa, saa), G, sa, saa, 0, 0)      # a quad that IS the template: the greatest dot there is at G = 64
    assert got["score"] == 1.0


@pytest.mark.parametrize("status", [0, 2, 3])
def test_other_statuses_zero_every_other_field(status):
    rec = record(status, 7, 3, 123456, 5, 1, -99, 17, 4000)
    rec["score"], rec["score2"] = 0.25, -0.5
    got = check(rec, 16, 5, 900, 6, 1000)
    assert got["status"] == status and got.tobytes()[4:] == bytes(52)


def test_limits_agree_with_the_header():
    txt = open(os.path.join(helpers.ROOT, "include", "rectdetect_hip.h")).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))
    lim = ra.match_limits()
    assert lim["max_templates"] == define("RD_MATCH_MAX_TEMPLATES") and lim["max_quads"] == define("RD_MATCH_MAX_QUADS")
    assert lim["grids"] == GRIDS and lim["oversamplings"] == (1, 2, 4)
    assert "G in {8, 16, 32, 64}" in txt and "m in {1, 2, 4}" in txt
    assert define("RD_MATCH_DOTS") == ra.MATCH_DOTS
    assert re.search(r"\}\s*rd_match;\s*/\* %d bytes \*/" % ra.MATCH_DTYPE.itemsize, txt)


def test_selection_rule_on_crafted_keys():
    # exact ties go to the lowest column
    assert match.select(np.array([1.0, 5.0, 5.0, 2.0, 5.0, 0.0, 0.0, 0.0])) == (1, 4)
    assert match.select(np.array([3.0, 3.0, 3.0, 3.0])) == (0, -1)      # one template: no runner-up
    # the runner-up skips the best's other rotations, however good they are
    assert match.select(np.array([0.0, 0.0, 0.0, 0.0, 9.0, 8.5, 8.0, 7.0, 1.0, 2.0, 2.0, 0.5])) == (4, 9)
    # a tie between the runner-up's candidates in different templates: the lowest column again
    assert match.select(np.array([6.0, -1.0, -1.0, -1.0, 4.0, 0.0, 0.0, 0.0, 7.0, 0.0, 0.0, 0.0, 4.0, 6.0, 0.0, 0.0])) == (8, 0)
    # negative keys are ordinary keys: anti-correlated everywhere, the least negative wins
    assert match.select(np.array([-5.0, -2.0, -3.0, -2.0, -9.0, -1.5, -8.0, -1.5])) == (5, 1)
    # the key is a signed square over vb: the order of num / sqrt(vb), computed without a square root
    num, vb = np.array([30, -40, 29, 41], np.int64), np.array([9, 16, 4, 25], np.int64)
    k = match.keys(num, vb)
    assert k.tolist() == [100.0, -100.0, 210.25, 67.24] and int(np.argmax(k)) == 2
    # keys of integers below 2^39 are exact products rounded once, then divided once
    big = np.array([(1 << 39) - 1, -((1 << 39) - 3)], np.int64)
    kk = match.keys(big, np.array([(1 << 39) - 5, 7], np.int64))
    assert kk[0] == (float(big[0]) * float(big[0])) / float((1 << 39) - 5) and kk[1] == -(float(big[1]) * float(big[1])) / 7.0


def test_rotation_is_a_clockwise_quarter_turn_and_four_make_the_identity():
    S = np.arange(64).reshape(8, 8)
    assert np.array_equal(match.rot(S), np.rot90(S, -1))
    assert np.array_equal(match.rot(match.rot(match.rot(match.rot(S)))), S)
    lib = match.library([S])
    assert lib.shape == (4, 64) and np.array_equal(lib[2].reshape(8, 8), S[::-1, ::-1])


def test_host_code_under_the_sanitizers_as_a_plain_process(tmp_path):
    """tests/native/match_host_check.c with csrc/rd_match_host.c, both compiled with -fsanitize=address,undefined, run as a process of its own"""
    csrc = os.path.join(helpers.ROOT, "rectdetect_amd", "csrc")
    exe = str(tmp_path / "match_host_check")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-DCL_TARGET_OPENCL_VERSION=120", "-I", csrc, "-I", os.path.join(helpers.ROOT, "include"),
           os.path.join(helpers.ROOT, "tests", "native", "match_host_check.c"), os.path.join(csrc, "rd_match_host.c"), "-o", exe, "-lm"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode != 0 and "sanitize" in p.stderr and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip("this compiler has no address / undefined sanitizer runtime: %s" % p.stderr[-200:])
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "match_host_check: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
