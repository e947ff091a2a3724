"""Graded quads without a GPU: the header's declarations and the library's exports, sizeof(rd_grade_spec) and sizeof(rd_grade_cell) with their offsets, the numpy
dtypes against them, rd_grade_spec_ok on every side of every bound, rd_grade_bytes, rd_grade_cell_of against the restatement (tests/grade.py) for every pixel, the
limits, the restatement two ways, its invariants, rd_grade_sharpness and rd_grade_percentile bit for bit, the bounds that make the sums 64-bit, the host-only code
under the sanitizers as a plain process - and that the contract does what it is for: a blurred page is less sharp in every cell that holds ink, and a glare spot
shows in the cells it overlaps and in no other.  No tolerance."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import grade
from tests import helpers

FUNCTIONS = ("rd_grade_spec_ok", "rd_grade_bytes", "rd_grade_cell_of", "rd_grade_limits", "rd_grade_sharpness", "rd_grade_percentile", "rd_rectifier_create_grade")
SPEC_FIELDS = ("cells", "dark", "bright", "edge", "oversample", "hist")
# per field: (legal values at its bounds, illegal values one past them)
BOUNDS = {"cells": ((1, 2, 4, 8), (0, 3, 5, 16, -1)), "dark": ((0, 1, 254, 255), (-1, 256)), "bright": ((0, 1, 254, 255), (-1, 256)), "edge": ((0, 1, 1019, 1020), (-1, 1021)),
          "oversample": ((1, 2, 4), (0, 3, 5, 8, -1)), "hist": ((0, 1), (-1, 2))}


def header():
    return open(os.path.join(helpers.ROOT, "include", "rectdetect_hip.h")).read()


def test_header_declares_the_functions_and_structs():
    txt = header()
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    assert re.search(r"typedef struct \{ int32_t cells, dark, bright, edge, oversample, hist, reserved\[2\]; \} rd_grade_spec;", txt)
    assert re.search(r"typedef struct \{ int32_t n, lo, hi, ne; int64_t sg, sgg, sl, sll; \} rd_grade_cell;", txt)
    assert txt.index("model-ready tensors:") < txt.index("scanned pages:") < txt.index("graded quads:") < txt.index("annotated frames:")
    assert "rd_grade_bytes" in txt[txt.index("size_t rd_rectifier_patch_bytes") - 300:txt.index("size_t rd_rectifier_patch_bytes")], "rd_rectifier_patch_bytes' comment names the new kind"
    assert (ra.GRADE_CELL_BYTES, ra.GRADE_HIST_BYTES, ra.GRADE_MAX_EDGE) == (48, 1024, 1020)
    for name in ("grade_spec", "grade_spec_ok", "grade_bytes", "grade_limits", "grade_sharpness", "grade_percentile", "grade_view", "GRADE_SPEC_DTYPE", "GRADE_CELL_DTYPE"):
        assert hasattr(ra, name), name


def test_library_exports_the_functions():
    L = ctypes.CDLL(ra.LIB_PATH)
    missing = [n for n in FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_sizeof_the_structs_and_the_numpy_dtypes(tmp_path):
    spec_off = {"cells": 0, "dark": 4, "bright": 8, "edge": 12, "oversample": 16, "hist": 20, "reserved": 24}
    cell_off = {"n": 0, "lo": 4, "hi": 8, "ne": 12, "sg": 16, "sgg": 24, "sl": 32, "sll": 40}
    checks = " && ".join(["offsetof(rd_grade_spec, %s) == %d" % kv for kv in spec_off.items()] + ["offsetof(rd_grade_cell, %s) == %d" % kv for kv in cell_off.items()])
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "rectdetect_hip.h"\nint main(void) { return sizeof(rd_grade_spec) == 32 && sizeof(rd_grade_cell) == 48 && %s ? 0 : 1; }\n' % checks)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-DCL_TARGET_OPENCL_VERSION=120", "-I", os.path.join(helpers.ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    assert ra.GRADE_SPEC_DTYPE.itemsize == 32 and ra.GRADE_SPEC_DTYPE.names == tuple(spec_off) and {f: ra.GRADE_SPEC_DTYPE.fields[f][1] for f in spec_off} == spec_off
    assert ra.GRADE_SPEC_DTYPE.fields["reserved"][0].shape == (2,)
    assert ra.GRADE_CELL_DTYPE.itemsize == 48 and ra.GRADE_CELL_DTYPE.names == grade.FIELDS and {f: ra.GRADE_CELL_DTYPE.fields[f][1] for f in cell_off} == cell_off
    assert [ra.GRADE_CELL_DTYPE.fields[f][0].itemsize for f in grade.FIELDS] == [4, 4, 4, 4, 8, 8, 8, 8]


def test_limits():
    lim = ra.grade_limits()
    assert lim["cells"] == grade.CELLS and lim["oversamplings"] == (1, 2, 4) and lim["max_edge"] == 1020 and lim["cell_bytes"] == 48 and lim["hist_bytes"] == 1024
    assert lim["tile_w"] >= 64 and lim["tile_w"] % 64 == 0 and lim["tile_h"] >= 1
    a = np.full(10, -7, np.int32)
    ra.lib().rd_grade_limits(a.ctypes.data + 4)
    assert a[0] == a[9] == -7 and a[1:3].tolist() == [15, 7] and a[6:9].tolist() == [48, 1024, 0]


def test_the_default_spec():
    s = ra.grade_spec()
    assert [int(s[f]) for f in SPEC_FIELDS] == [4, 8, 247, 64, 1, 0] and s["reserved"].tolist() == [0, 0]
    assert int(ra.grade_spec(hist=True)["hist"]) == 1


def test_spec_ok_on_every_side_of_every_bound():
    ok = ra.grade_spec(4, 8, 247, 64, 2, True)
    assert ra.grade_spec_ok(ok, 128, 96)
    for field, (legal, illegal) in BOUNDS.items():
        for v in legal:
            s = ok.copy()
            s[field] = v
            assert ra.grade_spec_ok(s, 128, 96), (field, v)
            assert ra.grade_bytes(s, 128, 96) > 0
        for v in illegal:
            s = ok.copy()
            s[field] = v
            assert not ra.grade_spec_ok(s, 128, 96), (field, v)
            assert ra.grade_bytes(s, 128, 96) == 0
    for k in (0, 1):
        for v in (1, -1):
            s = ok.copy()
            s["reserved"][k] = v
            assert not ra.grade_spec_ok(s, 128, 96), ("reserved", k, v)
    for c in grade.CELLS:
        s = ra.grade_spec(c)
        assert ra.grade_spec_ok(s, c, c) and ra.grade_spec_ok(s, c, 100) and ra.grade_spec_ok(s, 100, c)
        assert not ra.grade_spec_ok(s, c - 1, c) and not ra.grade_spec_ok(s, c, c - 1) and not ra.grade_spec_ok(s, c - 1, 100) and not ra.grade_spec_ok(s, 100, c - 1)
    for m in (1, 2, 4):
        s = ra.grade_spec(8, oversample=m)
        assert ra.grade_spec_ok(s, 16384 // m, 16384 // m) and ra.grade_spec_ok(s, 16384 // m - 1, 8)      # pw * m = 16384
        assert not ra.grade_spec_ok(s, 16384 // m + 1, 8) and not ra.grade_spec_ok(s, 8, 16384 // m + 1)   # pw * m = 16385 at m = 1, the first illegal size at every m
        assert not ra.grade_spec_ok(s, 0, 8) and not ra.grade_spec_ok(s, 8, 0) and not ra.grade_spec_ok(s, -1, 8)
    assert ra.grade_spec_ok(ra.grade_spec(1), 16384, 16384) and not ra.grade_spec_ok(ra.grade_spec(1), 16385, 1)
    assert ra.lib().rd_grade_spec_ok(None, 8, 8) == 0 and ra.lib().rd_grade_bytes(None, 8, 8) == 0


def test_bytes():
    for c in grade.CELLS:
        for h in (False, True):
            for m in (1, 4):
                s = ra.grade_spec(c, hist=h, oversample=m)
                assert ra.grade_bytes(s, 100, 60) == 48 * c * c + 1024 * h == grade.nbytes(s)
                assert ra.grade_bytes(s, 100, 60) % 8 == 0


def test_cell_of_equals_the_restatement_for_every_pixel():
    for pw, ph in ((9, 5), (65, 17), (131, 15)):
        for c in grade.CELLS:
            s = ra.grade_spec(c)
            if ph < c:
                assert not ra.grade_spec_ok(s, pw, ph) and ra.grade_cell_of(s, pw, ph, 0, 0) == -1
                continue
            want = grade.cell_index(pw, ph, c)
            got = np.array([[ra.lib().rd_grade_cell_of(s.ctypes.data, pw, ph, i, j) for i in range(pw)] for j in range(ph)])
            assert np.array_equal(got, want), (pw, ph, c)
            assert sorted(set(want.ravel().tolist())) == list(range(c * c)), "no cell is empty"
            for i, j in ((-1, 0), (pw, 0), (0, -1), (0, ph)):
                assert ra.grade_cell_of(s, pw, ph, i, j) == -1


def test_restatement_two_ways():
    rng = np.random.default_rng(17)
    for pw, ph in ((1, 1), (2, 1), (1, 3), (8, 8), (9, 5), (13, 11)):
        G = rng.integers(0, 256, (ph, pw))
        assert np.array_equal(grade.laplacian(G), grade.laplacian_loop(G)), (pw, ph)
        for c in grade.CELLS:
            if min(pw, ph) < c:
                continue
            for dark, bright, edge in ((8, 247, 64), (0, 255, 0), (255, 0, 1020), (100, 100, 300)):
                s = ra.grade_spec(c, dark, bright, edge)
                a, b = grade.cells_of(G, s), grade.cells_of_loop(G, s)
                assert a.tobytes() == b.tobytes(), (pw, ph, grade.name(s))
    assert grade.laplacian(np.full((4, 5), 200)).any() == False, "a constant plane has L = 0 up to the border"


def test_invariants():
    rng = np.random.default_rng(23)
    for pw, ph in ((8, 8), (65, 17), (131, 15), (100, 49)):
        G = rng.integers(0, 256, (ph, pw)).astype(np.uint8)
        for c in grade.CELLS:
            s = ra.grade_spec(c, hist=True, edge=0)
            cells, hist = ra.grade_view(grade.quad_bytes(G, s)[None], s)
            assert int(cells["n"].sum()) == pw * ph and int(hist.sum()) == pw * ph
            assert int(cells["sg"].sum()) == int((np.arange(256, dtype=np.int64) * hist[0]).sum()) == int(G.astype(np.int64).sum())
            assert int(cells["sgg"].sum()) == int((np.arange(256, dtype=np.int64) ** 2 * hist[0]).sum())
            assert np.array_equal(cells["ne"], cells["n"]), "edge 0: every pixel counts"
            assert cells.shape == (1, c, c) and cells["n"].min() >= 1
    z = grade.from_planes(np.zeros((2, 8, 8), np.uint8), [0, 1], ra.grade_spec(2, hist=True))
    assert not z[0].any() and z[1].any(), "an invalid quad is zero bytes"


def test_sharpness_bit_for_bit():
    rng = np.random.default_rng(29)
    cells = np.zeros(400, ra.GRADE_CELL_DTYPE)
    cells["n"] = rng.integers(1, 1 << 28, 400)
    cells["sl"] = rng.integers(-1020, 1021, 400) * cells["n"].astype(np.int64) // rng.integers(1, 50, 400)
    cells["sll"] = rng.integers(0, 1040401, 400) * cells["n"].astype(np.int64)
    cells[0] = (0, 0, 0, 0, 0, 0, 0, 0)
    cells[1] = (0, 0, 0, 0, 0, 0, 5, 25)      # n == 0 with sums: still 0
    cells[2] = (1 << 28, 0, 0, 0, 0, 0, -(1 << 28) * 1020, (1 << 28) * 1040400)
    cells[3] = (3, 0, 0, 0, 0, 0, 1, 1)
    for k, c in enumerate(cells):
        got, want = ra.grade_sharpness(c), grade.sharpness(c)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (k, c, got, want)
    assert ra.grade_sharpness(cells[0]) == 0.0 and ra.grade_sharpness(cells[1]) == 0.0 and ra.grade_sharpness(cells[2]) == 0.0
    assert ra.lib().rd_grade_sharpness(None) == 0.0


def test_percentile_bit_for_bit():
    rng = np.random.default_rng(31)
    hists = [rng.integers(0, 1000, 256).astype(np.uint32), np.zeros(256, np.uint32), np.full(256, 0xFFFFFFFF, np.uint32)]
    one = np.zeros(256, np.uint32)
    one[93] = 7
    sparse = np.zeros(256, np.uint32)
    sparse[[0, 10, 200, 255]] = (1, 50, 48, 1)
    hists += [one, sparse]
    for h in hists:
        for num, den in ((0, 100), (1, 100), (50, 100), (99, 100), (100, 100), (0, 1), (1, 1), (1, 3), (2, 3), (1 << 20, 1 << 20), (1, 1 << 20), (-1, 100), (101, 100), (1, 0), (1, -5), (1, (1 << 20) + 1)):
            assert ra.grade_percentile(h, num, den) == grade.percentile(h, num, den), (num, den)
    assert ra.grade_percentile(hists[1], 50) == -1, "the empty histogram"
    assert ra.grade_percentile(one, 0) == 0 and ra.grade_percentile(one, 1) == 93 and ra.grade_percentile(one, 100) == 93
    assert ra.grade_percentile(sparse, 1) == 0 and ra.grade_percentile(sparse, 2) == 10 and ra.grade_percentile(sparse, 99) == 200 and ra.grade_percentile(sparse, 100) == 255
    assert ra.lib().rd_grade_percentile(None, 1, 2) == -1


def test_the_sums_need_64_bits():
    s = ra.grade_spec(1)
    c = grade.cells_of(np.full((258, 258), 255, np.uint8), s)[0, 0]
    assert int(c["sgg"]) == 258 * 258 * 65025 == 4328324100 > 2 ** 32 and int(c["sg"]) == 258 * 258 * 255 and int(c["sl"]) == 0 == int(c["sll"]) and int(c["n"]) == int(c["hi"]) == 258 * 258
    yy, xx = np.mgrid[0:128, 0:64]
    c = grade.cells_of(np.where((xx + yy) & 1, 255, 0).astype(np.uint8), s)[0, 0]
    assert int(c["sll"]) > 2 ** 32 and int(c["sll"]) >= 62 * 126 * 1020 * 1020, "L = +-1020 in the interior"
    n = 16384 * 16384
    assert n == 2 ** 28 and n * 1040400 == 279280248422400 < 2 ** 63 and n < 2 ** 31
    txt = header()
    assert "279 280 248 422 400" in txt and "4 328 324 100" in txt


def text_page():
    """a 128 x 96 page of 4 x 4 cells: paper 220, strokes of ink 30 in the cells of the upper three cell rows - the bottom cell row is blank paper"""
    pw, ph = 128, 96
    G = np.full((ph, pw), 220, np.uint8)
    for y in range(4, 68, 6):
        for x in range(3, 125, 5):
            if (x * 7 + y * 3) % 11 < 8:
                G[y:y + 3, x:x + 2] = 30
    return G


def box_blur(G):
    P = np.pad(G.astype(np.int64), 1, mode="edge")
    s = sum(P[dy:dy + G.shape[0], dx:dx + G.shape[1]] for dy in range(3) for dx in range(3))
    return ((s + 4) // 9).astype(np.uint8)


def test_the_contract_ranks_frames_the_way_it_is_meant_to():
    G = text_page()
    spec = ra.grade_spec(4, 8, 247, 64, hist=True)
    page, _ = ra.grade_view(grade.quad_bytes(G, spec)[None], spec)
    blur, _ = ra.grade_view(grade.quad_bytes(box_blur(G), spec)[None], spec)
    ink = page[0]["lo"] + (page[0]["sg"] < 220 * page[0]["n"]) > 0      # cells that hold ink
    assert ink[:3].all() and not ink[3].any()
    for cy in range(4):
        for cx in range(4):
            a, b = ra.grade_sharpness(page[0, cy, cx]), ra.grade_sharpness(blur[0, cy, cx])
            if ink[cy, cx]:
                assert b < a, "the blurred page is strictly less sharp in a cell that holds ink: (%d, %d) %r %r" % (cx, cy, a, b)
            else:
                assert a == b == 0.0
    glare = G.copy()
    yy, xx = np.mgrid[0:96, 0:128]
    disc = (xx - 80) ** 2 + (yy - 36) ** 2 <= 9 ** 2      # inside cell (cx 2, cy 1): x 64 .. 95, y 24 .. 47
    assert disc[24:48, 64:96].sum() == disc.sum() > 200
    glare[disc] = 255
    gl, gh = ra.grade_view(grade.quad_bytes(glare, spec)[None], spec)
    assert not page[0]["hi"].any()
    for cy in range(4):
        for cx in range(4):
            assert int(gl[0, cy, cx]["hi"]) == (int(disc.sum()) if (cx, cy) == (2, 1) else 0), (cx, cy)
    assert ra.grade_percentile(gh[0], 1) == 30 and ra.grade_percentile(gh[0], 99) == 255      # what a scan spec's `white` can be taken from
    _, ph_ = ra.grade_view(grade.quad_bytes(G, spec)[None], spec)
    assert ra.grade_percentile(ph_[0], 99) == 220


def test_host_code_under_the_sanitizers_as_a_plain_process(tmp_path):
    """tests/native/grade_host_check.c with csrc/rd_grade_host.c, both compiled with -fsanitize=address,undefined, run as a process of its own"""
    csrc = os.path.join(helpers.ROOT, "rectdetect_amd", "csrc")
    exe = str(tmp_path / "grade_host_check")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-DCL_TARGET_OPENCL_VERSION=120", "-I", csrc, "-I", os.path.join(helpers.ROOT, "include"),
           os.path.join(helpers.ROOT, "tests", "native", "grade_host_check.c"), os.path.join(csrc, "rd_grade_host.c"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode != 0 and "sanitize" in p.stderr and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip("this compiler has no address / undefined sanitizer runtime: %s" % p.stderr[-200:])
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "grade_host_check: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
