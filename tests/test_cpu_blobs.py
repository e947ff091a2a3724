"""Page components without a GPU: the header's declarations and the library's exports, the sizes of the three structs, rd_blob_spec_ok on both sides of every bound,
rd_blob_bytes, the restatement (tests/blobs.py) against flooding pixel by pixel, every crafted case's own claim (tests/blobcases.py), rd_blob_page_host against the
restatement byte for byte on the whole catalogue and on random masks - and against scipy.ndimage.label where scipy is there -, and the host-only code under the
sanitizers as a plain process.  No tolerance."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import blobcases
from tests import blobs
from tests import helpers

FUNCTIONS = ("rd_blob_spec_ok", "rd_blob_bytes", "rd_blob_limits", "rd_blob_page_host", "rd_rectifier_create_blobs", "rd_blobs_pages_device")
FIELDS = ("radius", "k", "d", "oversample", "invert", "connectivity", "min_area", "max_area", "max_blobs", "page")
# per field: (legal values at its bounds, illegal values one past them), for a spec with radius 15, min_area 4 and max_area 100
BOUNDS = {"radius": ((0, 1, 62, 63), (-1, 64)), "k": ((0, 1, 254, 255), (-1, 256)), "d": ((0, 1, 254, 255), (-1, 256)), "oversample": ((1, 2, 4), (0, 3, 5, 8, -1)),
          "invert": ((0, 1), (-1, 2)), "connectivity": ((4, 8), (0, 3, 5, 6, 7, 9, -4)), "min_area": ((1, 2, 99, 100), (0, -1, 101, (1 << 22) + 1)),
          "max_area": ((0, 4, 5, 1 << 22), (-1, 1, 3, (1 << 22) + 1)), "max_blobs": ((1, 2, 4095, 4096), (0, -1, 4097)), "page": ((0, 1), (-1, 2))}
CASES = blobcases.cases()


def header():
    return open(os.path.join(helpers.ROOT, "include", "rectdetect_hip.h")).read()


def test_header_declares_the_functions_and_structs():
    txt = header()
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    assert re.search(r"typedef struct \{ int32_t radius, k, d, oversample, invert, connectivity, min_area, max_area, max_blobs, page, reserved\[2\]; \} rd_blob_spec;", txt)
    assert re.search(r"typedef struct \{ int32_t ink, all, found, written, ink_kept, largest, flags, reserved; \} rd_blob_head;", txt)
    assert re.search(r"typedef struct \{ int32_t x0, y0, x1, y1, area, first; int64_t sx, sy; \} rd_blob;", txt)
    assert re.search(r"#define\s+RD_BLOB_OVERFLOW\s+1\b", txt) and ra.BLOB_OVERFLOW == 1
    assert txt.index("decoded quads:") < txt.index("page components:") < txt.index("annotated frames:")


def test_library_exports_the_functions():
    L = ctypes.CDLL(ra.LIB_PATH)
    missing = [n for n in FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_sizes_and_offsets_of_the_structs(tmp_path):
    src = tmp_path / "t.c"
    checks = ["sizeof(rd_blob_spec) == 48", "sizeof(rd_blob_head) == 32", "sizeof(rd_blob) == 40", "offsetof(rd_blob_spec, reserved) == 40", "offsetof(rd_blob, sx) == 24", "offsetof(rd_blob, sy) == 32"]
    checks += ["offsetof(rd_blob_spec, %s) == %d" % (f, 4 * k) for k, f in enumerate(FIELDS)]
    checks += ["offsetof(rd_blob_head, %s) == %d" % (f, 4 * k) for k, f in enumerate(blobs.HEAD.names)]
    checks += ["offsetof(rd_blob, %s) == %d" % (f, 4 * k) for k, f in enumerate(blobs.REC.names[:6])]
    src.write_text('#include <stddef.h>\n#include "rectdetect_hip.h"\nint main(void) { return %s ? 0 : 1; }\n' % " && ".join(checks))
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-DCL_TARGET_OPENCL_VERSION=120", "-I", os.path.join(helpers.ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    assert ra.BLOB_SPEC_DTYPE.itemsize == 48 and ra.BLOB_SPEC_DTYPE.names == FIELDS + ("reserved",)
    assert ra.BLOB_HEAD_DTYPE == blobs.HEAD and ra.BLOB_DTYPE == blobs.REC


def test_limits():
    lim = ra.blob_limits()
    assert lim["connectivities"] == (4, 8) and lim["oversamplings"] == (1, 2, 4) and lim["max_radius"] == 63 and lim["max_blobs"] == 4096 and lim["max_pixels"] == 1 << 22
    assert lim["tile_w"] >= 64 and lim["tile_w"] % 64 == 0 and lim["tile_h"] >= 1
    a = np.full(10, -7, np.int32)
    ra.lib().rd_blob_limits(a.ctypes.data + 4)
    assert a[0] == a[9] == -7 and a[8] == 0


def test_the_default_spec():
    s = ra.blob_spec()
    assert [int(s[f]) for f in FIELDS] == [15, 26, 0, 1, 0, 8, 1, 0, 256, 0] and s["reserved"].tolist() == [0, 0]
    assert ra.blob_spec_ok(s, 128, 128) and int(ra.blob_spec(invert=True, page=True)["page"]) == 1


def test_spec_ok_on_both_sides_of_every_bound():
    ok = ra.blob_spec(15, 26, 3, 2, True, 4, 4, 100, 64, True)
    assert ra.blob_spec_ok(ok, 128, 96)
    for field, (legal, illegal) in BOUNDS.items():
        for v in legal + illegal:
            s = ok.copy()
            s[field] = v
            if field == "radius" and v == 0:
                s["d"] = 0
            assert ra.blob_spec_ok(s, 128, 96) == (v in legal), (field, v)
            assert (ra.blob_bytes(s, 128, 96) > 0) == (v in legal), (field, v)
    for k in range(2):
        s = ok.copy()
        s["reserved"][k] = 1
        assert not ra.blob_spec_ok(s, 128, 96)
    level = ra.blob_spec(radius=0, k=100, d=1)      # a fixed level has no d
    assert not ra.blob_spec_ok(level, 16, 16)
    level["d"] = 0
    assert ra.blob_spec_ok(level, 16, 16)
    assert not ra.lib().rd_blob_spec_ok(None, 16, 16) and ra.lib().rd_blob_bytes(None, 16, 16) == 0
    # the page's own bounds: sides under the oversampling, and pw * ph
    for m, side in ((1, 16384), (2, 8192), (4, 4096)):
        s = ra.blob_spec(oversample=m)
        assert ra.blob_spec_ok(s, side, 4) and ra.blob_spec_ok(s, 4, side) and not ra.blob_spec_ok(s, side + 1, 4) and not ra.blob_spec_ok(s, 4, side + 1)
    s = ra.blob_spec()
    assert ra.blob_spec_ok(s, 2048, 2048) and ra.blob_spec_ok(s, 16384, 256) and not ra.blob_spec_ok(s, 2048, 2049) and not ra.blob_spec_ok(s, 16384, 257)
    assert not ra.blob_spec_ok(s, 0, 4) and not ra.blob_spec_ok(s, 4, 0) and not ra.blob_spec_ok(s, -1, 4)


def test_bytes():
    for pw, ph in ((1, 1), (7, 3), (8, 8), (9, 5), (64, 1), (65, 2), (129, 130), (2048, 2048)):
        for B in (1, 64, 4096):
            for page in (False, True):
                s = ra.blob_spec(max_blobs=B, page=page)
                want = 32 + 40 * B + ((((pw + 7) // 8 * ph + 7) // 8 * 8) if page else 0)
                assert ra.blob_bytes(s, pw, ph) == want == blobs.nbytes(s, pw, ph) and want % 8 == 0


@pytest.mark.parametrize("connectivity", (4, 8))
def test_restated_components_equal_flooding(connectivity):
    rng = np.random.default_rng(5)
    for pw, ph, density in ((1, 1, 1.0), (7, 3, 0.5), (9, 9, 0.6), (20, 13, 0.45), (33, 17, 0.6), (40, 11, 0.8)):
        m = rng.random((ph, pw)) < density
        recs = blobs.components(m, connectivity)[0]
        got = [tuple(int(r[f]) for f in ("area", "first", "x0", "y0", "x1", "y1", "sx", "sy")) for r in recs]
        assert got == blobs.brute(m, connectivity)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_every_case_shows_what_it_was_built_for(case):
    blobcases.check(case)


def test_the_catalogue_covers_the_issue():
    names = {c.name for c in CASES}
    for n in ("empty", "corners", "full", "size", "checker", "checker-overflow", "diagonal", "antidiagonal", "comb-joined-at-the-bottom", "comb-joined-at-the-top",
              "spiral", "two-spirals", "filter", "capacity", "pad-bits", "int64-sums", "many-components"):
        assert n in names, n
    TW, TH = blobcases.TW, blobcases.TH
    sizes = {(c.pw, c.ph) for c in CASES if c.name == "size"}
    assert sizes == {(1, 1), (7, 3), (64, 1), (65, 2), (TW, TH), (TW + 1, TH + 1), (2 * TW + 3, 3 * TH - 1)}
    assert {(int(c.spec["max_blobs"]), int(c.mask.sum()) - int(c.spec["max_blobs"])) for c in CASES if c.name == "capacity"} == {(B, e) for B in (1, 64, 4096) for e in (-1, 0, 1)}
    assert all(c.pw >= 3 * TW and c.ph >= 3 * TH for c in CASES if "spiral" in c.name)
    assert {c.pw for c in CASES if c.name == "pad-bits"} == {1, 7, 9}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_page_host_equals_the_restatement(case):
    got = ra.blob_page_host(case.bits, case.pw, case.ph, case.spec)
    blobs.explain(got, blobcases.want(case), case.spec, case.pw, case.ph, repr(case))


def test_page_host_equals_the_restatement_on_random_masks():
    rng = np.random.default_rng(77)
    for trial in range(150):
        pw, ph = int(rng.integers(1, 140)), int(rng.integers(1, 70))
        m = rng.random((ph, pw)) < rng.random()
        lo = int(rng.integers(1, 6))
        spec = ra.blob_spec(connectivity=int(rng.choice([4, 8])), min_area=lo, max_area=int(rng.choice([0, lo, lo + 7])), max_blobs=int(rng.choice([1, 3, 64])), page=bool(rng.integers(0, 2)))
        blobs.explain(ra.blob_page_host(blobs.pack(m), pw, ph, spec), blobs.page(m, spec), spec, pw, ph, "trial %d (%d x %d, %s)" % (trial, pw, ph, blobs.name(spec)))


def test_page_host_refuses_bad_arguments():
    s, bits = ra.blob_spec(max_blobs=1), np.full(8, 0xff, np.uint8)
    out = np.full(16, 0xA5A5A5A5A5A5A5A5, np.uint64)
    L = ra.lib()
    assert L.rd_blob_page_host(bits.ctypes.data, 8, 8, s.ctypes.data, out.ctypes.data) == 1 and out[0] != 0xA5A5A5A5A5A5A5A5 and out[9] == 0xA5A5A5A5A5A5A5A5
    out[:] = 0xA5A5A5A5A5A5A5A5
    bad = ra.blob_spec(max_blobs=0)
    for args in ((None, 8, 8, s.ctypes.data, out.ctypes.data), (bits.ctypes.data, 8, 8, None, out.ctypes.data), (bits.ctypes.data, 8, 8, s.ctypes.data, None),
                 (bits.ctypes.data, 8, 8, s.ctypes.data, out.ctypes.data + 4), (bits.ctypes.data, 0, 8, s.ctypes.data, out.ctypes.data), (bits.ctypes.data, 8, 8, bad.ctypes.data, out.ctypes.data)):
        assert L.rd_blob_page_host(*args) == 0
    assert np.all(out == 0xA5A5A5A5A5A5A5A5)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_counts_and_areas_equal_scipy(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    for case in CASES:
        if int(case.spec["connectivity"]) != connectivity or not blobcases.SMALL(case):
            continue
        lab, count = ndimage.label(case.mask, structure)
        s = case.spec.copy()
        s["min_area"], s["max_area"], s["max_blobs"] = 1, 0, 4096
        heads, recs, _ = blobs.view(ra.blob_page_host(case.bits, case.pw, case.ph, s), s, case.pw, case.ph)
        assert int(heads[0]["all"]) == count, case
        if count <= 4096:
            assert sorted(recs[0][:count]["area"].tolist()) == sorted(np.bincount(lab.reshape(-1))[1:].tolist()), case


def test_host_code_under_the_sanitizers_as_a_plain_process(tmp_path):
    """tests/native/blob_host_check.c with csrc/rd_blob_host.c, both compiled with -fsanitize=address,undefined, run as a process of its own"""
    csrc = os.path.join(helpers.ROOT, "rectdetect_amd", "csrc")
    exe = str(tmp_path / "blob_host_check")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-DCL_TARGET_OPENCL_VERSION=120", "-I", csrc, "-I", os.path.join(helpers.ROOT, "include"),
           os.path.join(helpers.ROOT, "tests", "native", "blob_host_check.c"), os.path.join(csrc, "rd_blob_host.c"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode != 0 and "sanitize" in p.stderr and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip("this compiler has no address / undefined sanitizer runtime: %s" % p.stderr[-200:])
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "blob_host_check: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
