"""Scanned pages without a GPU: the header's declarations and the library's exports, sizeof(rd_scan_spec) and its offsets, rd_scan_spec_ok on every side of every
bound, rd_scan_bytes, rd_scan_pixel against the restatement (tests/scan.py) for every G0 over a grid of windows, the int32 bound, the restatement's integral image
against counting, the host-only code under the sanitizers as a plain process - and that the contract does what it is for: on a page under a 3 : 1 illumination ramp
the ink map IS the stroke mask, which no global threshold reproduces.  No tolerance."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers
from tests import scan

FUNCTIONS = ("rd_scan_spec_ok", "rd_scan_bytes", "rd_scan_pixel", "rd_scan_limits", "rd_rectifier_create_scan")
CONSTANTS = {"RD_SCAN_FLAT": 0, "RD_SCAN_BILEVEL": 1, "RD_SCAN_BITS": 2}
FIELDS = ("mode", "radius", "k", "d", "white", "oversample", "invert", "reserved")
# per field: (legal values at its bounds, illegal values one past them)
BOUNDS = {"mode": ((0, 1, 2), (-1, 3)), "radius": ((1, 2, 62, 63), (0, 64, -1)), "k": ((0, 1, 254, 255), (-1, 256)), "d": ((0, 1, 254, 255), (-1, 256)),
          "white": ((1, 2, 254, 255), (0, 256, -1)), "oversample": ((1, 2, 4), (0, 3, 5, 8, -1)), "invert": ((0, 1), (-1, 2)), "reserved": ((0,), (1, -1))}


def header():
    return open(os.path.join(helpers.ROOT, "include", "rectdetect_hip.h")).read()


def test_header_declares_the_functions_and_constants():
    txt = header()
    for name, value in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), txt), name
        assert getattr(ra, name[3:]) == value
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    assert re.search(r"typedef struct \{ int32_t mode, radius, k, d, white, oversample, invert, reserved; \} rd_scan_spec;", txt)
    assert txt.index("model-ready tensors:") < txt.index("scanned pages:") < txt.index("annotated frames:")


def test_library_exports_the_functions():
    L = ctypes.CDLL(ra.LIB_PATH)
    missing = [n for n in FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_sizeof_the_spec_is_32(tmp_path):
    src = tmp_path / "t.c"
    checks = " && ".join("offsetof(rd_scan_spec, %s) == %d" % (f, 4 * k) for k, f in enumerate(FIELDS))
    src.write_text('#include <stddef.h>\n#include "rectdetect_hip.h"\nint main(void) { return sizeof(rd_scan_spec) == 32 && %s ? 0 : 1; }\n' % checks)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-DCL_TARGET_OPENCL_VERSION=120", "-I", os.path.join(helpers.ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    assert ra.SCAN_SPEC_DTYPE.itemsize == 32 and ra.SCAN_SPEC_DTYPE.names == FIELDS
    assert [ra.SCAN_SPEC_DTYPE.fields[f][1] for f in FIELDS] == [4 * k for k in range(8)]


def test_limits():
    lim = ra.scan_limits()
    assert lim["modes"] == scan.MODES and lim["oversamplings"] == (1, 2, 4) and lim["max_radius"] == 63
    assert lim["tile_w"] >= 64 and lim["tile_w"] % 64 == 0 and lim["tile_h"] >= 1
    a = np.full(10, -7, np.int32)
    ra.lib().rd_scan_limits(a.ctypes.data + 4)
    assert a[0] == a[9] == -7 and a[6:9].tolist() == [0, 0, 0]


def test_the_default_spec():
    s = ra.scan_spec(ra.SCAN_BITS)
    assert [int(s[f]) for f in FIELDS] == [2, 15, 26, 0, 230, 1, 0, 0]
    assert int(ra.scan_spec(ra.SCAN_FLAT, invert=True)["invert"]) == 1


def test_spec_ok_on_every_side_of_every_bound():
    ok = ra.scan_spec(ra.SCAN_BILEVEL, 15, 26, 3, 230, 2, True)
    assert ra.scan_spec_ok(ok, 128, 96)
    for field, (legal, illegal) in BOUNDS.items():
        for v in legal:
            s = ok.copy()
            s[field] = v
            assert ra.scan_spec_ok(s, 128, 96), (field, v)
            assert ra.scan_bytes(s, 128, 96) > 0
        for v in illegal:
            s = ok.copy()
            s[field] = v
            assert not ra.scan_spec_ok(s, 128, 96), (field, v)
            assert ra.scan_bytes(s, 128, 96) == 0
    for m in (1, 2, 4):
        s = ok.copy()
        s["oversample"] = m
        assert ra.scan_spec_ok(s, 16384 // m, 16384 // m) and ra.scan_spec_ok(s, 16384 // m - 1, 1) and ra.scan_spec_ok(s, 1, 1)
        assert not ra.scan_spec_ok(s, 16384 // m + 1, 8) and not ra.scan_spec_ok(s, 8, 16384 // m + 1)
        assert not ra.scan_spec_ok(s, 0, 8) and not ra.scan_spec_ok(s, 8, 0) and not ra.scan_spec_ok(s, -1, 8)
    assert ra.lib().rd_scan_spec_ok(None, 8, 8) == 0 and ra.lib().rd_scan_bytes(None, 8, 8) == 0


def test_bytes_for_the_three_modes():
    for pw in (1, 7, 8, 9):
        for ph in (1, 5):
            for m in (1, 4):
                assert ra.scan_bytes(ra.scan_spec(ra.SCAN_FLAT, oversample=m), pw, ph) == pw * ph
                assert ra.scan_bytes(ra.scan_spec(ra.SCAN_BILEVEL, oversample=m), pw, ph) == pw * ph
                bits = ra.scan_spec(ra.SCAN_BITS, oversample=m)
                assert ra.scan_bytes(bits, pw, ph) == {1: 1, 7: 1, 8: 1, 9: 2}[pw] * ph
                for s in (bits, ra.scan_spec(ra.SCAN_FLAT)):
                    assert int(np.prod(scan.shape(s, 1, pw, ph))) == ra.scan_bytes(s, pw, ph)


def window_grid():
    """(N, T) pairs: N from 1 to 127^2, T = 0, 1, sixteenths of 255 N, 255 N - 1 and 255 N"""
    out = []
    for N in (1, 2, 9, 25, 289, 961, 4096, 16128, 127 * 127):
        for T in sorted({0, 1, 255 * N - 1, 255 * N} | {255 * N * t // 16 for t in range(17)}):
            out.append((N, T))
    return out


@pytest.mark.parametrize("invert", [0, 1])
def test_pixel_equals_the_restatement_for_every_gray_value(invert):
    L = ra.lib()
    G0 = np.arange(256)
    G = 255 - G0 if invert else G0
    ink, flat = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    inks = equal = capped = 0
    for k in (0, 26, 255):
        for d in (0, 26, 255):
            for n, (N, T) in enumerate(window_grid()):
                spec = ra.scan_spec(ra.SCAN_BITS, 63, k, d, (1, 230, 255)[n % 3], 1, invert)
                wink, wflat = scan.decide(spec, G, N, T)
                got = np.zeros((256, 2), np.int64)
                for g in range(256):
                    assert L.rd_scan_pixel(spec.ctypes.data, g, N, T, ink.ctypes.data, flat.ctypes.data) == 1
                    got[g] = ink[0], flat[0]
                assert np.array_equal(got[:, 0], wink.astype(np.int64)) and np.array_equal(got[:, 1], wflat), (scan.name(spec), N, T)
                inks += int(wink.sum())
                equal += int((256 * N * (G + d) == (256 - k) * T).sum())
                capped += int((wflat == 255).sum())
                if T == 0:
                    assert not wink.any() and (wflat == int(spec["white"])).all(), "an all-zero window has no ink and is white"
                if k == 0 and d == 0 and T % N == 0:
                    assert not wink[G == T // N].any() and (wflat[G == T // N] == int(spec["white"])).all(), "a pixel equal to its neighbourhood's mean"
    assert inks > 1000 and equal > 10 and capped > 1000, (inks, equal, capped)      # the sweep met what it was built to meet


def test_pixel_refuses_bad_arguments():
    spec = ra.scan_spec(ra.SCAN_FLAT)
    assert ra.scan_pixel(spec, 10, 4, 400) == (1, 23)
    for bad in (dict(G0=-1), dict(G0=256), dict(N=0), dict(N=127 * 127 + 1), dict(T=-1), dict(T=4 * 255 + 1), dict(k=256), dict(d=-1), dict(white=0), dict(invert=2)):
        s = spec.copy()
        args = dict(G0=10, N=4, T=400)
        for key, v in bad.items():
            if key in args:
                args[key] = v
            else:
                s[key] = v
        with pytest.raises(ValueError):
            ra.scan_pixel(s, **args)
    out = np.full(2, 0xA5, np.uint8)
    assert ra.lib().rd_scan_pixel(None, 1, 1, 1, out.ctypes.data, out.ctypes.data + 1) == 0 and out.tolist() == [0xA5, 0xA5]


def test_the_largest_term_fits_int32():
    N, G, d = 127 * 127, 255, 255
    assert 256 * N * (G + d) == 2105802240 < 2 ** 31
    assert 255 * N * 255 + (255 * N >> 1) < 2 ** 31 and 256 * 255 * N < 2 ** 31
    spec = ra.scan_spec(ra.SCAN_BITS, 63, 0, 255)
    assert ra.scan_pixel(spec, 255, N, 255 * N) == (0, 230)      # 2 105 802 240 < 256 * 255 * 16129 is false: no wrap-around made it true
    assert "2 105 802 240" in header()


def test_restated_window_equals_counting():
    rng = np.random.default_rng(11)
    for pw, ph, r in ((1, 1, 1), (7, 3, 1), (9, 5, 2), (13, 11, 8), (20, 6, 63)):
        G = rng.integers(0, 256, (ph, pw))
        N, T = scan.window(G, r)
        bN, bT = scan.brute(G, r)
        assert np.array_equal(N, bN) and np.array_equal(T, bT), (pw, ph, r)
    bits = scan.page(np.array([[0] * 9 + [255] * 2], np.int64).repeat(3, 0), ra.scan_spec(ra.SCAN_BITS, 2, 26, 0))
    assert bits.shape == (3, 2) and (bits[:, 1] & 0x1F == 0).all(), "pad bits are 0"


def ramp_page():
    """a 128 x 96 page under a 3 : 1 illumination ramp with vertical and horizontal strokes of 45 % reflectance: (the page, the stroke mask)"""
    pw, ph = 128, 96
    bg = np.broadcast_to(80 + (160 * np.arange(pw)) // 127, (ph, pw))
    mask = np.zeros((ph, pw), bool)
    for x in range(6, 122, 12):
        mask[8:88, x:x + 3] = True
    for y in range(10, 86, 20):
        mask[y:y + 2, 4:124] = True
    return np.where(mask, (bg * 45) // 100, bg).astype(np.uint8), mask


def test_the_contract_separates_ink_from_paper_where_no_global_threshold_can():
    G, mask = ramp_page()
    assert G[~mask].min() == 80 and G[~mask].max() == 240 and mask.sum() > 1000
    for r, k, d in ((4, 26, 0), (8, 26, 0), (8, 38, 0), (15, 26, 4)):
        for mode in (ra.SCAN_BILEVEL, ra.SCAN_BITS):
            out = scan.page(G, ra.scan_spec(mode, r, k, d))
            ink = out == 0 if mode == ra.SCAN_BILEVEL else np.unpackbits(out, axis=1, bitorder="big")[:, :128].astype(bool)
            assert np.array_equal(ink, mask), (r, k, d, int((ink != mask).sum()))
    for t in range(256):
        assert not np.array_equal(G < t, mask) and not np.array_equal(G <= t, mask), t
    F = scan.page(G, ra.scan_spec(ra.SCAN_FLAT, 8, white=230))
    assert 222 <= F[~mask].min() and F[~mask].max() <= 255, (F[~mask].min(), F[~mask].max())
    assert 107 <= F[mask].min() and F[mask].max() <= 136, (F[mask].min(), F[mask].max())
    inv = scan.page(255 - G, ra.scan_spec(ra.SCAN_BILEVEL, 8, 26, 0, invert=True))      # light ink on a dark page, inverted: the same page
    assert np.array_equal(inv == 0, mask)


def test_host_code_under_the_sanitizers_as_a_plain_process(tmp_path):
    """tests/native/scan_host_check.c with csrc/rd_scan_host.c, both compiled with -fsanitize=address,undefined, run as a process of its own"""
    csrc = os.path.join(helpers.ROOT, "rectdetect_amd", "csrc")
    exe = str(tmp_path / "scan_host_check")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-DCL_TARGET_OPENCL_VERSION=120", "-I", csrc, "-I", os.path.join(helpers.ROOT, "include"),
           os.path.join(helpers.ROOT, "tests", "native", "scan_host_check.c"), os.path.join(csrc, "rd_scan_host.c"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode != 0 and "sanitize" in p.stderr and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip("this compiler has no address / undefined sanitizer runtime: %s" % p.stderr[-200:])
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "scan_host_check: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
