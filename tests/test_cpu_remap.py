"""CPU tests of remapped frames (include/rectdetect_hip.h, "remapped frames"): the host functions - rd_remap_points, rd_remap_table_lens, rd_remap_table_map,
rd_view_tan_aov, rd_remap_limits - against the restatement of the header's text (tests/remap.py), bit for bit; the identity, a half-pixel map and the inside
rule at its edges against values worked out by hand; every argument error with a canary around the table; the host-only code under the sanitizers as a plain
process.  No GPU, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers
from tests import remap

SIZES = [(83, 59, 97, 61), (8, 8, 2, 2)]      # ow, oh, iw, ih


def cameras(name, ow, oh, iw, ih):
    """the lens and the view of a named case, scaled to the sizes: the lens looks through the middle of the source, the view through the middle of the output"""
    f = 0.6 * iw
    coef = {"barrel": dict(k1=-0.25), "pincushion": dict(k1=0.2, k2=0.05), "tangential": dict(k1=-0.12, k2=0.03, p1=0.011, p2=-0.007, k3=0.02),
            "zoom_out": dict(k1=-0.1), "zoom_in": dict(k1=-0.1)}[name]
    zoom = {"zoom_out": 0.45, "zoom_in": 6.0}.get(name, 1.0)
    lens = ra.lens(f, f * 1.01, (iw - 1) / 2 + 0.3, (ih - 1) / 2 - 0.2, **coef)
    view = ra.view(f * ow / iw * zoom, f * 1.01 * ow / iw * zoom, (ow - 1) / 2, (oh - 1) / 2)
    return lens, view


CASES = ["barrel", "pincushion", "tangential", "zoom_out", "zoom_in"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d_from_%dx%d" % s)
@pytest.mark.parametrize("name", CASES)
def test_tables_and_points_equal_the_restatement(name, size):
    ow, oh, iw, ih = size
    lens, view = cameras(name, ow, oh, iw, ih)
    got, n = ra.remap_table_lens(lens, view, ow, oh, iw, ih)
    want, wn = remap.table_lens(lens, view, ow, oh, iw, ih)
    assert got.dtype == np.int32 and got.shape == (oh, ow, 2)
    assert n == wn and np.array_equal(got, want), (name, size, n, wn)
    if name == "zoom_out":
        assert 0 < n < ow * oh
    if name == "zoom_in":
        assert n == ow * oh
    # the points of the grid and points between and beyond them, in every bit
    rng = np.random.default_rng(5)
    uv = np.concatenate([remap.grid(ow, oh), rng.uniform(-3.0, max(ow, oh) + 3.0, (500, 2))])
    assert np.array_equal(bits(ra.remap_points(lens, view, uv)), bits(remap.points(lens, view, uv))), (name, size)
    # the same table through float32 maps: the rounding to float32 is part of the contract
    XY = remap.points(lens, view, remap.grid(ow, oh)).astype(np.float32)
    gm, nm = ra.remap_table_map(XY[:, 0], XY[:, 1], ow, oh, iw, ih)
    wm, wnm = remap.table_map(XY[:, 0], XY[:, 1], ow, oh, iw, ih)
    assert nm == wnm and np.array_equal(gm, wm), (name, size)


def test_the_identity_is_exact():
    """fx = fy = 64, integer cx, cy, all coefficients 0, ow = iw, oh = ih: every operation of the map is exact, so xi = 256 u, yi = 256 v and apply returns the source"""
    iw, ih = 37, 23
    lens, view = ra.lens(64.0, 64.0, 18.0, 11.0), ra.view(64.0, 64.0, 18.0, 11.0)
    table, n = ra.remap_table_lens(lens, view, iw, ih, iw, ih)
    v, u = np.mgrid[0:ih, 0:iw]
    assert n == iw * ih and np.array_equal(table[..., 0], 256 * u) and np.array_equal(table[..., 1], 256 * v)
    src = np.random.default_rng(1).integers(0, 256, (ih, iw, 3), dtype=np.uint8)
    assert np.array_equal(remap.apply(src, table, iw, ih, (1, 2, 3)), src)


def test_a_half_pixel_map_averages_neighbours_and_loses_the_last_column():
    iw, ih = 9, 5
    v, u = np.mgrid[0:ih, 0:iw]
    table, n = ra.remap_table_map((u + 0.5).astype(np.float32), v.astype(np.float32), iw, ih, iw, ih)
    assert n == (iw - 1) * ih and (table[:, -1] == -1).all()
    assert np.array_equal(table[:, :-1, 0], 256 * u[:, :-1] + 128) and np.array_equal(table[:, :-1, 1], 256 * v[:, :-1])
    src = np.random.default_rng(2).integers(0, 256, (ih, iw, 3), dtype=np.uint8)
    out = remap.apply(src, table, iw, ih, (7, 8, 9))
    a, b = src[:, :-1].astype(np.int64), src[:, 1:].astype(np.int64)
    assert np.array_equal(out[:, :-1], (((a * 128 + b * 128) * 256 + 32768) >> 16).astype(np.uint8))
    assert (out[:, -1] == np.array([7, 8, 9], np.uint8)).all()


def test_the_inside_rule_at_its_edges():
    iw, ih = 6, 4
    f32 = np.float32
    last_x, last_y = f32(iw - 1), f32(ih - 1)
    tiny = np.nextafter(f32(0), f32(-1))      # the largest negative float
    assert tiny < 0 and tiny == -f32(1.401298464324817e-45)
    xs = [last_x, np.nextafter(last_x, f32(np.inf)), f32(-0.0), tiny, f32(np.nan), f32(np.inf), f32(-np.inf), f32(1.0), f32(1.0), f32(1.0), f32(1.0), f32(1.0), f32(0.0)]
    ys = [f32(1.0), f32(1.0), f32(1.0), f32(1.0), f32(1.0), f32(1.0), f32(1.0), last_y, np.nextafter(last_y, f32(np.inf)), f32(-0.0), tiny, f32(np.nan), f32(np.inf)]
    want = [(256 * (iw - 1), 256), (-1, -1), (0, 256), (-1, -1), (-1, -1), (-1, -1), (-1, -1), (256, 256 * (ih - 1)), (-1, -1), (256, 0), (-1, -1), (-1, -1), (-1, -1)]
    ow = len(xs)
    table, n = ra.remap_table_map(np.array(xs, f32), np.array(ys, f32), ow, 1, iw, ih)
    assert table.reshape(ow, 2).tolist() == [list(w) for w in want] and n == sum(w[0] >= 0 for w in want)
    wt, wn = remap.table_map(np.array(xs, f32), np.array(ys, f32), ow, 1, iw, ih)
    assert np.array_equal(table, wt) and n == wn
    # X = iw - 1 exactly: x1 is clamped, the output is the last column's pixel itself
    src = np.random.default_rng(3).integers(0, 256, (ih, iw, 3), dtype=np.uint8)
    out = remap.apply(src, table, ow, 1, (200, 100, 50))
    assert np.array_equal(out[0, 0], src[1, iw - 1]) and np.array_equal(out[0, 7], src[ih - 1, 1]) and np.array_equal(out[0, 2], src[1, 0])
    assert (out[0, [1, 3, 4, 5, 6, 8, 10, 11, 12]] == np.array([200, 100, 50], np.uint8)).all()
    # the same through a lens: a position that is not finite is outside (a view so narrow that the polynomial overflows)
    lens, view = ra.lens(1e300, 1e300, 0.0, 0.0, k1=1e300), ra.view(1e-300, 1e-300, 0.5, 0.5)
    table, n = ra.remap_table_lens(lens, view, 2, 2, iw, ih)
    assert n == 0 and (table == -1).all()
    assert np.array_equal(table, remap.table_lens(lens, view, 2, 2, iw, ih)[0])


def test_bad_arguments_return_minus_one_and_write_nothing():
    L = ra.lib()
    ow, oh, iw, ih = 5, 3, 7, 4
    CANARY = 0x5a5a5a5a
    buf = np.full(2 * ow * oh + 32, CANARY, np.int32)
    table = buf[16:].ctypes.data
    lens, view = ra.lens(4.0, 4.0, 3.0, 1.5, k1=-0.1), ra.view(4.0, 4.0, 2.0, 1.0)
    mx, my = np.zeros(ow * oh, np.float32), np.zeros(ow * oh, np.float32)
    lp, vp, mxp, myp = lens.ctypes.data, view.ctypes.data, mx.ctypes.data, my.ctypes.data

    def refused(r):
        assert r == -1 and (buf == CANARY).all()

    refused(L.rd_remap_table_lens(None, vp, ow, oh, iw, ih, table))
    refused(L.rd_remap_table_lens(lp, None, ow, oh, iw, ih, table))
    assert L.rd_remap_table_lens(lp, vp, ow, oh, iw, ih, None) == -1
    refused(L.rd_remap_table_map(None, myp, ow, oh, iw, ih, table))
    refused(L.rd_remap_table_map(mxp, None, ow, oh, iw, ih, table))
    assert L.rd_remap_table_map(mxp, myp, ow, oh, iw, ih, None) == -1
    for bad in ((0, oh, iw, ih), (ow, 0, iw, ih), (-1, oh, iw, ih), (16385, oh, iw, ih), (ow, 16385, iw, ih), (ow, oh, 0, ih), (ow, oh, iw, 0), (ow, oh, iw, -4),
                (ow, oh, 65537, ih), (ow, oh, iw, 65537)):
        refused(L.rd_remap_table_lens(lp, vp, *bad, table))
        refused(L.rd_remap_table_map(mxp, myp, *bad, table))
        with pytest.raises(ValueError):
            ra.remap_table_lens(lens, view, *bad)
    for field in ra.LENS_DTYPE.names:
        for v in (np.nan, np.inf, -np.inf):
            l = lens.copy()
            l[field] = v
            refused(L.rd_remap_table_lens(l.ctypes.data, vp, ow, oh, iw, ih, table))
    for field in ra.VIEW_DTYPE.names:
        for v in (np.nan, np.inf, -np.inf) + ((0.0, -0.0) if field in ("fx", "fy") else ()):
            w = view.copy()
            w[field] = v
            refused(L.rd_remap_table_lens(lp, w.ctypes.data, ow, oh, iw, ih, table))
    # ... and the good call writes exactly the table
    n = L.rd_remap_table_lens(lp, vp, ow, oh, iw, ih, table)
    assert n >= 0 and (buf[:16] == CANARY).all() and (buf[16 + 2 * ow * oh:] == CANARY).all()
    assert np.array_equal(buf[16:16 + 2 * ow * oh].reshape(oh, ow, 2), remap.table_lens(lens, view, ow, oh, iw, ih)[0])
    # the largest legal sizes are legal (a 1 x 1 output from the largest source)
    one = np.zeros(2, np.int32)
    assert L.rd_remap_table_lens(lp, vp, 1, 1, 65536, 65536, one.ctypes.data) in (0, 1)


def test_limits_tan_aov_and_the_records():
    assert ra.remap_limits() == {"min_out": 1, "max_out": 16384, "min_src": 1, "max_src": 65536}
    assert ra.LENS_DTYPE.itemsize == 72 and ra.VIEW_DTYPE.itemsize == 32
    assert ra.LENS_DTYPE.names == remap.LENS_FIELDS and ra.VIEW_DTYPE.names == remap.VIEW_FIELDS
    for ow, fx in ((1920, 1000.0), (1919, 1000.0), (83, 47.3), (1, 3.0), (640, -500.0)):
        v = ra.view(fx, fx, 0.0, 0.0)
        assert ra.view_tan_aov(v, ow) == float(np.float64(ow // 2) / np.float64(fx))
    assert ra.view_tan_aov(ra.view(960.0, 1.0, 0.0, 0.0), 1920) == 1.0 and ra.view_tan_aov(ra.view(960.0, 1.0, 0.0, 0.0), 1921) == 1.0


def test_the_header_lays_the_records_out_as_the_binding_does(tmp_path):
    src = '#include "rectdetect_hip.h"\n#include <stddef.h>\nint main(void) { return sizeof(rd_lens) == 72 && sizeof(rd_view) == 32 && offsetof(rd_lens, k1) == 32 && ' \
          'offsetof(rd_lens, p1) == 48 && offsetof(rd_lens, k3) == 64 && offsetof(rd_view, cx) == 16 ? 0 : 1; }\n'
    f, exe = tmp_path / "t.c", tmp_path / "t"
    f.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(helpers.ROOT, "include"), str(f), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    assert [ra.LENS_DTYPE.fields[n][1] for n in ("k1", "p1", "k3")] == [32, 48, 64] and ra.VIEW_DTYPE.fields["cx"][1] == 16


def test_host_code_under_the_sanitizers_as_a_plain_process(tmp_path):
    """tests/native/remap_host_check.c with csrc/rd_remap_host.c, both compiled with -fsanitize=address,undefined, run as a process of its own"""
    csrc = os.path.join(helpers.ROOT, "rectdetect_amd", "csrc")
    exe = str(tmp_path / "remap_host_check")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", csrc, "-I", os.path.join(helpers.ROOT, "include"), os.path.join(helpers.ROOT, "tests", "native", "remap_host_check.c"),
           os.path.join(csrc, "rd_remap_host.c"), "-o", exe, "-lm"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode != 0 and "sanitize" in p.stderr and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip("this compiler has no address / undefined sanitizer runtime: %s" % p.stderr[-200:])
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "remap_host_check: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
