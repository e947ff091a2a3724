"""rd_detector_enqueue_planes without a GPU: the header's declaration and constants, the exported symbol, the numpy restatement of the conversion
contract against hand-computed values, and the YUV4MPEG2 layout examples/rdy4m reads."""
import os
import re
import subprocess

import numpy as np

import rectdetect_amd as ra
from tests import helpers
from tests import pixfmt

HEADER = os.path.join(helpers.ROOT, "include", "rectdetect_hip.h")


def test_header_declares_formats_and_entry():
    src = open(HEADER).read()
    want = {"RD_PIX_BGR": 0, "RD_PIX_RGB": 1, "RD_PIX_BGRA": 2, "RD_PIX_RGBA": 3, "RD_PIX_NV12": 4, "RD_PIX_I420": 5}
    for name, v in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, src)
        assert m and int(m.group(1)) == v, name
    assert re.search(r"long\s+rd_detector_enqueue_planes\s*\(\s*rd_detector\s*\*\s*d\s*,\s*int\s+format\s*,\s*const\s+void\s*\*\s*const\s+planes\[3\]\s*,"
                     r"\s*const\s+int\s+pitches\[3\]\s*,\s*int\s+on_device\s*\)\s*;", src)
    assert [ra.PIX_BGR, ra.PIX_RGB, ra.PIX_BGRA, ra.PIX_RGBA, ra.PIX_NV12, ra.PIX_I420] == list(range(6))


def test_library_exports_enqueue_planes():
    out = subprocess.run(["nm", "-D", "--defined-only", ra.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\sT rd_detector_enqueue_planes$", out, re.M)
    assert ra.lib().rd_detector_enqueue_planes


def test_formula_anchors():
    bgr = lambda y, u, v: tuple(int(c) for c in pixfmt.yuv2bgr(y, u, v))
    assert bgr(16, 128, 128) == (0, 0, 0)
    assert bgr(235, 128, 128) == (255, 255, 255)
    for y in range(16):      # below black clamps to black
        assert bgr(y, 128, 128) == (0, 0, 0)
    assert bgr(255, 128, 128) == (255, 255, 255)
    # mid grey: (126 - 16) * 1220542 / 2^20 = 128.04
    assert bgr(126, 128, 128) == (128, 128, 128)
    # extreme chroma saturates: U = 255 drives B up, U = 0 drives it to 0; V likewise for R
    b, g, r = bgr(128, 255, 128)
    assert b == 255 and r == 130
    b, g, r = bgr(128, 0, 128)
    assert b == 0 and r == 130
    b, g, r = bgr(128, 128, 255)
    assert r == 255 and b == 130
    b, g, r = bgr(128, 128, 0)
    assert r == 0 and b == 130
    assert bgr(235, 255, 255)[0] == 255 and bgr(235, 255, 255)[2] == 255 and bgr(16, 0, 0)[1] == (852492 * 128 + 409993 * 128 + (1 << 19)) >> 20 == 154
    # the formula by hand for one interior triple: Y 100, U 90, V 160
    yy = (100 - 16) * 1220542
    assert bgr(100, 90, 160) == (max(0, (yy + 2116026 * -38 + (1 << 19)) >> 20), (yy - 852492 * 32 - 409993 * -38 + (1 << 19)) >> 20, (yy + 1673527 * 32 + (1 << 19)) >> 20)


def test_formula_whole_range_is_int32_safe():
    Y, U, V = np.meshgrid(np.arange(256), np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij")
    b64 = pixfmt.yuv2bgr(Y.astype(np.int64), U.astype(np.int64), V.astype(np.int64))
    b32 = pixfmt.yuv2bgr(Y, U, V)
    for a, c in zip(b32, b64):
        assert np.array_equal(a, c)


def test_converted_planes_have_the_contract_layouts():
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (6, 10, 3), dtype=np.uint8)
    (y, uv), ref = pixfmt.convert(bgr, ra.PIX_NV12)
    assert y.shape == (6, 10) and uv.shape == (3, 10)
    (y2, u, v), ref2 = pixfmt.convert(bgr, ra.PIX_I420)
    assert u.shape == v.shape == (3, 5) and np.array_equal(uv[:, 0::2], u) and np.array_equal(uv[:, 1::2], v) and np.array_equal(ref, ref2)
    assert ref[1, 3].tolist() == list(pixfmt.yuv2bgr(y[1, 3], u[0, 1], v[0, 1]))      # 2x2 nearest chroma
    (rgba,), ref = pixfmt.convert(bgr, ra.PIX_RGBA)
    assert rgba.shape == (6, 10, 4) and np.array_equal(rgba[..., 2::-1], bgr) and ref is bgr
    (rgb,), _ = pixfmt.convert(bgr, ra.PIX_RGB)
    assert np.array_equal(rgb[..., ::-1], bgr)


def test_y4m_layout(tmp_path):
    rng = np.random.default_rng(5)
    iw, ih = 20, 14
    frames = [tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((ih, iw), (ih // 2, iw // 2), (ih // 2, iw // 2))) for _ in range(3)]
    path = str(tmp_path / "a.y4m")
    pixfmt.write_y4m(path, frames, iw, ih)
    raw = open(path, "rb").read()
    head = raw.split(b"\n", 1)[0].split()
    assert head[0] == b"YUV4MPEG2" and b"W20" in head and b"H14" in head and b"C420jpeg" in head
    assert len(raw) == len(raw.split(b"\n", 1)[0]) + 1 + 3 * (len(b"FRAME\n") + iw * ih * 3 // 2)
    w, h, back = pixfmt.read_y4m(path)
    assert (w, h) == (iw, ih) and len(back) == 3
    for a, b in zip(frames, back):
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    src = open(os.path.join(helpers.ROOT, "examples", "rdy4m.c")).read()
    assert "RD_PIX_I420" in src and "rd_detector_enqueue_planes" in src and '"C420"' in src
    assert os.access(os.path.join(helpers.ROOT, "examples", "rdy4m"), os.X_OK)


def test_rdy4m_refuses_other_sample_layouts(tmp_path):
    """only 8-bit 4:2:0 streams: a C420p10 stream (16-bit samples, what ffmpeg writes for 10-bit sources) or 4:2:2 is refused from its header, before any frame is read"""
    exe = os.path.join(helpers.ROOT, "examples", "rdy4m")
    for tag in ("C420p10", "C420p12", "C422", "C444", "Cmono"):
        path = str(tmp_path / ("%s.y4m" % tag))
        with open(path, "wb") as f:
            f.write(("YUV4MPEG2 W16 H16 F30:1 %s\nFRAME\n" % tag).encode() + bytes(16 * 16 * 4))
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "only 8-bit 4:2:0" in r.stderr and "frame " not in r.stdout, (tag, r.returncode, r.stderr)
    src = open(os.path.join(helpers.ROOT, "examples", "rdy4m.c")).read()
    for tag in ("C420", "C420jpeg", "C420paldv", "C420mpeg2"):
        assert '"%s"' % tag in src
