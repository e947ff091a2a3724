"""Rectified patches for the tests: the contract of include/rectdetect_hip.h ("rectified patches") restated in numpy float64, written from the header's text
and not from the kernel - coefficients, validity, the per-pixel map, the 8.8 fixed-point bilinear blend.  Frames in the other pixel formats go through the
conversion contract of tests/pixfmt.py first: the header says that the patch from such a frame equals the patch from the BGR frame the contract gives for it."""
import math

import numpy as np

import rectdetect_amd as ra
from tests import pixfmt


def valid(quad):
    """strictly convex in either orientation, all eight values finite"""
    p = [(float(x), float(y)) for x, y in np.asarray(quad, np.float64).reshape(4, 2)]
    if not all(math.isfinite(v) for c in p for v in c):
        return False
    cr = []
    for i in range(4):
        (xa, ya), (xb, yb), (xc, yc) = p[i], p[(i + 1) % 4], p[(i + 2) % 4]
        cr.append((xb - xa) * (yc - yb) - (yb - ya) * (xc - xb))
    return all(c > 0 for c in cr) or all(c < 0 for c in cr)


def coefficients(quad):
    """(a, b, c, d, e, f, g, h as float64[8], status); zeros and 0 for an invalid quad.  Python floats are IEEE doubles and nothing here is contracted."""
    if not valid(quad):
        return np.zeros(8, np.float64), 0
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(float(x), float(y)) for x, y in np.asarray(quad, np.float64).reshape(4, 2)]
    dx1 = x1 - x2; dx2 = x3 - x2; sx = ((x0 - x1) + x2) - x3
    dy1 = y1 - y2; dy2 = y3 - y2; sy = ((y0 - y1) + y2) - y3
    den = dx1 * dy2 - dx2 * dy1
    g = (sx * dy2 - dx2 * sy) / den
    h = (dx1 * sy - sx * dy1) / den
    a = (x1 - x0) + g * x1; b = (x3 - x0) + h * x3; c = x0
    d = (y1 - y0) + g * y1; e = (y3 - y0) + h * y3; f = y0
    co = np.array([a, b, c, d, e, f, g, h], np.float64)
    if not np.isfinite(co).all():
        return np.zeros(8, np.float64), 0
    return co, 1


def _fix8(v, size):
    """floor(v * 256) clamped in double to [0, (size - 1) * 256] (anything not above 0, a NaN too: 0), then an integer"""
    q = np.floor(v * 256.0)
    q = np.where(q > 0.0, q, 0.0)
    q = np.where(q < (size - 1) * 256.0, q, (size - 1) * 256.0)
    return q.astype(np.int64)


def patch(bgr, quad, pw, ph):
    """the (ph, pw, 3) uint8 patch of one quad from an (ih, iw, 3) BGR image, and the quad's status"""
    co, status = coefficients(quad)
    if not status:
        return np.zeros((ph, pw, 3), np.uint8), 0
    ih, iw = bgr.shape[:2]
    a, b, c, d, e, f, g, h = (np.float64(v) for v in co)
    s = ((np.arange(pw, dtype=np.float64) + 0.5) / np.float64(pw))[None, :]
    t = ((np.arange(ph, dtype=np.float64) + 0.5) / np.float64(ph))[:, None]
    with np.errstate(all="ignore"):
        w = (g * s + h * t) + 1.0
        x = ((a * s + b * t) + c) / w
        y = ((d * s + e * t) + f) / w
        xi, yi = _fix8(x, iw), _fix8(y, ih)
    x0, fx = xi >> 8, (xi & 255)[..., None]
    y0, fy = yi >> 8, (yi & 255)[..., None]
    x1, y1 = np.minimum(x0 + 1, iw - 1), np.minimum(y0 + 1, ih - 1)
    p = bgr.astype(np.int64)
    top = p[y0, x0] * (256 - fx) + p[y0, x1] * fx
    bot = p[y1, x0] * (256 - fx) + p[y1, x1] * fx
    return ((top * (256 - fy) + bot * fy + 32768) >> 16).astype(np.uint8), 1


def patches(bgr, quads, pw, ph):
    """((n, ph, pw, 3) patches, uint8 status[n]) of n quads"""
    q = np.asarray(quads, np.float64).reshape(-1, 8)
    out, st = np.zeros((len(q), ph, pw, 3), np.uint8), np.zeros(len(q), np.uint8)
    for k in range(len(q)):
        out[k], st[k] = patch(bgr, q[k], pw, ph)
    return out, st


def contract_bgr(fmt, planes):
    """the BGR frame the conversion contract gives for planes in format fmt (what tests/pixfmt.convert made them from, for the packed formats)"""
    if fmt == ra.PIX_BGR:
        return planes[0]
    if fmt == ra.PIX_RGB:
        return np.ascontiguousarray(planes[0][..., ::-1])
    if fmt == ra.PIX_BGRA:
        return np.ascontiguousarray(planes[0][..., :3])
    if fmt == ra.PIX_RGBA:
        return np.ascontiguousarray(planes[0][..., 2::-1])
    if fmt == ra.PIX_NV12:
        return pixfmt.nv12_to_bgr(planes[0], planes[1])
    return pixfmt.i420_to_bgr(*planes)


def rect_quads(rects):
    """c2[0], c2[3], c2[2], c2[1] of each rectangle: (n, 4, 2)"""
    return np.ascontiguousarray(np.asarray(rects)["c2"].reshape(-1, 4, 2)[:, [0, 3, 2, 1], :])


def rect_aspect(rect):
    c3 = np.asarray(rect)["c3"].reshape(4, 3)
    length = lambda u, v: math.sqrt(float((u[0] - v[0]) * (u[0] - v[0]) + (u[1] - v[1]) * (u[1] - v[1])) + float((u[2] - v[2]) * (u[2] - v[2])))
    return length(c3[0], c3[1]) / length(c3[1], c3[2])
