"""Annotated frames for the tests: the contract of include/rectdetect_hip.h ("annotated frames") restated from its DEFINITION - the loop over the major coordinate
with V(u) by floor division, not the per-pixel e test the kernel evaluates - in Python integers (covers) and numpy int64 (draw: every product stays below 2^45).
Painter's order, the chroma rule, RD_ANNOT_CLEAR and the host helpers (rd_annot_rects, rd_annot_segments) are restated here too; rd_annot_yuv is tests/pixfmt.py's bgr2yuv."""
import math

import numpy as np

import rectdetect_amd as ra
from tests.pixfmt import bgr2yuv as yuv      # rd_annot_yuv: (Y, U, V)

COORD_MIN, COORD_MAX = -1048576, 1048575
VIDRECT_STYLE = ((0, 255, 0, 1), (0, 200, 255, 2), (255, 0, 0, 1), (0, 0, 255, 2))      # b, g, r, thickness by status


def prims(rows):
    """PRIM_DTYPE array from (x0, y0, x1, y1, b, g, r, thickness) rows"""
    out = np.zeros(len(rows), ra.PRIM_DTYPE)
    for k, row in enumerate(rows):
        out[k] = tuple(int(v) for v in row)
    return out


def _major(x0, y0, x1, y1):
    """(x-major?, ua, va, ub, vb) with the endpoints swapped so that the major coordinate does not decrease"""
    xmajor = abs(x1 - x0) >= abs(y1 - y0)
    a, b = ((x0, y0), (x1, y1)) if xmajor else ((y0, x0), (y1, x1))
    if a[0] > b[0]:
        a, b = b, a
    return xmajor, a[0], a[1], b[0], b[1]


def covers(x0, y0, x1, y1, t, x, y):
    """does the primitive cover pixel (x, y)?  Python integers throughout."""
    x0, y0, x1, y1, t, x, y = (int(v) for v in (x0, y0, x1, y1, t, x, y))
    xmajor, ua, va, ub, vb = _major(x0, y0, x1, y1)
    u, v = (x, y) if xmajor else (y, x)
    if not ua <= u <= ub:
        return False
    D = ub - ua
    V = va if D == 0 else va + (2 * (u - ua) * (vb - va) + D) // (2 * D)
    return -((t - 1) // 2) <= v - V <= t // 2


def owners(prim_array, iw, ih, origin=(0, 0)):
    """(ih, iw) int32: the index of the primitive that owns each pixel - the highest one that covers it - or -1.  Element [row, col] is pixel
    (origin[0] + col, origin[1] + row): (0, 0) for a frame, anything for a window of the plane."""
    own = np.full((ih, iw), -1, np.int32)
    ox, oy = origin
    for k, p in enumerate(prim_array):
        x0, y0, x1, y1, t = int(p["x0"]), int(p["y0"]), int(p["x1"]), int(p["y1"]), int(p["thickness"])
        xmajor, ua, va, ub, vb = _major(x0, y0, x1, y1)
        (nu, ou), (nv, ov) = ((iw, ox), (ih, oy)) if xmajor else ((ih, oy), (iw, ox))
        u = np.arange(max(ua, ou), min(ub, ou + nu - 1) + 1, dtype=np.int64)      # (pixels outside the frame are not written: only these u can matter)
        if len(u) == 0:
            continue
        D = ub - ua
        V = np.full(len(u), va, np.int64) if D == 0 else va + np.floor_divide(2 * (u - ua) * (vb - va) + D, 2 * D)
        for o in range(-((t - 1) // 2), t // 2 + 1):
            v = V + o
            ok = (v >= ov) & (v < ov + nv)
            if xmajor:
                own[v[ok] - oy, u[ok] - ox] = k
            else:
                own[u[ok] - oy, v[ok] - ox] = k
    return own


def draw(fmt, planes, iw, ih, prim_array, clear=False):
    """planes: 2-D uint8 arrays of (rows, pitch) bytes, padding included; returns new ones with the job drawn in place.  An out-of-place job gives the same bytes
    in the destination's rows (its padding stays what it was)."""
    out = [np.array(p, dtype=np.uint8, copy=True) for p in planes]
    own = owners(prim_array, iw, ih)
    hit = own >= 0
    idx = np.where(hit, own, 0)
    pb, pg, pr = (np.asarray(prim_array[c], np.uint8) if len(prim_array) else np.zeros(1, np.uint8) for c in ("b", "g", "r"))
    if fmt <= ra.PIX_RGBA:
        bpp = 3 if fmt in (ra.PIX_BGR, ra.PIX_RGB) else 4
        order = (pb, pg, pr) if fmt in (ra.PIX_BGR, ra.PIX_BGRA) else (pr, pg, pb)
        px = out[0][:ih, :iw * bpp].reshape(ih, iw, bpp)      # (a view: rows of the padded plane)
        for c in range(3):
            ch = px[..., c]
            if clear:
                ch[...] = 0
            ch[hit] = order[c][idx][hit]
        return out
    assert iw % 2 == 0 and ih % 2 == 0
    Y, U, V = (np.asarray(v).astype(np.uint8).reshape(-1) for v in yuv(pb, pg, pr))
    ypl = out[0][:ih, :iw]
    if clear:
        ypl[...] = 16
    ypl[hit] = Y[idx][hit]
    cown = own.reshape(ih // 2, 2, iw // 2, 2).max(axis=(1, 3))      # the highest index that covers any of the sample's four luma pixels
    chit = cown >= 0
    cidx = np.where(chit, cown, 0)
    if fmt == ra.PIX_NV12:
        uv = out[1][:ih // 2, :iw].reshape(ih // 2, iw // 2, 2)
        targets = ((uv[..., 0], U), (uv[..., 1], V))
    else:
        targets = ((out[1][:ih // 2, :iw // 2], U), (out[2][:ih // 2, :iw // 2], V))
    for pl, val in targets:
        if clear:
            pl[...] = 128
        pl[chit] = val[cidx][chit]
    return out


def _coord(v, scale):
    m = float(v) * 2.0 + 0.5 if scale == 2 else float(v)
    if not math.isfinite(m) or not (COORD_MIN - 1 < m < COORD_MAX + 1):
        return None
    return int(m)      # (truncates toward zero)


def rects_prims(rects, scale=1, style=None):
    """rd_annot_rects: six primitives per rectangle in showRect's order"""
    style = VIDRECT_STYLE if style is None else [tuple(int(v) for v in s) for s in np.asarray(style).reshape(4, 4)]
    rows = []
    for r in np.asarray(rects).reshape(-1):
        if int(r["status"]) > 3:
            continue
        c = [(_coord(x, scale), _coord(y, scale)) for x, y in np.asarray(r["c2"]).reshape(4, 2)]
        if any(v is None for xy in c for v in xy):
            continue
        b, g, rr, t = style[int(r["status"])]
        for i in range(4):
            rows.append(c[i] + c[(i + 1) % 4] + (b, g, rr, min(t * scale, 255)))
        rows.append(c[0] + c[2] + (b, g, rr, scale))
        rows.append(c[1] + c[3] + (b, g, rr, scale))
    return prims(rows)


def segments_prims(segs, mode, scale=1):
    """rd_annot_segments: every primitive there is (the caller cuts the list to `max`)"""
    segs = np.asarray(segs).reshape(-1)
    n = int(segs.view("<i4")[0])
    rows = []

    def emit(j, colour):
        c = [_coord(segs[j][k], scale) for k in ("x0", "y0", "x1", "y1")]
        if all(v is not None for v in c):
            rows.append(tuple(c) + colour + (scale,))

    for i in range(1, n + 1):
        if mode == ra.ANNOT_SEG_ALL:
            emit(i, (255, 255, 255))
            continue
        if int(segs[i]["polyid"]) == 0 or int(segs[i]["leftPtr"]) > 0:
            continue
        j, cnt = i, 0
        while 0 < j <= n and cnt < n:
            emit(j, (100, 100, 255) if cnt & 1 else (255, 255, 100))
            j, cnt = int(segs[j]["rightPtr"]), cnt + 1
    return prims(rows)
