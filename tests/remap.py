"""Remapped frames for the tests: the contract of include/rectdetect_hip.h ("remapped frames") restated in numpy float64, written from the header's text and
not from the C code - the source position of an output pixel under a lens and a view, the table entry of a position, the table from a caller's float32 maps,
and the 8.8 fixed-point bilinear blend with the fill colour for outside entries.  Frames in the other pixel formats go through tests/rectify.py: contract_bgr
first: the header says that the output from such a frame equals the output from the BGR frame the conversion contract gives for it."""
import numpy as np

LENS_FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
VIEW_FIELDS = ("fx", "fy", "cx", "cy")


def _fields(rec, names):
    """the named fields of a record (a numpy record, a dict or a sequence in that order) as numpy float64 scalars"""
    if isinstance(rec, dict):
        return [np.float64(rec[n]) for n in names]
    a = np.asarray(rec)
    if a.dtype.names:
        return [np.float64(a[n]) for n in names]
    return [np.float64(v) for v in a.reshape(-1)[:len(names)]]


def points(lens, view, uv):
    """(n, 2) source positions X, Y of (n, 2) output points u, v.  numpy float64 element-wise operations are IEEE doubles and nothing here is contracted."""
    lfx, lfy, lcx, lcy, k1, k2, p1, p2, k3 = _fields(lens, LENS_FIELDS)
    vfx, vfy, vcx, vcy = _fields(view, VIEW_FIELDS)
    p = np.asarray(uv, np.float64).reshape(-1, 2)
    u, v = p[:, 0], p[:, 1]
    with np.errstate(all="ignore"):
        x = (u - vcx) / vfx
        y = (v - vcy) / vfy
        xx = x * x
        yy = y * y
        xy = x * y
        r2 = xx + yy
        rad = ((k3 * r2 + k2) * r2 + k1) * r2 + 1.0
        xd = (x * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
        yd = (y * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
        X = lfx * xd + lcx
        Y = lfy * yd + lcy
    return np.stack([X, Y], axis=1)


def entries(X, Y, iw, ih):
    """the int32 entries (..., 2) of positions X, Y (float64 arrays of one shape) in an iw x ih source, and how many are inside"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    with np.errstate(all="ignore"):
        inside = (X >= 0.0) & (X <= np.float64(iw - 1)) & (Y >= 0.0) & (Y <= np.float64(ih - 1))      # (a NaN compares false)
        xi = np.floor(np.where(inside, X, 0.0) * 256.0).astype(np.int32)
        yi = np.floor(np.where(inside, Y, 0.0) * 256.0).astype(np.int32)
    out = np.stack([np.where(inside, xi, -1), np.where(inside, yi, -1)], axis=-1).astype(np.int32)
    return out, int(inside.sum())


def grid(ow, oh):
    """the (ow * oh, 2) output pixels u, v in the table's order: rows back to back"""
    v, u = np.mgrid[0:oh, 0:ow]
    return np.stack([u.reshape(-1), v.reshape(-1)], axis=1).astype(np.float64)


def table_lens(lens, view, ow, oh, iw, ih):
    """((oh, ow, 2) int32 table, inside entries) of an ow x oh output from an iw x ih source under a lens and a view"""
    XY = points(lens, view, grid(ow, oh))
    return entries(XY[:, 0].reshape(oh, ow), XY[:, 1].reshape(oh, ow), iw, ih)


def table_map(mapx, mapy, ow, oh, iw, ih):
    """the same from two planes of ow * oh float32 values: each value widened to double, then the same entry rule"""
    mx, my = np.asarray(mapx, np.float32).reshape(oh, ow), np.asarray(mapy, np.float32).reshape(oh, ow)
    return entries(mx.astype(np.float64), my.astype(np.float64), iw, ih)


def apply(bgr, table, ow, oh, fill):
    """the (oh, ow, 3) uint8 output of an (ih, iw, 3) BGR source through a table; fill = (b, g, r) for outside entries"""
    ih, iw = bgr.shape[:2]
    t = np.asarray(table, np.int64).reshape(oh, ow, 2)
    xi, yi = t[..., 0], t[..., 1]
    outside = xi < 0
    xi, yi = np.where(outside, 0, xi), np.where(outside, 0, yi)
    x0, fx = xi >> 8, (xi & 255)[..., None]
    y0, fy = yi >> 8, (yi & 255)[..., None]
    x1, y1 = np.minimum(x0 + 1, iw - 1), np.minimum(y0 + 1, ih - 1)
    p = np.asarray(bgr).astype(np.int64)
    top = p[y0, x0] * (256 - fx) + p[y0, x1] * fx
    bot = p[y1, x0] * (256 - fx) + p[y1, x1] * fx
    out = ((top * (256 - fy) + bot * fy + 32768) >> 16).astype(np.uint8)
    out[outside] = np.asarray(fill, np.uint8).reshape(3)
    return out
