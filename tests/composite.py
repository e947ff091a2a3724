"""Composited quads for the tests: the contract of include/rectdetect_hip.h ("composited quads") restated in numpy float64 from the header's text and not from the
kernel or the host code - the adjugate and the pixel box of an item, the per-pixel coverage test, fill and paste, painter's order, the chroma mean of NV12 / I420 and
the set of tiles an in-place job launches.  What tests/rectify.py (the forward coefficients, validity) and tests/pixfmt.py / tests/annotate.py (formats, rd_annot_yuv)
already state is imported from there."""
import math

import numpy as np

import rectdetect_amd as ra
from tests import annotate
from tests import rectify

EMPTY_BOX = (0, 0, -1, -1)


def items(rows):
    """COMP_ITEM_DTYPE array from (quad, patch, (b, g, r)) rows"""
    out = np.zeros(len(rows), ra.COMP_ITEM_DTYPE)
    for k, (quad, patch, colour) in enumerate(rows):
        out[k]["quad"] = np.asarray(quad, np.float64).reshape(4, 2)
        out[k]["patch"] = patch
        out[k]["b"], out[k]["g"], out[k]["r"] = colour
    return out


def _axis(v, size):
    """one axis of the pixel box, or None when it is empty.  Python floats: IEEE doubles"""
    fl = math.floor(min(v)) - 1.0 if all(math.isfinite(x) for x in v) else None
    ce = math.ceil(max(v)) + 1.0
    if ce < 0.0 or fl > float(size - 1):
        return None
    return int(max(fl, 0.0)), int(min(ce, float(size - 1)))


def coefficients(quad, iw, ih):
    """(A..I as float64[9], (bx0, by0, bx1, by1), status): zeros, the empty box and 0 for an invalid item; a valid item with an empty box has the empty box"""
    co, status = rectify.coefficients(quad)
    if not status:
        return np.zeros(9, np.float64), EMPTY_BOX, 0
    a, b, c, d, e, f, g, h = (float(v) for v in co)
    inv = [e - f * h, c * h - b, b * f - c * e,
           f * g - d, a - c * g, c * d - a * f,
           d * h - e * g, b * g - a * h, a * e - b * d]
    if not all(math.isfinite(v) for v in inv):
        return np.zeros(9, np.float64), EMPTY_BOX, 0
    q = [float(v) for v in np.asarray(quad, np.float64).reshape(8)]
    bx, by = _axis(q[0::2], iw), _axis(q[1::2], ih)
    box = EMPTY_BOX if bx is None or by is None else (bx[0], by[0], bx[1], by[1])
    return np.array(inv, np.float64), box, 1


def st_window(inv, x0, y0, x1, y1):
    """s and t of the pixels [x0, x1] x [y0, y1] (inclusive) as (rows, columns) float64 arrays, in the header's operations"""
    A, B, C, D, E, F, G, H, I = (np.float64(v) for v in inv)
    X = np.arange(x0, x1 + 1, dtype=np.float64)[None, :]
    Y = np.arange(y0, y1 + 1, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        wn = (G * X + H * Y) + I
        s = ((A * X + B * Y) + C) / wn
        t = ((D * X + E * Y) + F) / wn
    return s, t


def coverage(quad, iw, ih):
    """((ih, iw) bool coverage of one quad, s, t as (ih, iw) float64 - valid inside the box only), status"""
    inv, box, status = coefficients(quad, iw, ih)
    cov = np.zeros((ih, iw), bool)
    s, t = np.zeros((ih, iw)), np.zeros((ih, iw))
    if status and box[0] <= box[2]:
        bx0, by0, bx1, by1 = box
        sw, tw = st_window(inv, bx0, by0, bx1, by1)
        s[by0:by1 + 1, bx0:bx1 + 1], t[by0:by1 + 1, bx0:bx1 + 1] = sw, tw
        cov[by0:by1 + 1, bx0:bx1 + 1] = (sw >= 0.0) & (sw < 1.0) & (tw >= 0.0) & (tw < 1.0)      # (a NaN or an infinity fails)
    return cov, s, t, status


def _fix8(v, size):
    q = np.floor(v * 256.0)
    q = np.where(q > 0.0, q, 0.0)      # (anything not above 0, a NaN too)
    q = np.where(q < (size - 1) * 256.0, q, (size - 1) * 256.0)
    return q.astype(np.int64)


def paste(patch, s, t):
    """the (..., 3) uint8 colours a (ph, pw, 3) BGR patch gives at s, t"""
    ph, pw = patch.shape[:2]
    with np.errstate(all="ignore"):
        u = s * np.float64(pw) - 0.5
        v = t * np.float64(ph) - 0.5
        ui, vi = _fix8(u, pw), _fix8(v, ph)
    x0, fx = ui >> 8, (ui & 255)[..., None]
    y0, fy = vi >> 8, (vi & 255)[..., None]
    x1, y1 = np.minimum(x0 + 1, pw - 1), np.minimum(y0 + 1, ph - 1)
    p = patch.astype(np.int64)
    top = p[y0, x0] * (256 - fx) + p[y0, x1] * fx
    bot = p[y1, x0] * (256 - fx) + p[y1, x1] * fx
    return ((top * (256 - fy) + bot * fy + 32768) >> 16).astype(np.uint8)


def colours(item_array, patches, iw, ih):
    """painter's order: ((ih, iw) bool covered, (ih, iw, 3) uint8 final B, G, R of the covered pixels, uint8 status[n]) - later items overwrite earlier ones"""
    hit = np.zeros((ih, iw), bool)
    col = np.zeros((ih, iw, 3), np.uint8)
    status = np.zeros(len(item_array), np.uint8)
    for k, it in enumerate(item_array):
        cov, s, t, status[k] = coverage(it["quad"], iw, ih)
        if not cov.any():
            continue
        if int(it["patch"]) >= 0:
            col[cov] = paste(np.asarray(patches)[int(it["patch"])], s[cov], t[cov])
        else:
            col[cov] = (int(it["b"]), int(it["g"]), int(it["r"]))
        hit |= cov
    return hit, col, status


def draw(fmt, planes, iw, ih, item_array, patches=None):
    """planes: 2-D uint8 arrays of (rows, pitch) bytes, padding included; returns (new planes with the job composited in place, status).  An out-of-place job gives the
    same bytes in the destination's rows (its padding stays what it was)."""
    out = [np.array(p, dtype=np.uint8, copy=True) for p in planes]
    hit, col, status = colours(item_array, patches, iw, ih)
    if fmt <= ra.PIX_RGBA:
        bpp = 3 if fmt in (ra.PIX_BGR, ra.PIX_RGB) else 4
        order = (0, 1, 2) if fmt in (ra.PIX_BGR, ra.PIX_BGRA) else (2, 1, 0)
        px = out[0][:ih, :iw * bpp].reshape(ih, iw, bpp)      # (a view: rows of the padded plane)
        for c in range(3):
            px[..., c][hit] = col[..., order[c]][hit]
        return out, status
    assert iw % 2 == 0 and ih % 2 == 0
    Y, _, _ = annotate.yuv(col[..., 0], col[..., 1], col[..., 2])
    out[0][:ih, :iw][hit] = Y.astype(np.uint8)[hit]
    # a chroma sample: the rounded mean colour of the covered ones among its four luma pixels
    n = hit.reshape(ih // 2, 2, iw // 2, 2).sum(axis=(1, 3)).astype(np.int64)
    S = (col.astype(np.int64) * hit[..., None]).reshape(ih // 2, 2, iw // 2, 2, 3).sum(axis=(1, 3))
    chit = n >= 1
    nn = np.where(chit, n, 1)
    M = (S + (nn // 2)[..., None]) // nn[..., None]
    _, U, V = annotate.yuv(M[..., 0], M[..., 1], M[..., 2])
    U, V = U.astype(np.uint8), V.astype(np.uint8)
    if fmt == ra.PIX_NV12:
        uv = out[1][:ih // 2, :iw].reshape(ih // 2, iw // 2, 2)
        uv[..., 0][chit], uv[..., 1][chit] = U[chit], V[chit]
    else:
        out[1][:ih // 2, :iw // 2][chit] = U[chit]
        out[2][:ih // 2, :iw // 2][chit] = V[chit]
    return out, status


def tiles(item_array, iw, ih, tile_w, tile_h):
    """the set of (tx, ty) the boxes of the valid items reach"""
    out = set()
    for it in item_array:
        _, box, status = coefficients(it["quad"], iw, ih)
        if not status or box[0] > box[2]:
            continue
        for ty in range(box[1] // tile_h, box[3] // tile_h + 1):
            for tx in range(box[0] // tile_w, box[2] // tile_w + 1):
                out.add((tx, ty))
    return out


def random_quad(rng, cx, cy, radius, flip=False):
    """a strictly convex quad around (cx, cy): four points at increasing angles on a wobbly circle; flip: the other orientation"""
    while True:
        ang = np.sort(rng.uniform(0, 2 * np.pi, 4))
        if np.min(np.diff(np.concatenate([ang, [ang[0] + 2 * np.pi]]))) < 0.5:
            continue
        r = radius * rng.uniform(0.6, 1.0, 4)
        q = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], axis=1)
        if flip:
            q = q[::-1].copy()
        if rectify.valid(q):
            return q


def seeded_quads(n=300, iw=320, ih=200, seed=20240):
    """n random strictly convex quads, both orientations, partly outside an iw x ih frame"""
    rng = np.random.default_rng(seed)
    return [random_quad(rng, rng.uniform(-20, iw + 20), rng.uniform(-20, ih + 20), rng.uniform(3, 90), flip=bool(k & 1)) for k in range(n)]
