"""Scanned pages for the tests: steps 2-5 of the contract of include/rectdetect_hip.h ("scanned pages") restated in numpy from a G plane, written from the header's
text and not from the kernel - an integral image in int64 for the window sums, the window's pixel count from the clamps, the two decisions as array expressions,
np.packbits for the bit rows.  Step 1 is tests/tensor.py's { U8, NHWC, GRAY, m } element on tests/rectify.py's patch."""
import numpy as np

import rectdetect_amd as ra
from tests import tensor

MODES = (ra.SCAN_FLAT, ra.SCAN_BILEVEL, ra.SCAN_BITS)
MODE_NAMES = {ra.SCAN_FLAT: "flat", ra.SCAN_BILEVEL: "bilevel", ra.SCAN_BITS: "bits"}


def name(spec):
    return "%s-r%d-k%d-d%d-w%d-m%d%s" % (MODE_NAMES[int(spec["mode"])], int(spec["radius"]), int(spec["k"]), int(spec["d"]), int(spec["white"]), int(spec["oversample"]), "-inv" if int(spec["invert"]) else "")


def gray_spec(spec):
    """the tensor spec of step 1"""
    return ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, int(spec["oversample"]))


def shape(spec, n, pw, ph):
    return (n, ph, (pw + 7) // 8 if int(spec["mode"]) == ra.SCAN_BITS else pw)


def window(G, r):
    """step 2 for every pixel of a (ph, pw) plane of (already inverted) values: (N, T) as int64 arrays"""
    G = np.asarray(G, np.int64)
    ph, pw = G.shape
    I = np.zeros((ph + 1, pw + 1), np.int64)
    I[1:, 1:] = G.cumsum(0).cumsum(1)
    x0, x1 = np.maximum(0, np.arange(pw) - r), np.minimum(pw - 1, np.arange(pw) + r) + 1
    y0, y1 = np.maximum(0, np.arange(ph) - r), np.minimum(ph - 1, np.arange(ph) + r) + 1
    T = I[y1[:, None], x1[None, :]] - I[y0[:, None], x1[None, :]] - I[y1[:, None], x0[None, :]] + I[y0[:, None], x0[None, :]]
    N = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    return N, T


def decide(spec, G, N, T):
    """steps 3 and 4 for arrays of (already inverted) G, N and T: (ink as bool, F as int64)"""
    G, N, T = np.asarray(G, np.int64), np.asarray(N, np.int64), np.asarray(T, np.int64)
    k, d, white = int(spec["k"]), int(spec["d"]), int(spec["white"])
    ink = 256 * N * (G + d) < (256 - k) * T
    F = np.where(T == 0, white, np.minimum(255, (G * N * white + (T >> 1)) // np.maximum(T, 1)))
    return ink, F


def page(G0, spec):
    """steps 1 (the inversion) to 5 for one valid quad: its output as a uint8 array of shape(spec, 1, pw, ph)[1:], from the (ph, pw) plane G0"""
    G = np.asarray(G0, np.int64)
    if int(spec["invert"]):
        G = 255 - G
    N, T = window(G, int(spec["radius"]))
    ink, F = decide(spec, G, N, T)
    mode = int(spec["mode"])
    if mode == ra.SCAN_FLAT:
        return F.astype(np.uint8)
    if mode == ra.SCAN_BILEVEL:
        return np.where(ink, 0, 255).astype(np.uint8)
    return np.packbits(ink, axis=1, bitorder="big")      # (pads a row's last byte with 0 bits)


def from_planes(planes, status, spec):
    """the pages of a job from its (n, ph, pw) G planes (the tensor rectifier's output, or tensor.tensors'): zero bytes for an invalid quad"""
    planes = np.asarray(planes)
    n, ph, pw = planes.shape[:3]
    out = np.zeros(shape(spec, n, pw, ph), np.uint8)
    for q in range(n):
        if status[q]:
            out[q] = page(planes[q].reshape(ph, pw), spec)
    return out


def pages(bgr, quads, pw, ph, spec):
    """(the uint8 array of shape(spec, n, pw, ph) of n quads of an (ih, iw, 3) BGR image, uint8 status[n]): the full restatement"""
    planes, st = tensor.tensors(bgr, quads, pw, ph, gray_spec(spec))
    return from_planes(planes.reshape(len(st), ph, pw), st, spec), st


def brute(G, r):
    """step 2 by counting and adding, for small planes: the check of window()"""
    G = np.asarray(G, np.int64)
    ph, pw = G.shape
    N, T = np.zeros((ph, pw), np.int64), np.zeros((ph, pw), np.int64)
    for j in range(ph):
        for i in range(pw):
            w = G[max(0, j - r):min(ph - 1, j + r) + 1, max(0, i - r):min(pw - 1, i + r) + 1]
            N[j, i], T[j, i] = w.size, w.sum()
    return N, T


def assert_pages(got, status, want, wstatus, what=""):
    assert np.array_equal(status, wstatus), "%s: status %r, expected %r" % (what, np.asarray(status).tolist(), np.asarray(wstatus).tolist())
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, "%s: %r %r, expected %r %r" % (what, got.shape, got.dtype, want.shape, want.dtype)
    for q in range(len(want)):
        if not np.array_equal(got[q], want[q]):
            ys, xs = np.nonzero(got[q] != want[q])
            raise AssertionError("%s: quad %d differs in %d bytes, first at row %d byte %d: got %d, expected %d" % (what, q, len(ys), ys[0], xs[0], got[q][ys[0], xs[0]], want[q][ys[0], xs[0]]))
