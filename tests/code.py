"""Decoded quads for the tests: steps 2-9 of the contract of include/rectdetect_hip.h ("decoded quads") restated from a G plane, written from the header's text and
not from the kernel - the cell of a pixel and whether it counts as two 0/1 matrices (one per axis), the cell sums as Wy . G . Wx^T in int64, threshold, ring,
payload, rotations and the search in Python integers and numpy; a pixel-by-pixel, entry-by-entry twin checks the vectorised form.  The host helpers
(rotate, distance, dictionary, render, upright) in Python integers.  Step 1 is tests/tensor.py's { U8, NHWC, GRAY, m } element on tests/rectify.py's patch."""
import numpy as np

import rectdetect_amd as ra
from tests import tensor

FIELDS = ("bits", "id", "rot", "hamming", "second", "border_errors", "lo", "hi", "margin", "ok", "reserved")
NONE = 65
MASK64 = (1 << 64) - 1


def name(spec, ndict=0):
    return "n%d-b%d-i%d-p%d-m%d-c%d-e%d-h%d-d%d" % tuple([int(spec[f]) for f in ("n", "border", "inset", "polarity", "oversample", "contrast", "max_border", "max_hamming")] + [ndict])


def side(spec):
    return int(spec["n"]) + 2 * int(spec["border"])


def gray_spec(spec):
    """the tensor spec of step 1"""
    return ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, int(spec["oversample"]))


def spec_ok(spec, pw, ph):
    """the legality rule, in Python integers"""
    n, b, inset, pol, m, con, mb, mh = (int(spec[f]) for f in ("n", "border", "inset", "polarity", "oversample", "contrast", "max_border", "max_hamming"))
    if not (3 <= n <= 8 and b in (1, 2) and 0 <= inset <= 3 and pol in (0, 1) and m in (1, 2, 4) and 0 <= con <= 255):
        return False
    C = n + 2 * b
    if not (0 <= mb <= C * C - n * n and 0 <= mh <= n * n):
        return False
    least = 4 * C if inset else C
    return least <= pw <= 1024 and least <= ph <= 1024


def axis(p, C, inset):
    """step 2 for one axis of p pixels: (the cell of every pixel, whether it counts)"""
    a = (2 * np.arange(p, dtype=np.int64) + 1) * C
    c, f = a // (2 * p), a % (2 * p)
    return c, (inset * p <= 4 * f) & (4 * f <= (8 - inset) * p)


def cell_of(spec, pw, ph, i, j):
    """step 2 for one pixel, in Python integers: (cell number, counted)"""
    C, inset = side(spec), int(spec["inset"])
    cx, fx = divmod((2 * i + 1) * C, 2 * pw)
    cy, fy = divmod((2 * j + 1) * C, 2 * ph)
    return cy * C + cx, inset * pw <= 4 * fx <= (8 - inset) * pw and inset * ph <= 4 * fy <= (8 - inset) * ph


def means(G, spec):
    """steps 2 and 3 for one quad: (M, cnt) as (C, C) int64 arrays indexed [cy, cx]; cnt == 0 leaves M = 0 (no legal spec has such a cell)"""
    G = np.asarray(G, np.int64)
    ph, pw = G.shape
    C, inset = side(spec), int(spec["inset"])
    cx, okx = axis(pw, C, inset)
    cy, oky = axis(ph, C, inset)
    Wx = ((cx[None, :] == np.arange(C)[:, None]) & okx[None, :]).astype(np.int64)
    Wy = ((cy[None, :] == np.arange(C)[:, None]) & oky[None, :]).astype(np.int64)
    sg = Wy @ G @ Wx.T
    cnt = Wy.sum(1)[:, None] * Wx.sum(1)[None, :]
    return np.where(cnt > 0, (256 * sg) // np.maximum(cnt, 1), 0), cnt


def means_loop(G, spec):
    """steps 2 and 3 pixel by pixel: the check of means()"""
    G = np.asarray(G)
    ph, pw = G.shape
    C = side(spec)
    sg, cnt = [0] * (C * C), [0] * (C * C)
    for j in range(ph):
        for i in range(pw):
            cell, counted = cell_of(spec, pw, ph, i, j)
            if counted:
                sg[cell] += int(G[j, i])
                cnt[cell] += 1
    M = [(256 * s) // c if c else 0 for s, c in zip(sg, cnt)]
    return np.array(M, np.int64).reshape(C, C), np.array(cnt, np.int64).reshape(C, C)


def rotate(bits, n, k=1):
    """step 6 in Python integers"""
    bits &= (1 << (n * n)) - 1
    for _ in range(k % 4):
        out = 0
        for r in range(n):
            for c in range(n):
                out |= ((bits >> ((n - 1 - c) * n + r)) & 1) << (r * n + c)
        bits = out
    return bits


def popcount(v):
    return bin(v).count("1")


def popcounts(a):
    """popcount of every element of a uint64 array"""
    return np.unpackbits(np.ascontiguousarray(a, np.uint64).view(np.uint8).reshape(-1, 8), axis=1).sum(1).astype(np.int64)


def search(bits, dictionary, n):
    """step 7: (id, rot, hamming, second); numpy over the dictionary"""
    d = np.ascontiguousarray(dictionary if dictionary is not None else [], np.uint64).reshape(-1)
    if len(d) == 0:
        return -1, 0, NONE, NONE
    dist = np.stack([popcounts(d ^ np.uint64(rotate(bits, n, k))) for k in range(4)], axis=1)      # [id, k]
    key = (dist * len(d) + np.arange(len(d))[:, None]) * 4 + np.arange(4)[None, :]                  # (dist, id, k) in lexicographic order
    at = int(np.argmin(key))
    i, k = at // 4, at % 4
    others = np.delete(dist, i, axis=0)
    return i, k, int(dist[i, k]), int(others.min()) if len(others) else NONE


def search_loop(bits, dictionary, n):
    """step 7 entry by entry in Python integers: the check of search()"""
    d = [int(v) for v in (dictionary if dictionary is not None else [])]
    if not d:
        return -1, 0, NONE, NONE
    best = min((popcount(rotate(bits, n, k) ^ d[i]), i, k) for i in range(len(d)) for k in range(4))
    second = min([popcount(rotate(bits, n, k) ^ d[i]) for i in range(len(d)) for k in range(4) if i != best[1]] or [NONE])
    return best[1], best[2], best[0], second


def decide(M, spec, dictionary=None, find=search):
    """steps 4-9 for one valid quad from its (C, C) means: a CODE_DTYPE record"""
    n, b, pol = int(spec["n"]), int(spec["border"]), int(spec["polarity"])
    C = n + 2 * b
    Ml = [[int(v) for v in row] for row in np.asarray(M).reshape(C, C)]
    flat = [v for row in Ml for v in row]
    lo, hi = min(flat), max(flat)
    v = [[int(2 * Ml[y][x] > lo + hi) ^ pol for x in range(C)] for y in range(C)]
    margin = min(abs(2 * m - (lo + hi)) for m in flat)
    errors = sum(v[y][x] for y in range(C) for x in range(C) if x < b or x >= C - b or y < b or y >= C - b)
    bits = 0
    for r in range(n):
        for c in range(n):
            bits |= v[b + r][b + c] << (r * n + c)
    ndict = 0 if dictionary is None else len(dictionary)
    i, k, ham, second = find(bits, dictionary, n)
    rec = np.zeros((), ra.CODE_DTYPE)
    rec["bits"], rec["id"], rec["rot"], rec["hamming"], rec["second"], rec["border_errors"], rec["lo"], rec["hi"], rec["margin"] = bits, i, k, ham, second, errors, lo, hi, margin
    rec["ok"] = int(hi - lo >= 256 * int(spec["contrast"]) and errors <= int(spec["max_border"]) and (ndict == 0 or ham <= int(spec["max_hamming"])))
    return rec


def from_planes(planes, status, spec, dictionary=None):
    """the (n, 48) uint8 output of a job from its (n, ph, pw) G planes (the tensor rectifier's output, or tensor.tensors'): zero bytes for an invalid quad"""
    planes = np.asarray(planes)
    n, ph, pw = planes.shape[:3]
    out = np.zeros(n, ra.CODE_DTYPE)
    for q in range(n):
        if status[q]:
            out[q] = decide(means(planes[q].reshape(ph, pw), spec)[0], spec, dictionary)
    return out.view(np.uint8).reshape(n, 48)


def records(bgr, quads, pw, ph, spec, dictionary=None):
    """(the (n, 48) uint8 output of n quads of an (ih, iw, 3) BGR image, uint8 status[n]): the full restatement"""
    planes, st = tensor.tensors(bgr, quads, pw, ph, gray_spec(spec))
    return from_planes(planes.reshape(len(st), ph, pw), st, spec, dictionary), st


def distance(dictionary, n):
    """rd_code_distance in Python integers (65 for an empty dictionary)"""
    d = [int(v) for v in dictionary]
    best = NONE
    for a in range(len(d)):
        for k in range(1, 4):
            best = min(best, popcount(rotate(d[a], n, k) ^ d[a]))
        for b in range(a + 1, len(d)):
            for k in range(4):
                best = min(best, popcount(rotate(d[a], n, k) ^ d[b]))
    return best


def splitmix64(s):
    """(the next state, the next value) of the header's generator"""
    s = (s + 0x9E3779B97F4A7C15) & MASK64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return s, z ^ (z >> 31)


def dictionary(n, count, min_dist, seed, tries):
    """rd_code_dictionary in Python integers: the list of accepted codes"""
    out, s = [], seed & MASK64
    for _ in range(tries):
        if len(out) >= count:
            break
        s, z = splitmix64(s)
        cand = z & ((1 << (n * n)) - 1)
        if distance(out + [cand], n) >= min_dist:
            out.append(cand)
    return out


def render(spec, bits, cell_px):
    """rd_code_render restated: the (C * cell_px)^2 image"""
    n, b, pol = int(spec["n"]), int(spec["border"]), int(spec["polarity"])
    C = n + 2 * b
    v = np.zeros((C, C), np.uint8)
    for r in range(n):
        for c in range(n):
            v[b + r, b + c] = (bits >> (r * n + c)) & 1
    return np.kron(np.where(v ^ pol, 255, 0).astype(np.uint8), np.ones((cell_px, cell_px), np.uint8))


def upright(quad, rot):
    q = np.asarray(quad, np.float64).reshape(4, 2)
    return np.array([q[(c + 4 - rot) % 4] for c in range(4)])


def identity_quad(x0, y0, w, h):
    """the quad whose pw = w, ph = h patch samples frame pixel (x0 + i, y0 + j) exactly (tests/rectify.py: x = X - 1/2 + ...)"""
    return np.array([(x0 - 0.5, y0 - 0.5), (x0 + w - 0.5, y0 - 0.5), (x0 + w - 0.5, y0 + h - 0.5), (x0 - 0.5, y0 + h - 0.5)], np.float64)


def assert_records(got, status, want, wstatus, what=""):
    """names the quad and the field that differ"""
    assert np.array_equal(status, wstatus), "%s: status %r, expected %r" % (what, np.asarray(status).tolist(), np.asarray(wstatus).tolist())
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, "%s: %r %r, expected %r %r" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if np.array_equal(got, want):
        return
    g, w = ra.code_view(got), ra.code_view(want)
    for q in range(len(w)):
        for f in FIELDS:
            if g[q][f] != w[q][f]:
                raise AssertionError("%s: quad %d field %s: got %r, expected %r (the record: got %r, expected %r)" % (what, q, f, g[q][f], w[q][f], g[q], w[q]))
    raise AssertionError("%s: bytes differ outside the records" % what)
