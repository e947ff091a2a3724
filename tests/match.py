"""Matched quads for the tests: the contract of include/rectdetect_hip.h ("matched quads") restated in numpy, written from the header's text and not from the
kernels - the signature on tests/rectify.py's patches, the library's rotations, int64 sums and dots, the float64 keys with the tie rule, the float64 scores."""
import math

import numpy as np

import rectdetect_amd as ra
from tests import rectify


def whole(iw, ih):
    """the quad a NULL template quad stands for"""
    return np.array([(-0.5, -0.5), (iw - 0.5, -0.5), (iw - 0.5, ih - 0.5), (-0.5, ih - 0.5)], np.float64)


def cells(patch, G, m):
    """the (G, G) int64 values a of a (G*m, G*m, 3) BGR patch: grey per pixel, the rounded mean per cell, minus 128"""
    p = patch.astype(np.int64)
    grey = (29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8
    s = grey.reshape(G, m, G, m).sum(axis=(1, 3))
    return ((s + (m * m) // 2) >> int(math.log2(m * m))) - 128


def signatures(bgr, quads, G, m):
    """((n, G, G) int64 signatures - zeros for an invalid quad -, uint8 status[n]) of n quads of a BGR frame"""
    pt, st = rectify.patches(bgr, quads, G * m, G * m)
    sig = np.zeros((len(pt), G, G), np.int64)
    for k in range(len(pt)):
        if st[k]:
            sig[k] = cells(pt[k], G, m)
            assert sig[k].min() >= -128 and sig[k].max() <= 127
    return sig, st


def rot(S):
    """one quarter turn: rot(S)[j][i] = S[G-1-i][j]"""
    G = S.shape[0]
    out = np.zeros_like(S)
    for j in range(G):
        for i in range(G):
            out[j, i] = S[G - 1 - i, j]
    return out


def flat(S):
    s = S.astype(np.int64).reshape(-1)
    return len(s) * int((s * s).sum()) - int(s.sum()) ** 2 == 0


def library(templates):
    """the (4T, D) int64 columns of T template signatures (each (G, G)): column 4k + r is template k turned r times"""
    cols = []
    for S in templates:
        R = np.asarray(S, np.int64)
        for r in range(4):
            cols.append(R.reshape(-1))
            R = rot(R)
    return np.array(cols, np.int64).reshape(len(cols), -1) if cols else np.zeros((0, 0), np.int64)


def keys(num, vb):
    """key_c = (num * |num|) / vb in float64, one operation after the other"""
    n = np.asarray(num, np.int64).astype(np.float64)
    return (n * np.abs(n)) / np.asarray(vb, np.int64).astype(np.float64)


def select(key):
    """(best column, runner-up or -1): the greatest key, the lowest column among equal keys; the runner-up by the same rule among the columns of other templates"""
    best = -1
    for c in range(len(key)):
        if best < 0 or key[c] > key[best]:
            best = c
    second = -1
    for c in range(len(key)):
        if c // 4 != best // 4 and (second < 0 or key[c] > key[second]):
            second = c
    return best, second


def score(D, dot, sa, saa, sb, sbb):
    num = D * int(dot) - int(sa) * int(sb)
    va, vb = D * int(saa) - int(sa) ** 2, D * int(sbb) - int(sb) ** 2
    return float(num) / math.sqrt(float(va) * float(vb))


def complete(rec, D, sb, sbb, sb2, sbb2):
    """what rd_match_score makes of a record"""
    out = np.zeros((), ra.MATCH_DTYPE)
    out["status"] = rec["status"]
    if int(rec["status"]) != 1:
        return out
    for f in ("tmpl", "rot", "dot", "tmpl2", "rot2", "dot2", "sa", "saa"):
        out[f] = rec[f]
    out["score"] = score(D, rec["dot"], rec["sa"], rec["saa"], sb, sbb)
    out["score2"] = score(D, rec["dot2"], rec["sa"], rec["saa"], sb2, sbb2) if int(rec["tmpl2"]) >= 0 else 0.0
    return out


def records(sig, status, lib):
    """(MATCH_DTYPE records, (n, 4T) int64 dots) of n signatures (zeros where status is 0) against the (4T, D) columns of a library"""
    n, ncols = len(sig), len(lib)
    D = int(np.prod(np.shape(sig)[1:]))
    a = np.asarray(sig, np.int64).reshape(n, D)
    dots = a @ lib.T if ncols else np.zeros((n, 0), np.int64)
    sb, sbb = lib.sum(axis=1), (lib * lib).sum(axis=1)
    out = np.zeros(n, ra.MATCH_DTYPE)
    for q in range(n):
        sa, saa = int(a[q].sum()), int((a[q] * a[q]).sum())
        va = D * saa - sa * sa
        st = 0 if not status[q] else (3 if ncols == 0 else (2 if va == 0 else 1))
        out[q]["status"] = st
        if st != 1:
            continue
        best, second = select(keys(D * dots[q] - sa * sb, D * sbb - sb * sb))
        r = out[q]
        r["tmpl"], r["rot"], r["dot"], r["sa"], r["saa"] = best // 4, best % 4, dots[q, best], sa, saa
        if second >= 0:
            r["tmpl2"], r["rot2"], r["dot2"] = second // 4, second % 4, dots[q, second]
        else:
            r["tmpl2"] = -1
        out[q] = complete(r, D, sb[best], sbb[best], sb[max(second, 0)], sbb[max(second, 0)])
    return out, dots


def assert_records(got, want, what=""):
    assert len(got) == len(want), "%s: %d records, expected %d" % (what, len(got), len(want))
    for k in range(len(want)):
        assert got[k].tobytes() == want[k].tobytes(), "%s: record %d is %r, expected %r" % (what, k, got[k], want[k])
