"""The fused gradient / suppression kernel (k_grad_nms, rectdetect_amd/csrc/rd_k_nms.hip: 64 x 16 tiles, four waves) at the sizes where its tiles end and on
content that fills its list of local maxima: the `nms` plane of the frame path (TAPS 0) and, through the debug planes `plab1`, `vxy` and `strength`, the TAPS 1
instantiation - which writes `nms` again - against the oracle's planes.  Every value is the reference's expression tree evaluated in its order, so every
comparison is np.array_equal on the raw bits.

Frames, on one single-slot detector, in this order:
  a0, a1  frames 0 and 1 of a synthetic stream: about 29 % of the pixels carry a response, like the benchmark stream
  b       a constant frame right after: every pixel is a local maximum (the list of maxima overflows in every tile) and the whole plane must turn into +0
          bits - a store skipped on the overflow path leaves a1's values behind
  c       the constant frame with a single 255 pixel every 23 columns and 11 rows: flat stretches between many non-zero responses
  c2      the same with a dot every 61 columns and 29 rows: tiles that are almost all maxima and also hold non-zero responses
  d       frame a0 with its left half constant: flat areas next to busy ones in one frame
The spacing of c (23 x 11) leaves at most 348 certain maxima in a full tile of the 130 x 34 frame - fewer than any capacity the list may have (it holds at
least 512) - so c2 was added with the spacing widened to 61 x 29, which leaves 827 .. 885 per full tile: more than the largest capacity the kernel's LDS
budget admits (796).  What the frames must contain for the comparisons to mean something is asserted on the CPU (test_fixtures_are_what_they_claim; no GPU)."""
import functools
import os
import re

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
GN_W, GN_H = 64, 16            # the tile: 64 columns x GN_ROWS of rd_k_nms.hip - keep them equal
# (iw, ih); the kernel accepts a remainder of 0 or of at least 2 per axis: one tile with every halo cell mirrored, the smallest remainder tiles both ways,
# 2 x 2 full tiles, full tiles plus remainders, remainders 62 and 15
SHAPES = [(64, 16), (66, 18), (128, 32), (130, 34), (190, 47)]
BIG = (130, 34)
SEED = 3
FRAMES = ("a0", "a1", "b", "c", "c2", "d")
PLANES = [("nms", 1), ("plab1", 1), ("vxy", 2), ("strength", 1), ("nms", 1)]      # in this order: asking for a tap runs TAPS 1, which writes nms again


def dotted(iw, ih, dx, dy):
    f = np.full((ih, iw, 3), 90, np.uint8)
    f[::dy, ::dx] = 255
    return f


@functools.lru_cache(maxsize=None)
def frames(iw, ih):
    a0, a1 = (synth.frame(synth.SEED0 + SEED, iw, ih, t) for t in range(2))
    d = a0.copy()
    d[:, :iw // 2] = 90
    f = {"a0": a0, "a1": a1, "b": np.full((ih, iw, 3), 90, np.uint8), "c": dotted(iw, ih, 23, 11), "c2": dotted(iw, ih, 61, 29), "d": d}
    for a in f.values():
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def oracle_planes(iw, ih):
    """frame name -> plane name -> the oracle's plane as uint32 (computed once per shape, shared, read-only)"""
    orc = helpers.OracleRect(iw, ih, helpers.REGION_SPEC)
    out = {}
    for name in FRAMES:
        orc.frame(frames(iw, ih)[name])
        out[name] = {p: orc.plane(p).view(np.uint32) for p, _ in PLANES}
        for a in out[name].values():
            a.setflags(write=False)
    orc.close()
    return out


def compare_planes(det, want, what):
    for p, k in PLANES:
        got = det.plane(p, np.uint32, det.N * k)
        assert np.array_equal(got, want[p]), f"{what}: plane {p} differs in {int((got != want[p]).sum())} words, first at {np.flatnonzero(got != want[p])[:4].tolist()}"


# ---- 1. the frame path and the taps against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("iw,ih", SHAPES)
def test_planes_against_oracle(iw, ih):
    det = ra.Detector(iw, ih, nslots=1)
    want = oracle_planes(iw, ih)
    for name in FRAMES:
        det.enqueue(frames(iw, ih)[name])
        det.poll(TAN36)
        compare_planes(det, want[name], f"{iw}x{ih} frame {name}")
    det.close()


# ---- 2. group launches
@pytest.mark.gpu
def test_group_launches_equal_the_single_slot_detector():
    """frames of a group work on planes `zs` bytes behind the first's: planes and rectangle lists of a 32-slot detector (groups of 8) must equal the
    single-slot detector's, whose planes are pinned to the oracle above"""
    iw, ih = BIG
    f = frames(iw, ih)
    seq = [synth.frame(synth.SEED0 + SEED, iw, ih, t // 2) if t % 2 == 0 else f["c" if t % 4 == 1 else "c2"] for t in range(16)]
    outs = []
    for slots in (1, 32):
        det = ra.Detector(iw, ih, nslots=slots, nworkers=1 if slots > 1 else 0)
        got = []
        take = lambda: got.append((det.poll(TAN36), {(i, p): det.plane(p, np.uint32, det.N * k) for i, (p, k) in enumerate(PLANES)}))
        if slots == 1:
            for fr in seq:
                det.enqueue(fr)
                take()
        else:
            for fr in seq:
                det.enqueue(fr)
            for _ in seq:
                take()
            assert det.frames_per_launch() == 8
        det.close()
        outs.append(got)
    for t, ((r1, p1), (r2, p2)) in enumerate(zip(*outs)):
        for g in p1:
            assert np.array_equal(p1[g], p2[g]), f"frame {t} of 16 in groups of 8: plane {g[1]} differs in {int((p1[g] != p2[g]).sum())} words"
        assert helpers.rects_equal(r1, r2), f"frame {t} of 16 in groups of 8: rectangle lists differ"


# ---- 3. the fixtures are what they claim (no GPU)
def certain_maxima(strength):
    """pixels whose strength is zero on the whole window -3 .. +4 around them (cells outside the frame: the mirrored ones): every sample is 0 there, so
    am1 <= a0 && a0 >= ap1 holds whatever the direction"""
    ih, iw = strength.shape
    z = np.pad(strength == 0, 4, mode="reflect")
    c = np.ones((ih, iw), bool)
    for dy in range(-3, 5):
        for dx in range(-3, 5):
            c &= z[4 + dy:4 + dy + ih, 4 + dx:4 + dx + iw]
    return c


def test_fixtures_are_what_they_claim():
    src = open(os.path.join(helpers.ROOT, "rectdetect_amd", "csrc", "rd_k_nms.hip")).read()
    assert int(re.search(r"#define GN_ROWS (\d+)", src).group(1)) == GN_H, "the fixtures are placed by the kernel's tile"
    cap = int(re.search(r"#define GN_LCAP (\d+)", src).group(1))
    assert 512 <= cap <= 796
    for iw, ih in SHAPES:
        want = oracle_planes(iw, ih)
        # (b): no response anywhere - every pixel is a maximum of zeros
        assert not want["b"]["strength"].any() and not want["b"]["nms"].any(), (iw, ih)
        # (a): responses on about 29 % of the pixels, and values for (b) to wipe out
        share = float((want["a1"]["nms"].view(np.float32) > 0).mean())
        assert 0.2 <= share <= 0.4, (iw, ih, share)
    iw, ih = BIG
    c2 = oracle_planes(iw, ih)["c2"]
    cert = certain_maxima(c2["strength"].view(np.float32).reshape(ih, iw))
    pos = c2["nms"].view(np.float32).reshape(ih, iw) > 0
    tiles = [(slice(y, y + GN_H), slice(x, x + GN_W)) for y in range(0, ih - GN_H + 1, GN_H) for x in range(0, iw - GN_W + 1, GN_W)]
    assert any(int(cert[t].sum()) > cap and pos[t].any() for t in tiles), [(int(cert[t].sum()), int(pos[t].sum())) for t in tiles]
