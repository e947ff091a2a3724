"""The two small dense kernels of the rect path - the run extents of the edge-stopped blur (k_blblur_extents, 64 x 32 tiles) and quantise / despeckle
(k_despeckle, 64 x 30 tiles) - against the oracle at the sizes where their tiles end: `smooth` (twenty blur passes over the extents) and `quant` must be
bit-identical, frame by frame and inside group launches.  What the fixtures must contain for that to mean something is asserted on the CPU from the
oracle's own planes (test_fixtures_cover_the_cases; it needs no GPU)."""
import functools
import os
import re

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
DS_ROWS, BE_ROWS = 30, 32      # tile heights of k_despeckle and k_blblur_extents (both 64 wide): DS_ROWS and BE_ROWS of rectdetect_amd/csrc/rd_k_rect.hip - keep them equal
# width below / equal to / one over 64; height below, equal to, one over and one row short of the tile heights (29 30 31 | 31 32 33) and of 54 rows (the blur
# pair's tile, and a height the despeckle tile was also measured at); several tiles both ways; (65, 31, 14) holds the hot pixel with a single candidate, (191, 161) many tiles
FIXTURES = [(17, 19, 0), (63, 29, 0), (64, 30, 0), (65, 31, 14), (64, 32, 0), (65, 33, 0), (63, 53, 1), (65, 55, 1), (129, 47, 0), (191, 161, 9)]
NFRAMES = 2                    # the second frame's edge mask carries the first frame's strong mask


@functools.lru_cache(maxsize=None)
def oracle_frames(iw, ih, seed, n=NFRAMES):
    """the oracle's planes of frames 0 .. n-1 of a synthetic stream (computed once, shared, read-only)"""
    orc = helpers.OracleRect(iw, ih)
    out = []
    for t in range(n):
        orc.frame(synth.frame(synth.SEED0 + seed, iw, ih, t))
        planes = {k: orc.plane(k) for k in ("smooth", "quant", "nms", "edge500")}
        for a in planes.values():
            a.setflags(write=False)
        out.append(planes)
    orc.close()
    return tuple(out)


def shifted(a, dx, dy, fill):
    """a[y + dy, x + dx], `fill` outside the frame"""
    h, w = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = a[ys, xs]
    return out


def runs_along_x(E):
    """oclrect.cl:155-205 on a boolean edge mask: samples taken towards smaller and towards larger x (0..5 each), before "no run at all -> the centre alone" """
    Ep, En, Es = shifted(E, -1, 0, False), shifted(E, 1, 0, False), shifted(E, 0, 1, False)
    stop_l = ((E & ~Ep) | (~E & Ep & Es)) & (np.arange(E.shape[1])[None, :] > 0)      # this cell ends the scan towards smaller x before it is counted
    stop_r = ~E & En                                                                   # ... towards larger x, centre not on an edge (on an edge: the first cell off it)
    nl, nr = np.zeros(E.shape, int), np.zeros(E.shape, int)
    run_l, run_r = np.ones(E.shape, bool), np.ones(E.shape, bool)
    for d in range(5):
        run_l &= ~shifted(stop_l, -d, 0, True)
        run_r &= ~np.where(E, ~shifted(E, d, 0, False), shifted(stop_r, d, 0, True))
        nl += run_l
        nr += run_r
    return nl, nr


@pytest.mark.gpu
@pytest.mark.parametrize("iw,ih,seed", FIXTURES)
def test_smooth_and_quant_bit_identical_at_tile_borders(iw, ih, seed):
    det = ra.Detector(iw, ih, nslots=1)
    for t, want in enumerate(oracle_frames(iw, ih, seed)):
        det.enqueue(synth.frame(synth.SEED0 + seed, iw, ih, t))
        det.poll(TAN36)
        for name in ("smooth", "quant"):
            a, b = det.plane(name, np.uint32), want[name].view(np.uint32)
            assert np.array_equal(a, b), f"{iw}x{ih} frame {t}: plane {name} differs in {int((a != b).sum())} pixels, first at {np.flatnonzero(a != b)[:4].tolist()}"
    det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nslots,group", [(6, 2), (32, 8)])
@pytest.mark.parametrize("iw,ih,seed", [(130, 109, 3), (64, 54, 1)])      # (64 x 54: the blur pair's own tile)
def test_group_launches_equal_the_single_slot_detector(iw, ih, seed, nslots, group):
    """the second and later frames of a group work on planes `zs` bytes behind the first's, and a group of 8 maps frames to XCDs: planes and lists must equal the
    single-slot detector's (whose first frames are pinned to the oracle as well)"""
    n = 2 * group
    frames = [synth.frame(synth.SEED0 + seed, iw, ih, t) for t in range(n)]
    outs = []
    for slots in (1, nslots):
        det = ra.Detector(iw, ih, nslots=slots, nworkers=1 if slots > 1 else 0)
        got = []
        if slots == 1:
            for f in frames:
                det.enqueue(f)
                got.append((det.poll(TAN36), det.last_segments(), det.plane("smooth", np.uint32), det.plane("quant", np.uint32)))
        else:
            for f in frames:
                det.enqueue(f)
            for _ in frames:
                got.append((det.poll(TAN36), det.last_segments(), det.plane("smooth", np.uint32), det.plane("quant", np.uint32)))
            assert det.frames_per_launch() == group
        det.close()
        outs.append(got)
    for t, want in enumerate(oracle_frames(iw, ih, seed)):
        assert np.array_equal(outs[0][t][2], want["smooth"].view(np.uint32)) and np.array_equal(outs[0][t][3], want["quant"].view(np.uint32)), f"single slot, frame {t}"
    for t, ((r1, s1, sm1, q1), (r2, s2, sm2, q2)) in enumerate(zip(*outs)):
        assert np.array_equal(sm1, sm2), f"frame {t} of {n} in groups of {group}: smooth differs in {int((sm1 != sm2).sum())} pixels"
        assert np.array_equal(q1, q2), f"frame {t} of {n} in groups of {group}: quant differs in {int((q1 != q2).sum())} pixels"
        assert helpers.rects_equal(r1, r2) and helpers.segments_equal(s1, s2), f"frame {t} of {n} in groups of {group}: lists differ"


def test_fixtures_cover_the_cases():
    """What the fixtures above must contain, from the oracle's planes (no GPU):
    - NMS responses (>= 1e-6: pixels the despeckle replaces) on the first and the last row and column of one fixture and inside it, and on a corner of a 64 x 30 tile where four tiles meet;
    - every run length 0..5 towards smaller and larger coordinates on both axes (the edge mask `edge500`);
    - a replaced pixel with as few candidates as synthetic frames offer.  "All eight neighbours have a response themselves: nothing to adopt" does NOT occur
      in the synthetic frames: over seeds 0..15 of six of these sizes (two frames each) no replaced pixel has fewer than ONE neighbour
      without a response inside the frame.  The nearest case is asserted instead - a single candidate, (65, 31, 14) - where eight of the nine cells of the
      search (the centre included) are skipped and the strict `<` has exactly one taker."""
    src = open(os.path.join(helpers.ROOT, "rectdetect_amd", "csrc", "rd_k_rect.hip")).read()
    assert (int(re.search(r"#define DS_ROWS (\d+)", src).group(1)), int(re.search(r"#define BE_ROWS (\d+)", src).group(1))) == (DS_ROWS, BE_ROWS), "the fixtures are placed by the kernels' tile heights"
    border_and_inside = corner = False
    seen = {k: set() for k in ("smaller x", "larger x", "smaller y", "larger y")}
    fewest = 9
    for iw, ih, seed in FIXTURES + [(130, 109, 3), (64, 54, 1)]:
        for planes in oracle_frames(iw, ih, seed):
            hot = planes["nms"].reshape(ih, iw) >= 1e-6
            border_and_inside |= bool(hot[0].any() and hot[-1].any() and hot[:, 0].any() and hot[:, -1].any() and hot[1:-1, 1:-1].any())
            ys, xs = np.nonzero(hot)
            # a corner of a despeckle tile where four tiles meet (not a corner of the frame): the last column / row of a tile with a tile beyond it, or the first with one before it
            on_x = ((xs % 64 == 63) & (xs + 1 < iw)) | ((xs % 64 == 0) & (xs > 0))
            on_y = ((ys % DS_ROWS == DS_ROWS - 1) & (ys + 1 < ih)) | ((ys % DS_ROWS == 0) & (ys > 0))
            corner |= bool((on_x & on_y).any())
            cand = sum((~shifted(hot, dx, dy, True)).astype(int) for dy in (-1, 0, 1) for dx in (-1, 0, 1))      # (outside the frame: no candidate)
            fewest = min(fewest, int(cand[hot].min()))
            E = planes["edge500"].reshape(ih, iw) != 0
            for key, a in zip(seen, runs_along_x(E) + tuple(r.T for r in runs_along_x(E.T))):
                seen[key] |= set(np.unique(a).tolist())
    assert border_and_inside and corner
    assert all(v == set(range(6)) for v in seen.values()), seen
    assert fewest == 1, fewest
