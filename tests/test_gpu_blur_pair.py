"""The blur pair (k_blblur_pair, 64 x 54 tiles on a staged 62 x 72 strip) against the oracle at the sizes where its ownership can go wrong: thread (wave wv, lane tx)
owns strip rows 8 wv + j at frame column x0 + tx in staging, in the horizontal and in the vertical pass, so what matters is where tiles, halo columns and the
waves' row ranges end.  `smooth` (ten pairs) must be bit-identical to the oracle's, frame by frame and inside group launches of eight.  What the fixtures must
contain for that to mean something is asserted on the CPU from the oracle's edge mask (test_fixtures_reach_into_the_halo; it needs no GPU)."""
import os
import re

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers
from tests.test_gpu_small_dense import NFRAMES, TAN36, oracle_frames, runs_along_x

TILE_W, TILE_H = 64, 54        # the blur pair's tile: 64 lanes x BQ_ROWS of rectdetect_amd/csrc/rd_k_rect.hip - keep them equal
SEED = 0
# 60x50 / 64x54 / 68x58: one tile short of, equal to and beyond the tile in both directions (halo columns 0..3 / 68..71 at the frame's edge);
# 69x59: a second tile column and row of 5 pixels each; 67x57, 68x58: a second tile row of 3 and 4 rows (wave 0's four and wave 7's two output rows at the
# frame's bottom); 132x112: tile (1, 1) is interior with both bounds tight (x0 + 68 == iw, y0 + 58 == ih); 131x111: the same tile on the border path;
# 200x170: an interior tile with neighbours on all sides
SHAPES = [(60, 50), (64, 54), (68, 58), (69, 59), (67, 57), (132, 112), (131, 111), (200, 170)]
HALO_SHAPES = [(69, 59), (131, 111), (132, 112), (200, 170)]


@pytest.mark.gpu
@pytest.mark.parametrize("iw,ih", SHAPES)
def test_smooth_bit_identical(iw, ih):
    det = ra.Detector(iw, ih, nslots=1)
    for t, want in enumerate(oracle_frames(iw, ih, SEED)):
        det.enqueue(synth.frame(synth.SEED0 + SEED, iw, ih, t))
        det.poll(TAN36)
        a, b = det.plane("smooth", np.uint32), want["smooth"].view(np.uint32)
        assert np.array_equal(a, b), f"{iw}x{ih} frame {t}: plane smooth differs in {int((a != b).sum())} pixels, first at {np.flatnonzero(a != b)[:4].tolist()}"
    det.close()


@pytest.mark.gpu
def test_groups_of_eight_equal_the_single_slot_detector():
    """groups of eight: frame z works on planes `zs` bytes behind the first's and the tiles of a frame go to one XCD; `smooth` and the lists must equal the
    single-slot detector's, whose first frames are pinned to the oracle"""
    iw, ih, group = 132, 112, 8
    n = 2 * group
    frames = [synth.frame(synth.SEED0 + SEED, iw, ih, t) for t in range(n)]
    det = ra.Detector(iw, ih, nslots=1)
    one = []
    for f in frames:
        det.enqueue(f)
        one.append((det.poll(TAN36), det.last_segments(), det.plane("smooth", np.uint32)))
    det.close()
    det = ra.Detector(iw, ih, nslots=32, nworkers=1)
    many = []
    for f in frames:
        det.enqueue(f)
    for _ in frames:
        many.append((det.poll(TAN36), det.last_segments(), det.plane("smooth", np.uint32)))
    assert det.frames_per_launch() == group
    det.close()
    for t, want in enumerate(oracle_frames(iw, ih, SEED)):
        assert np.array_equal(one[t][2], want["smooth"].view(np.uint32)), f"single slot, frame {t}"
    for t, ((r1, s1, sm1), (r2, s2, sm2)) in enumerate(zip(one, many)):
        assert np.array_equal(sm1, sm2), f"frame {t} of {n} in groups of {group}: smooth differs in {int((sm1 != sm2).sum())} pixels"
        assert helpers.rects_equal(r1, r2) and helpers.segments_equal(s1, s2), f"frame {t} of {n} in groups of {group}: lists differ"


@pytest.mark.parametrize("iw,ih", HALO_SHAPES)
def test_fixtures_reach_into_the_halo(iw, ih):
    """Each of these fixtures holds every run length 0..5 towards smaller and towards larger coordinates on both axes among the pixels within four cells of a
    border between two blur tiles - the pixels whose window reaches into the halo columns (runs along x) or the halo rows (runs along y) of a tile.
    From the oracle's edge mask `edge500` (no GPU).  If a change of the synthetic stream breaks this, pick another seed rather than weaken the condition."""
    src = open(os.path.join(helpers.ROOT, "rectdetect_amd", "csrc", "rd_k_rect.hip")).read()
    assert int(re.search(r"#define BQ_ROWS (\d+)", src).group(1)) == TILE_H, "the fixtures are placed by the kernel's tile height"
    xs, ys = np.arange(iw), np.arange(ih)
    # within four cells of a tile border that has a tile on both sides
    bx = ((xs % TILE_W < 4) & (xs >= TILE_W)) | ((xs % TILE_W >= TILE_W - 4) & (xs - xs % TILE_W + TILE_W < iw))
    by = ((ys % TILE_H < 4) & (ys >= TILE_H)) | ((ys % TILE_H >= TILE_H - 4) & (ys - ys % TILE_H + TILE_H < ih))
    seen = {k: set() for k in ("smaller x", "larger x", "smaller y", "larger y")}
    frames = oracle_frames(iw, ih, SEED)
    assert len(frames) == NFRAMES
    for planes in frames:
        E = planes["edge500"].reshape(ih, iw) != 0
        nl, nr = runs_along_x(E)
        nu, nd = (r.T for r in runs_along_x(E.T))
        for key, a in zip(seen, (nl[:, bx], nr[:, bx], nu[by, :], nd[by, :])):
            seen[key] |= set(np.unique(a).tolist())
    assert all(v == set(range(6)) for v in seen.values()), seen
