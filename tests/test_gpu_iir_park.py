"""The blocked IIR blur (k_iir_fused / k_iir_fused_edge / k_iir_check_fix, rectdetect_amd/csrc/rd_k_front.hip) at the smallest sizes that reach each of its
paths: interior blocks (a block with 32 run-in rows on either side: H >= 2 * rows + 32; their parked half lives in registers, the sweeps swap state at
mid-block), edge blocks (first and last of a column, mirrored rows, the LDS tile), a remainder of fewer than 8 rows merged into the last block, partial
64-column strips, the transposed output of the pass along x and the full-length fix path.  Single frames and the operator API use 64-row blocks, group
launches 128-row blocks (GROUP_ROWS: keep it equal to IF_GROUP_ROWS).  Everything is compared bit for bit: the operator against rdo_iirblur, the frame path's
`lblur`, `plab1` (a and b through their quantisation) and `nms` against the oracle's planes.

Inputs: a frame of the bench generator, and a frame whose columns alternate 0 / 255 in blocks of 3 - the hardest drive of the recurrence along x; along y the
same pattern transposed is used for the operator.  The on-device check of the 32 run-in rows must still pass on both (`iirflags` zero)."""
import functools
import os
import re

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
GROUP_ROWS = 128
SEED = 5
PLANES = [("lblur", "Lblur"), ("plab1", "plab1"), ("nms", "nms")]      # detector's name, oracle's name
OP_SIZES = [(170, 165), (64, 200), (200, 64), (97, 61), (128, 192)]      # (iw, ih): one interior block each way and a partial strip; one pass interior, the other edges only (twice); no interior block; whole blocks only, each way
FRAME_SIZES = [(170, 165), (300, 290), (192, 128)]      # the last: multiples of 64 - the last block of a column is a whole one
GROUP_SIZES = [(300, 290), (389, 261), (384, 256)]      # (the last: multiples of 128 - the last block of a column is a whole one) interior 128-row blocks both ways, width no multiple of 64; 261 = 2 * 128 + 5: the remainder joins the last block


def stripes(iw, ih):
    f = np.zeros((ih, iw, 3), np.uint8)
    f[:, (np.arange(iw) // 3) % 2 == 1] = 255
    return f


@functools.lru_cache(maxsize=None)
def frames(iw, ih):
    f = {"synth": synth.frame(synth.SEED0 + SEED, iw, ih, 0), "stripes": stripes(iw, ih)}
    for a in f.values():
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def stream(iw, ih):
    """16 distinct frames, interleaved: synthetic frames of a stream and striped frames shifted by one column each"""
    out = []
    for t in range(16):
        a = synth.frame(synth.SEED0 + SEED, iw, ih, t // 2) if t % 2 == 0 else np.roll(stripes(iw, ih), t // 2, axis=1)
        a = np.ascontiguousarray(a)
        a.setflags(write=False)
        out.append(a)
    return out


def oracle_of(iw, ih, imgs):
    orc = helpers.OracleRect(iw, ih, helpers.REGION_SPEC)
    out = []
    for img in imgs:
        orc.frame(img)
        out.append({d: orc.plane(o).view(np.uint32) for d, o in PLANES})
    orc.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_frames(iw, ih):
    names = sorted(frames(iw, ih))
    return dict(zip(names, oracle_of(iw, ih, [frames(iw, ih)[n] for n in names])))


@functools.lru_cache(maxsize=None)
def oracle_stream(iw, ih):
    return oracle_of(iw, ih, stream(iw, ih))


def det_planes(det):
    return {d: det.plane(d, np.uint32) for d, _ in PLANES}


def assert_planes(got, want, what):
    for d, _ in PLANES:
        assert np.array_equal(got[d], want[d]), f"{what}: plane {d} differs in {int((got[d] != want[d]).sum())} words, first at {np.flatnonzero(got[d] != want[d])[:4].tolist()}"


def test_group_rows_is_the_kernels():
    src = open(os.path.join(helpers.ROOT, "rectdetect_amd", "csrc", "rd_k_front.hip")).read()
    assert int(re.search(r"#define IF_GROUP_ROWS (\d+)", src).group(1)) == GROUP_ROWS, "the grouped sizes are placed by the block height of group launches"
    assert int(re.search(r"#define IF_WU (\d+)", src).group(1)) == 32
    assert 261 % GROUP_ROWS == 5 and 389 >= 2 * GROUP_ROWS + 32 and 300 >= 2 * GROUP_ROWS + 32 and 290 >= 2 * GROUP_ROWS + 32


# ---- 1. the operator API: one float plane, both passes, 64-row blocks
@pytest.mark.gpu
@pytest.mark.parametrize("iw,ih", OP_SIZES)
def test_operator_against_oracle(iw, ih):
    ctx = ra.Context(0)
    L = ra.lib()
    iu = L.init_oclimgutil(ctx.device, ctx.context)
    O = helpers.oracle()
    f = frames(iw, ih)
    planes = {"synth": f["synth"][:, :, 1].astype(np.float32) / 255, "stripes_x": f["stripes"][:, :, 0].astype(np.float32),
              "stripes_y": np.ascontiguousarray(stripes(ih, iw)[:, :, 0].T).astype(np.float32)}
    try:
        for name, x in planes.items():
            x = np.ascontiguousarray(x)
            assert x.shape == (ih, iw)
            a, o, t0, t1 = ctx.buffer(x), ctx.buffer(iw * ih * 4), ctx.buffer(iw * ih * 4), ctx.buffer(iw * ih * 4)
            L.oclimgutil_iirblur_f_f(iu, o, a, t0, t1, 2, iw, ih, ctx.queue, None)
            got = ctx.read(o, np.float32, iw * ih).view(np.uint32)
            ctx.release(a, o, t0, t1)
            want = np.zeros(iw * ih, np.float32)
            O.rdo_iirblur(helpers.P(want), helpers.P(x), iw, ih)
            want = want.view(np.uint32)
            assert np.array_equal(got, want), f"{iw}x{ih} {name}: {int((got != want).sum())} words differ, first at {np.flatnonzero(got != want)[:4].tolist()}"
    finally:
        L.dispose_oclimgutil(iu)
        ctx.close()


# ---- 2. the frame path, one slot (64-row blocks)
@pytest.mark.gpu
@pytest.mark.parametrize("iw,ih", FRAME_SIZES)
def test_single_frames_against_oracle(iw, ih):
    det = ra.Detector(iw, ih, nslots=1)
    try:
        for name in sorted(frames(iw, ih)):
            det.enqueue(frames(iw, ih)[name])
            det.poll(TAN36)
            assert_planes(det_planes(det), oracle_frames(iw, ih)[name], f"{iw}x{ih} frame {name}")
            assert det.plane("iirflags", np.int32, 16)[:2].tolist() == [0, 0], f"{iw}x{ih} frame {name}: the run-in check failed"
    finally:
        det.close()


# ---- 3. the frame path in group launches (128-row blocks)
@pytest.mark.gpu
@pytest.mark.parametrize("iw,ih", GROUP_SIZES)
def test_group_launches_against_single_slot_and_oracle(iw, ih):
    seq = stream(iw, ih)
    outs = []
    for slots in (1, 32):
        det = ra.Detector(iw, ih, nslots=slots, nworkers=1 if slots > 1 else 0)
        got = []
        try:
            if slots == 1:
                for fr in seq:
                    det.enqueue(fr)
                    det.poll(TAN36)
                    got.append((det_planes(det), det.plane("iirflags", np.int32, 16)[:2].tolist()))
            else:
                for fr in seq:
                    det.enqueue(fr)
                for _ in seq:
                    det.poll(TAN36)
                    got.append((det_planes(det), det.plane("iirflags", np.int32, 16)[:2].tolist()))
                assert det.frames_per_launch() >= 6, "group launches of at least 6 frames: nz > 1, the 128-row form"
        finally:
            det.close()
        outs.append(got)
    want = oracle_stream(iw, ih)
    for t, ((p1, f1), (pg, fg)) in enumerate(zip(*outs)):
        assert f1 == [0, 0] and fg == [0, 0], f"{iw}x{ih} frame {t}: the run-in check failed ({f1}, {fg})"
        assert_planes(pg, p1, f"{iw}x{ih} frame {t} of 16, grouped against one slot")
        assert_planes(pg, want[t], f"{iw}x{ih} frame {t} of 16, grouped against the oracle")
        assert_planes(p1, want[t], f"{iw}x{ih} frame {t} of 16, one slot against the oracle")


# ---- 4. the fix path is still reachable
@pytest.mark.gpu
def test_forced_fix_reproduces_the_planes(monkeypatch):
    iw, ih = 300, 290
    img = frames(iw, ih)["synth"]
    det = ra.Detector(iw, ih, nslots=1)
    det.enqueue(img)
    det.poll(TAN36)
    want = det_planes(det)
    assert det.plane("iirflags", np.int32, 16)[:2].tolist() == [0, 0]
    det.close()
    assert_planes(want, oracle_frames(iw, ih)["synth"], "300x290 without the fix")
    monkeypatch.setenv("RD_IIR_FORCE_FIX", "1")
    det = ra.Detector(iw, ih, nslots=1)
    det.enqueue(img)
    det.poll(TAN36)
    got, flags = det_planes(det), det.plane("iirflags", np.int32, 16)[:2].tolist()
    det.close()
    assert flags == [1, 1]
    assert_planes(got, want, "300x290 with every column of block 0 evaluated again")
