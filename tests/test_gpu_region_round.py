"""k_region_round (rectdetect_amd/csrc/rd_k_rect.hip) at the frame sizes where its 64 x 32 tiles end and where the first tile appears that lies inside the frame with
its one-pixel ring - such a tile runs the body without bounds tests -, on planes that keep the merge going for many launches, that leave tiles quiet next to busy
ones, and that change pixels in the first and the last lane of a wave (the ends of the wave shifts and of the edge-column loads).

Planes go through the region tap (rd_region_planes_device) at a budget of 8 launches and at the budget the ladder ends on, and are judged as tests/regioncases.py
judges its stage-0 cases: region0, rsize, region, boundarysrc, boundary and the flags of the launches against the oracle, int for int.  What the planes must do for
these comparisons to mean something is asserted from the oracle alone (test_inputs_reach_what_they_are_for, no GPU): launch_todo() restates one launch of
rdo_region_concurrent in numpy, is checked against it launch by launch, and says which pixels a launch changes.

Sixteen frames that alternate two of the inputs (as images) run in groups of 8 against a single-slot detector."""
import functools

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers
from tests import regioncases as rc

LIM = rc.LIM
TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
TW, TH = LIM["merge_tile"]        # 64 x 32: the tile of a block; a wave takes 8 rows of it
DEEP = 3                          # launches 3, 4, .. (the fourth on) run the instantiation that combines parents per block: RR_DEEP of rd_k_rect.hip
# (iw, ih): one tile and no inner tile; a one-pixel last tile column and row; partial last tiles; the smallest frame with an inner tile - tile (1, 1), border tiles
# on every side; partial last tiles next to the inner one
SHAPES = [(64, 32), (65, 33), (130, 70), (192, 96), (200, 100)]
INNER_SHAPES = [(192, 96), (200, 100)]
KINDS = ("uniform", "noise", "serpentine", "columns")
BUDGETS = (8, 0)                  # 8 launches, and what the ladder ends on (0: as the frame path does)


# ---------------------------------------------------------------------------------------------------------------- the inputs
def uniform(iw, ih):
    """one colour everywhere: one region, settled after the first launches - every wave quiet from then on"""
    return np.ones((ih, iw), np.int32), np.zeros((ih, iw), np.int32), np.zeros((ih, iw), np.int32)


def noise(iw, ih):
    """three colours at random, a merge mask on one pixel in 16 and a strong edge on one in 16: regions of a few pixels that settle at once next to chains of regions
    the masked pixels join one link per launch"""
    rng = np.random.default_rng(1000 * iw + ih)
    pix = rng.integers(0, 3, (ih, iw)).astype(np.int32)
    mask = (rng.integers(0, 16, (ih, iw)) == 0).astype(np.int32)
    edge = (rng.integers(0, 16, (ih, iw)) == 0).astype(np.int32) * 5
    return pix, mask, edge


PITCH = 10


def comb(iw, ih, xs):
    """A path one pixel wide of colour 1 on colour 0 that winds through the columns `xs`: vertical runs from row 3 to row ih - 3, joined alternately along row ih - 3 and
    along row 3, the rightmost pair at the bottom; the rightmost run goes on up to a corridor along row 1 that starts at column 1, which gives it the smallest label of
    the path.  The links of a pixel point up or to the left, so every pair of runs joined at the top is a tree of its own whose root lies left of and below the
    corridor: the small label enters a pair at the bottom of its right-hand run - the pixel of the join beside it adopts it and hooks the pair's root - and a launch
    later every pixel of the pair changes.  Two launches per pair, from right to left: no pointer jump shortens that."""
    pix = np.zeros((ih, iw), np.int32)
    xs = sorted(xs)
    for x in xs:
        pix[3:ih - 2, x] = 1
    pix[1:3, xs[-1]] = 1
    pix[1, 1:xs[-1]] = 1
    for r, (xa, xb) in enumerate(zip(xs[-2::-1], xs[:0:-1])):      # pairs of neighbouring runs from the right
        pix[ih - 3 if r % 2 == 0 else 3, xa:xb] = 1
    return pix, np.zeros((ih, iw), np.int32), np.zeros((ih, iw), np.int32)


def serpentine(iw, ih):
    """the comb on every tenth column from column 2"""
    return comb(iw, ih, range(2, iw - 2, PITCH))


def column_groups(iw, ih):
    """The chains of one-pixel columns, each as (columns in the order the small label visits them, their top rows, their masked rows, from_left).
    Across 63 | 64 the label travels from left to right, across 128 | 127 - where the frame has them - from right to left."""
    groups = []
    xs = list(range(TW - 4, TW + 3))                    # 60 .. 66: column 63 is lane 63 of its waves, column 64 lane 0 (its left neighbour comes from the edge-column load)
    tops = [34 + 3 * (TW + 2 - x) for x in xs]          # 52 .. 34: stepping up to the right
    groups.append((xs, tops, [t + 3 for t in tops], True))      # the masked pixel of a column lies on the row of its left neighbour's top
    if 2 * TW + 4 <= iw - 3:
        xs = list(range(2 * TW + 3, 2 * TW - 5, -1))    # 131 .. 124: column 128 is lane 0, column 127 lane 63 (its right neighbour comes from the edge-column load)
        groups.append((xs, [30] * len(xs), [36 + 3 * (x - (2 * TW - 4)) for x in xs], False))
    return groups


def columns(iw, ih):
    """Vertical regions one pixel wide, each of a colour of its own, on one background: columns 0 and iw - 1 (the ring: they never act) from top to bottom, and two chains
    of neighbouring columns that hand a small label on from column to column, late, through one masked pixel per column that strong edges fence in so that it can adopt
    from one side only.
      60 .. 66, from left to right.  The tops step up to the right, so a column's label is smaller than its left neighbour's; the masked pixel of column x lies beside
          the left neighbour's top, a root, which holds a larger label until it is hooked.  Column 59, the source, hangs on a column 58 that starts at row 2.
      131 .. 124, from right to left (frames that have them).  All tops on one row, so labels rise to the right; the source, column 132, starts at row 2.
    A column whose masked pixel adopts hooks its root, and in the next launch every pixel of it changes: column 63 (lane 63), then column 64 (lane 0, from column 63
    through the edge-column load), column 128 (lane 0), then column 127 (lane 63, from column 128 through that load).  The masked rows of columns 64 and 127 lie in the
    inner tile (1, 1) of the frames that have one."""
    pix, mask, edge = _blank(iw, ih)
    pix[:, 0], pix[:, iw - 1] = 8, 9
    colour = 10
    bottom = ih - 5
    for xs, tops, rows, from_left in column_groups(iw, ih):
        for x, t, y in zip(xs, tops, rows):
            pix[t:bottom, x] = colour
            colour += 1
            mask[y, x] = 1
            edge[y + 1, x] = 5                   # nothing from below ...
            if from_left:
                edge[y, x + 1] = 5               # ... nor from the right: from the left (and from its own column above) only
            else:
                edge[y, x] = 5                   # ... nor from the left or from above: from the right only
        if from_left:                            # the source: a column beside the first one's masked pixel, hanging on a column that starts at row 2
            pix[rows[0]:bottom, xs[0] - 1] = colour
            pix[2:rows[0] + 1, xs[0] - 2] = colour
        else:
            pix[2:bottom, xs[0] + 1] = colour
        colour += 1
    return pix, mask, edge


def _blank(iw, ih):
    return np.zeros((ih, iw), np.int32), np.zeros((ih, iw), np.int32), np.zeros((ih, iw), np.int32)


BUILDERS = dict(uniform=uniform, noise=noise, serpentine=serpentine, columns=columns)


def fits(kind, iw, ih):
    """the columns need a second tile column for their lane 0, and rows for their stairs"""
    return kind != "columns" or (iw >= TW + 6 and ih >= 64)


CASES = [(kind, iw, ih) for iw, ih in SHAPES for kind in KINDS if fits(kind, iw, ih)]


@functools.lru_cache(maxsize=None)
def planes(kind, iw, ih):
    p = BUILDERS[kind](iw, ih)
    for a in p:
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def needed(kind, iw, ih):
    """launches of the merge until one changes nothing (the quiet one counts)"""
    return rc.oracle_merge(*planes(kind, iw, ih), 1000)[1]


@functools.lru_cache(maxsize=None)
def expected(kind, iw, ih, launches):
    """the oracle's planes for a budget (0: the ladder's), as regioncases.expected computes them for its stage-0 cases: computed once, shared, read-only"""
    pix, mask, edge = planes(kind, iw, ih)
    budget, settled = rc.ladder_end(needed(kind, iw, ih), launches)
    region0, _ = rc.oracle_merge(pix, mask, edge, budget)
    rsize = rc.junction_counts(edge)
    helpers.oracle().rdo_region_size(helpers.P(rsize), helpers.P(region0), iw * ih)
    region, marks, comp = rc.oracle_absorb(region0, rsize, iw, ih)
    out = dict(budget=budget, settled=settled, region0=region0, rsize=rsize, region=region, boundarysrc=marks, boundary=comp)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- one launch, restated
def launch_todo(label, pix, mask, edge):
    """One launch of rdo_region_concurrent on the labels `label` (flat): (labels after it, 2-D map of the pixels that change their own label in it - `todo` of
    k_region_round).  A pixel inside the ring takes the smallest label among itself and the neighbours it may adopt from, follows the labels eight times, and where that
    differs from its label proposes it to itself and to its old label's pixel."""
    ih, iw = pix.shape
    lab = label.reshape(ih, iw)
    c = (slice(1, ih - 1), slice(1, iw - 1))
    g = lab[c].copy()
    anym = mask[c] != 0
    for dy, dx, at_self in ((-1, 0, True), (0, -1, True), (0, 1, False), (1, 0, False)):
        n = (slice(1 + dy, ih - 1 + dy), slice(1 + dx, iw - 1 + dx))
        ok = ((pix[c] == pix[n]) | anym) & ((edge[c] if at_self else edge[n]) <= 0)
        g = np.where(ok & (lab[n] < g), lab[n], g)
    for _ in range(8):
        g = label[g]
    og = lab[c]
    todo = g != og
    nxt = label.copy()
    p0 = (np.arange(ih * iw, dtype=np.int32).reshape(ih, iw))[c]
    np.minimum.at(nxt, og[todo], g[todo])
    np.minimum.at(nxt, p0[todo], g[todo])
    full = np.zeros((ih, iw), bool)
    full[c] = todo
    return nxt, full


@functools.lru_cache(maxsize=None)
def todo_maps(kind, iw, ih):
    """the todo map of every launch 0 .. needed - 1 (the last one is empty), each launch checked against the oracle's labels"""
    pix, mask, edge = planes(kind, iw, ih)
    label, _ = rc.oracle_merge(pix, mask, edge, 0)
    maps = []
    for l in range(needed(kind, iw, ih)):
        label, todo = launch_todo(label, pix, mask, edge)
        want, _ = rc.oracle_merge(pix, mask, edge, l + 1)
        assert np.array_equal(label, want), f"launch_todo is not the oracle's launch {l} on {kind} {iw}x{ih}"
        maps.append(todo)
    assert not maps[-1].any() and all(m.any() for m in maps[:-1])
    return maps


def tiles_changing(todo):
    ih, iw = todo.shape
    return np.array([[todo[y:y + TH, x:x + TW].any() for x in range(0, iw, TW)] for y in range(0, ih, TH)])


# ---------------------------------------------------------------------------------------------------------------- CPU: the inputs reach what they are for
def test_inputs_reach_what_they_are_for():
    assert (TW, TH) == (64, 32) and LIM["first_budget"] >= 8
    inner_busy = []
    for iw, ih in INNER_SHAPES:
        # an inner tile exists: tile (1, 1) and its ring lie inside the frame; at 64 .. 130 columns or 32 .. 70 rows none does
        assert 2 * TW + 1 <= iw and 2 * TH + 1 <= ih
        n = needed("serpentine", iw, ih)
        print("serpentine", iw, ih, "launches", n)
        assert n >= 10, (iw, ih, n)
        # noise: from the fourth launch on, a launch in which some tile changes nothing while another does; over the two frames an inner tile is busy in one such
        # launch and an inner tile is quiet in one
        maps = todo_maps("noise", iw, ih)
        mixed = [l for l in range(DEEP, len(maps)) if tiles_changing(maps[l]).any() and not tiles_changing(maps[l]).all()]
        inner = [bool(b) for l in mixed for b in tiles_changing(maps[l])[1:(ih - 1) // TH, 1:(iw - 1) // TW].reshape(-1)]
        print("noise", iw, ih, "launches", len(maps), "with quiet and busy tiles", mixed, "inner tiles busy", inner)
        assert mixed and inner, (iw, ih, len(maps), mixed, inner)
        inner_busy += inner
    assert True in inner_busy and False in inner_busy, inner_busy
    for iw, ih in [(w, h) for k, w, h in CASES if k == "columns"]:
        # columns: from the fourth launch on, every pixel of column 63 (lane 63 of its waves) changes in one launch and every pixel of column 64 (lane 0) in a later one,
        # which it can only have from column 63; where the frame has them, column 128 (lane 0) and then column 127 (lane 63) likewise
        maps = todo_maps("columns", iw, ih)
        for xs, tops, rows, from_left in column_groups(iw, ih):
            # (every pixel but the column's top, which is hooked, and the masked pixel, which has adopted the launch before)
            whole = lambda m, x, t, y: m[t + 1:y, x].all() and m[y + 1:ih - 5, x].all()
            first = {x: min([l for l in range(len(maps)) if whole(maps[l], x, t, y)], default=None) for x, t, y in zip(xs, tops, rows)}
            print("columns", iw, ih, "launches", len(maps), "from the left" if from_left else "from the right", "every pixel of a column changes first in launch", first)
            pair = (TW - 1, TW) if from_left else (2 * TW, 2 * TW - 1)
            # (the first column of a chain takes the label while the source's tree is still being flattened, in more than one step)
            assert None not in [first[x] for x in xs[1:]] and DEEP <= first[pair[0]] < first[pair[1]], (iw, ih, first)
            assert all(first[a] < first[b] for a, b in zip(xs[1:], xs[2:])), (iw, ih, first)      # one after the other: each has it from the one before
    for kind, iw, ih in CASES:
        n = needed(kind, iw, ih)
        assert 2 <= n <= LIM["max_launches"], (kind, iw, ih, n)       # every case settles inside the ladder: the budget it ends on is not the cap
    # the two budgets differ where it matters: the serpentine is cut short by a budget of 8 and settles on the ladder
    for iw, ih in INNER_SHAPES:
        e8, e0 = expected("serpentine", iw, ih, 8), expected("serpentine", iw, ih, 0)
        assert not e8["settled"] and e0["settled"] and not np.array_equal(e8["region0"], e0["region0"])


# ---------------------------------------------------------------------------------------------------------------- GPU: the tap against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("launches", BUDGETS, ids=("budget8", "ladder"))
@pytest.mark.parametrize("kind,iw,ih", CASES, ids=[f"{k}_{w}x{h}" for k, w, h in CASES])
def test_tap_against_oracle(kind, iw, ih, launches):
    e = expected(kind, iw, ih, launches)
    n = needed(kind, iw, ih)
    got = ra.region_planes_device(*planes(kind, iw, ih), launches=launches)
    print(kind, f"{iw}x{ih}", "needed", n, "budget", got.budget, "settled", got.settled, "flags", got.flags.tolist())
    assert (got.budget, got.settled) == (e["budget"], e["settled"])
    changed = np.arange(got.budget) < max(n, 2) - 1      # launch r changed something <=> it is not the quiet one or behind it
    assert np.array_equal(got.flags != 0, changed), (kind, iw, ih, got.flags.tolist())
    assert not got.info[got.budget:LIM["max_launches"]].any()
    for name in ("region0", "rsize", "region", "boundarysrc", "boundary"):
        a, b = getattr(got, name).reshape(-1), e[name]
        assert np.array_equal(a, b), f"{kind} {iw}x{ih} budget {launches}: plane {name} differs from the oracle in {int((a != b).sum())} ints, first at {np.flatnonzero(a != b)[:4].tolist()}"


# ---------------------------------------------------------------------------------------------------------------- GPU: groups of 8
PALETTE = np.array([[40 + 210 * (i & 1), 40 + 70 * ((i >> 1) & 3), 40 + 210 * (i >> 3)] for i in range(16)], np.uint8)


def image(kind, iw, ih):
    """an input as a frame: its colour plane through a palette of 16 colours, neighbouring numbers far apart (the detector's own front end makes the planes of the
    merge from it: not the planes of the tap cases, but two kinds of content)"""
    return np.ascontiguousarray(PALETTE[planes(kind, iw, ih)[0] % len(PALETTE)])


@pytest.mark.gpu
def test_group_launches_equal_the_single_slot_detector():
    """frames of a group work on planes `zs` bytes behind the first's, and a group's launches run until the last of its frames has settled: the merged labels and
    the regions of a 32-slot detector (groups of 8) must equal the single-slot detector's, frame by frame"""
    iw, ih = 200, 100
    pair = (image("noise", iw, ih), image("columns", iw, ih))
    seq = [pair[t % 2] for t in range(16)]
    outs = []
    for slots in (1, 32):
        det = ra.Detector(iw, ih, nslots=slots, nworkers=1 if slots > 1 else 0)
        got = []
        take = lambda: got.append((det.poll(TAN36), {p: det.plane(p, np.int32, det.N) for p in ("region0", "region")}))
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
    assert not np.array_equal(outs[0][0][1]["region0"], outs[0][1][1]["region0"]), "the two frames give the same labels: nothing alternates"
    for t, ((r1, p1), (r2, p2)) in enumerate(zip(*outs)):
        for p in p1:
            assert np.array_equal(p1[p], p2[p]), f"frame {t} of 16 in groups of 8: plane {p} differs in {int((p1[p] != p2[p]).sum())} ints"
        assert helpers.rects_equal(r1, r2), f"frame {t} of 16 in groups of 8: rectangle lists differ"
