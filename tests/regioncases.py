"""Crafted planes for the region stage (rd_k_rect.hip: k_region_init, k_region_round, k_region_size, k_absorb_tile, k_absorb_tail, despeckle2_slow; rd_k_label.hip:
label8_boundary), each with the claim it is built for.  What a case claims about itself is asserted from the oracle alone by tests/test_cpu_regioncases.py; the GPU
runs them through rd_region_planes_device in tests/test_gpu_regioncases.py.  Every edge comes from rectdetect_amd.region_limits(), none from a literal.

  stage 0  (pix, mask, edge) -> the merge and everything behind it.  The cascade sets the number of launches of the merge exactly; the two-wave cascade makes pixels
           change twice 1..28 launches apart (the marks of k_region_round repeat every 7); small planes for the details of the merge rule and the junction counts.
  stage 1  (region0, rsize) -> the absorption and everything behind it: chains against the tile kernel's halo, small-region cells per tile, undecided pixels around
           every capacity of the tail, reccap, ties of the first-maximum scan, the threshold, nothing to absorb, and a chain the tail's sweeps cannot finish.

Which pixels the tile kernel leaves undecided is the kernel's own property; tile_undecided() restates that rule (not the arithmetic) and gives the count as a range: the
rounds of a tile read cells other threads write in the same round, so a chain longer than the rounds may or may not be finished.  A case that names a count keeps to
planes where both ends of the range agree."""
import functools

import numpy as np

import rectdetect_amd as ra
from tests import helpers

LIM = ra.region_limits()
THRE = LIM["thre"]
MIN_SIDE = 16      # the smallest frame side a detector accepts (rd_detector_create), hence the tap


class Case:
    def __init__(self, name, claim, stage, planes, launches=0, **expect):
        self.name, self.claim, self.stage, self.planes, self.launches, self.expect = name, claim, stage, planes, launches, expect
        self.ih, self.iw = planes[0].shape

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------- the oracle
def oracle_merge(pix, mask, edge, limit):
    """rdo_region_concurrent with at most `limit` launches: (labels, launches evaluated - the quiet one counts)"""
    ih, iw = pix.shape
    lab = np.zeros(iw * ih, np.int32)
    a = [np.ascontiguousarray(p, dtype=np.int32) for p in (pix, mask, edge)]
    n = helpers.oracle().rdo_region_concurrent(helpers.P(lab), *[helpers.P(p) for p in a], iw, ih, int(limit))
    return lab, int(n)


def junction_counts(edge):
    ih, iw = edge.shape
    out = np.zeros(iw * ih, np.int32)
    O = helpers.oracle()
    O.rdo_junction(helpers.P(out), helpers.P(np.ascontiguousarray(edge, dtype=np.int32)), 0, iw, ih)
    return out


def oracle_absorb(region0, rsize, iw, ih):
    """(region, boundarysrc, boundary) of the serial raster order from labels and the size table"""
    O, P = helpers.oracle(), helpers.P
    region = np.ascontiguousarray(region0, dtype=np.int32).reshape(-1).copy()
    rsize = np.ascontiguousarray(rsize, dtype=np.int32).reshape(-1)
    O.rdo_despeckle2(P(region), P(rsize), THRE, iw, ih)
    marks = np.zeros(iw * ih, np.int32)
    O.rdo_mark_boundary(P(marks), P(region), iw, ih)
    comp = np.zeros(iw * ih, np.int32)
    O.rdo_label8(P(comp), P(marks), -1, iw, ih)
    return region, marks, comp


def jacobi_rounds(region0, rsize, iw, ih):
    """(result, rounds) of rdo_despeckle2_jacobi_k run to its fixed point"""
    lab = np.ascontiguousarray(region0, dtype=np.int32).reshape(-1).copy()
    r = helpers.oracle().rdo_despeckle2_jacobi_k(helpers.P(lab), helpers.P(np.ascontiguousarray(rsize, dtype=np.int32).reshape(-1)), THRE, iw, ih, None, 1 << 30)
    return lab, int(r)


def ladder_end(needed, launches=0):
    """(final budget, settled) of a frame whose merge needs `needed` launches (the quiet one counts; at least 2: launch 0 always counts as a change)"""
    needed = max(needed, 2)
    if launches:
        return launches, needed <= launches
    for b in [LIM["first_budget"]] + LIM["ladder"]:
        if needed <= b:
            return b, True
    return LIM["max_launches"], False


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = BY_NAME[name]
    iw, ih = c.iw, c.ih
    if c.stage == 0:
        pix, mask, edge = c.planes
        _, needed = oracle_merge(pix, mask, edge, 1000)
        budget, settled = ladder_end(needed, c.launches)
        region0, _ = oracle_merge(pix, mask, edge, budget)
        rsize = junction_counts(edge)
        helpers.oracle().rdo_region_size(helpers.P(rsize), helpers.P(region0), iw * ih)
    else:
        needed, budget, settled = 0, 0, True
        region0, rsize = (np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in c.planes)
    region, marks, comp = oracle_absorb(region0, rsize, iw, ih)
    _, rounds = jacobi_rounds(region0, rsize, iw, ih)
    lo, hi = tile_undecided(region0.reshape(ih, iw), rsize)
    out = dict(needed=needed, budget=budget, settled=settled, region0=region0, rsize=rsize, region=region, boundarysrc=marks, boundary=comp, jacobi_rounds=rounds, undecided=(lo, hi))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def expected(case):
    """the oracle's planes and figures for a case, computed once and shared (read-only)"""
    return _expected(case.name)


# ---------------------------------------------------------------------------------------------------------------- the tile kernel's rule, restated
def tile_undecided(region0, rsize, lim=None):
    """(least, most) pixels k_absorb_tile leaves undecided.  A tile loads its cells, AB_HK columns left and right, AB_HK rows above and one more ring; a small-region cell
    becomes exact once its predecessors NW, N, NE, W are exact; small-region cells on the loaded rim never are; a tile with more small-region cells than it can own (or
    none) runs no rounds.  most: every round reads only what the round before left (tile_rounds rounds); least: rounds that see every earlier write (the fixed point)."""
    lim = lim or LIM
    ih, iw = region0.shape
    tw, th = lim["absorb_tile"]
    hk, cap, rounds = lim["AB_HK"], lim["AB_OWNED"], lim["tile_rounds"]
    small_all = np.asarray(rsize).reshape(-1)[region0] <= lim["thre"]
    lw, lh = tw + 2 * hk + 2, th + hk + 2
    pad = np.zeros((ih + lh + th, iw + lw + tw), bool)      # small-region flags with room for every tile's loaded cells (outside the frame: not small)
    oy, ox = hk + 1, hk + 1
    pad[oy:oy + ih, ox:ox + iw] = small_all
    lo = hi = 0
    for by in range((ih + th - 1) // th):
        for bx in range((iw + tw - 1) // tw):
            cell = pad[by * th: by * th + lh, bx * tw: bx * tw + lw]
            own = np.zeros_like(cell)
            own[hk + 1: hk + 1 + th, hk + 1: hk + 1 + tw] = True
            inner = np.zeros_like(cell)
            inner[1:-1, 1:-1] = True
            ns = int((cell & inner).sum())
            if ns == 0:
                continue
            if ns > cap:
                k = int((cell & own).sum())
                lo, hi = lo + k, hi + k
                continue
            res = []
            for limit in (rounds, 1 << 30):
                inexact = cell.copy()
                for _ in range(limit):
                    ready = np.zeros_like(cell)
                    ready[1:-1, 1:-1] = inexact[1:-1, 1:-1] & ~(inexact[:-2, :-2] | inexact[:-2, 1:-1] | inexact[:-2, 2:] | inexact[1:-1, :-2])
                    if not ready.any():
                        break
                    inexact = inexact & ~ready
                res.append(int((inexact & own).sum()))
            hi, lo = hi + res[0], lo + res[1]
    return lo, hi


def absorb_with_ties(region0, rsize):
    """rc:348-371 in serial raster order, restated in Python: (result, {pixel: [positions of the scan order that hold the maximum]}) - positions 0..8 = NW, N, NE, W, C, E, SW,
    S, SE; only pixels where more than one position holds the maximum with DIFFERENT labels are listed"""
    ih, iw = region0.shape
    lab = region0.astype(np.int64).copy()
    size = np.asarray(rsize).reshape(-1)
    ties = {}
    for y in range(ih):
        for x in range(iw):
            if size[lab[y, x]] > THRE:
                continue
            cand = []
            for k, (dy, dx) in enumerate((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)):
                if 0 <= y + dy < ih and 0 <= x + dx < iw:
                    cand.append((k, int(lab[y + dy, x + dx])))
            best = max(int(size[l]) for _, l in cand)
            top = [(k, l) for k, l in cand if int(size[l]) == best]
            if len({l for _, l in top}) > 1:
                ties[(y, x)] = [k for k, _ in top]
            lab[y, x] = top[0][1] if best > 0 else lab[y, x]
    return lab.astype(np.int32), ties


# ---------------------------------------------------------------------------------------------------------------- stage 0: builders
def cascade(n, h, second=None):
    """n stripes two pixels wide from x = 2, stripe i of colour i + 1 on rows top..h-3; the last stripe's colour also fills row 1 from x = 1 to the stripe, which gives it the
    smallest label; the merge mask is set in the right-hand column of every stripe but the last.  A masked pixel adopts across colours only from its right neighbour and
    labels rise from left to right, so the low label walks left one stripe per two launches.  second = (stripe, row): that stripe gets a corridor of its own along `row`,
    and its label follows the first one through the same pixels."""
    iw = 2 * n + 4
    top = 2 if second is None else 6
    pix = np.zeros((h, iw), np.int32)
    mask = np.zeros((h, iw), np.int32)
    for i in range(n):
        pix[top:h - 2, 2 + 2 * i: 4 + 2 * i] = i + 1
        if i < n - 1:
            mask[top + 1:h - 3, 3 + 2 * i] = 1

    def corridor(i, row):
        pix[row, 1: 4 + 2 * i] = i + 1
        pix[row:top, 2 + 2 * i: 4 + 2 * i] = i + 1
    corridor(n - 1, 1)
    if second is not None:
        corridor(*second)
    return pix, mask, np.zeros((h, iw), np.int32)


def lag_table(pix, mask, edge):
    """{lag: pixels} over all pairs of successive changes of one pixel's label, from the oracle run with launch limits 1, 2, ..; and the launches it needs"""
    _, needed = oracle_merge(pix, mask, edge, 1000)
    prev, _ = oracle_merge(pix, mask, edge, 0)
    last = np.full(prev.shape, -1)
    table = {}
    for l in range(1, needed + 1):
        cur, _ = oracle_merge(pix, mask, edge, l)
        ch = cur != prev
        for lag in np.unique((l - last)[ch & (last >= 0)]):
            table[int(lag)] = table.get(int(lag), 0) + int(((l - last == lag) & ch & (last >= 0)).sum())
        last[ch] = l
        prev = cur
    return table, needed


def _blank(iw, ih):
    return np.zeros((ih, iw), np.int32), np.zeros((ih, iw), np.int32), np.zeros((ih, iw), np.int32)


ASYM_BLOCKS = {"up": (24, 34), "left": (44, 54), "down": (66, 78)}      # first column of the 3 x 3 block of each pair: (adoption refused, adoption allowed)


def asym_edge():
    """The edge test reads the plane at the pixel itself for an adoption from above or from the left, at the neighbour for one from the right or from below: of a pair
    of pixels it is always the right / lower one that counts.  One pair of planes per direction, in which that adoption alone decides a label; in the first of each pair
    the strong edge lies on the pixel the test reads (two regions), in the second on the other pixel of the pair (one region).
    right: two columns of one colour, the right one starting higher - it holds the smaller label and the columns are not linked to begin with; the left column's pixels
           join by adopting from the right.  Edges down the right column / down the left column.
    up, left, down: a 3 x 3 block of a colour of its own whose one masked pixel - the middle of its top row, of its left column, of its bottom row - has a single
           neighbour of another colour: the background above it, the background left of it, or, below it, a bar that runs left and up past the block's first row and
           so holds a smaller label than the block.  Edge on the masked pixel / on that neighbour for up and left, on the neighbour / on the masked pixel for down."""
    pix, mask, edge = _blank(90, 24)
    for x0, ex in ((4, 1), (14, 0)):
        pix[6:13, x0] = 5
        pix[4:13, x0 + 1] = 5
        edge[6:13, x0 + ex] = 9
    colour = 20
    for kind, (dy, dx) in (("up", (-1, 0)), ("left", (0, -1)), ("down", (1, 0))):
        for k, x0 in enumerate(ASYM_BLOCKS[kind]):
            colour += 1
            pix[8:11, x0:x0 + 3] = colour
            y, x = 9 + dy, x0 + 1 + dx                 # the masked pixel: the middle of the block's side that faces the neighbour
            mask[y, x] = 1
            if kind == "down":                         # the bar: under the block, then up its left side with a column of background between
                pix[11, x0 - 2:x0 + 4] = 40 + k
                pix[5:12, x0 - 2] = 40 + k
            reads = (y, x) if kind != "down" else (y + dy, x + dx)
            other = (y + dy, x + dx) if kind != "down" else (y, x)
            edge[reads if k == 0 else other] = 9
    return pix, mask, edge


def mask_directions():
    """a masked pixel adopts across colours, an unmasked one never: pairs of blocks of two colours side by side, the smaller label now in the right block, now in the left,
    the mask now on the side that can adopt (joins) and now on the side that already has the smaller label (stays apart)"""
    pix, mask, edge = _blank(40, 20)
    for k, (x0, low_right, mask_right) in enumerate(((2, True, False), (12, False, True), (22, True, True), (32, False, False))):
        ya, yb = (6, 3) if low_right else (3, 6)
        pix[ya:14, x0:x0 + 3] = 2 * k + 1
        pix[yb:14, x0 + 3:x0 + 6] = 2 * k + 2
        mask[8:11, x0 + 3 if mask_right else x0 + 2] = 1
    return pix, mask, edge


def ring_parent():
    """the frame's ring is never processed but its pixels are parents: masked ring pixels of another colour keep their labels, interior pixels that link to the ring hook it"""
    pix, mask, edge = _blank(20, 18)
    pix[0:8, 6:9] = 3        # a block that starts on the ring: the ring pixels are the roots of its columns
    pix[5:12, 8:14] = 3      # ... and an arm whose columns link to a later root until the merge hooks them
    pix[9, 0] = 7
    mask[9, 0] = 1           # a masked ring pixel never adopts
    pix[17, 10] = 8
    mask[17, 10] = 1
    pix[9, 1] = 6
    mask[9, 1] = 1           # its interior neighbour does
    return pix, mask, edge


def word_straddle(iw):
    """stripes two pixels wide whose tops step up towards the right (the smaller labels are on the right), the mask in every stripe's right-hand column, one group
    with a stripe boundary at x = 63 | 64 and one that ends at the frame's last column; a strong edge right of the last masked pixel of each group - at x = 64 and in the
    frame's last column - keeps the group from joining what lies to its right"""
    ih = 24
    pix, mask, edge = _blank(iw, ih)
    starts = [iw - 9]
    if iw >= 72:
        starts.append(56)
    for x0 in starts:
        for i in range(4):
            xa = x0 + 2 * i
            pix[8 - i:16, xa:xa + 2] = 10 + i + (x0 & 64)
            mask[11, xa + 1] = 1
        edge[11, x0 + 8] = 5
    pix[:, iw - 1] = 99
    # the edge bit of the frame's last column: two masked pixels of colours of their own beside the ring, strong edges on themselves (nothing from above or from the left) and below
    # them (nothing from there): the ring pixel to their right is all they can adopt from, and the first one's is a strong edge
    for y, blocked in ((17, True), (20, False)):
        pix[y, iw - 2] = 50 + y
        mask[y, iw - 2] = 1
        edge[y, iw - 2] = edge[y + 1, iw - 2] = 5
        edge[y, iw - 1] = 5 if blocked else 0
    return pix, mask, edge


def junction_threshold():
    """H2: the sizes start from the junction counts, at the label's own pixel.  Four regions of 15, 15, 16, 16 pixels whose first pixel is a strong edge: alone (count 1 -> 0)
    or with one strong neighbour (count 2).  15 + 0 and 16 + 0 are absorbed, 15 + 2 and 16 + 2 are kept."""
    pix, mask, edge = _blank(44, 18)
    for k, (npx, pair) in enumerate(((15, False), (15, True), (16, False), (16, True))):
        x0 = 4 + 10 * k
        cells = [(5 + j // 4, x0 + j % 4) for j in range(npx)]
        for (y, x) in cells:
            pix[y, x] = k + 1
        edge[5, x0] = 7
        if pair:
            edge[4, x0 - 1] = 7
    return pix, mask, edge


# ---------------------------------------------------------------------------------------------------------------- stage 1: builders
BG, BG_SIZE, SEED_SIZE = 0, 50, 1000


def _plane(iw, ih):
    """a plane of one large label (BG) and its size table; small pixels are added as labels of their own"""
    region0 = np.full((ih, iw), BG, np.int32)
    rsize = np.ones(iw * ih, np.int32)
    rsize[BG] = BG_SIZE
    return region0, rsize


def _own(region0, rsize, y, x, size=1):
    region0[y, x] = y * region0.shape[1] + x
    rsize[region0[y, x]] = size


def chain(length, kind, x0):
    """a run of `length` small-region pixels (labels of their own, sizes 1..thre) whose first pixel has ONE large predecessor, a seed of a size above everything else's: the
    seed's label reaches the run's end only through every pixel of it.  kind: row (interior row), last (the frame's last row), col, diag (down-right), anti (down-left);
    the run starts at column x0 (row x0 for col, diag, anti): just left or just right of a tile edge"""
    tw, th = LIM["absorb_tile"]
    m = 4
    if kind in ("row", "last"):
        iw, ih = x0 + length + m, 24
        y = 10 if kind == "row" else ih - 1
        cells = [(y, x0 + i) for i in range(length)]
        seed = (y, x0 - 1)
    elif kind == "col":
        iw, ih = max(MIN_SIDE, x0 + m), x0 + length + m
        cells = [(x0 + i, x0) for i in range(length)]
        seed = (x0 - 1, x0)
    elif kind == "diag":
        iw = ih = x0 + length + m
        cells = [(x0 + i, x0 + i) for i in range(length)]
        seed = (x0 - 1, x0 - 1)
    else:
        iw = ih = x0 + length + m
        cells = [(x0 + i, iw - 1 - x0 - i) for i in range(length)]
        seed = (x0 - 1, iw - x0)
    region0, rsize = _plane(iw, ih)
    for i, (y, x) in enumerate(cells):
        _own(region0, rsize, y, x, 1 + i % THRE)
    _own(region0, rsize, *seed, SEED_SIZE)
    return region0, rsize


def cells_per_tile(k):
    """k small-region cells in 3 x 3 blocks (chains of at most a few links) inside the first tile: with up to AB_R * AB_NT of them the tile owns and decides every one, with one
    more it runs no rounds and hands all of them to the tail"""
    tw, th = LIM["absorb_tile"]
    iw = ih = tw + 32
    region0, rsize = _plane(iw, ih)
    spots = [(y, x) for y in range(1, th) for x in range(1, tw) if y % 4 != 0 and x % 4 != 0][:k]
    assert len(spots) == k
    for i, (y, x) in enumerate(spots):
        _own(region0, rsize, y, x, 1 + i % THRE)
    _own(region0, rsize, 0, 0, SEED_SIZE)
    return region0, rsize


def stem_slab(n):
    """exactly n undecided pixels: a plane one tile wide; a stem of small-region pixels down column 0 that starts on the row the SECOND tile row loads as its rim - the tile
    above decides the stem (AB_HK + 1 links), the tile below can decide nothing that hangs on it -, and below the stem a slab of n small-region pixels in full rows and one
    partial row, every one of which hangs on the stem.  The seed above the stem reaches all of them."""
    tw, th = LIM["absorb_tile"]
    hk = LIM["AB_HK"]
    iw = tw
    rows = (n + iw - 1) // iw
    ih = th + rows + 2
    while ra.region_limits(iw, ih)["reccap"] < min(n, LIM["AT_CAP"]):      # room for n records: the plane grows until the fast path's list holds them
        ih += 1
    region0, rsize = _plane(iw, ih)
    for y in range(th - hk - 1, th):
        _own(region0, rsize, y, 0, 1 + y % THRE)
    _own(region0, rsize, th - hk - 2, 0, SEED_SIZE)
    for i in range(n):
        _own(region0, rsize, th + i // iw, i % iw, 1 + i % THRE)
    return region0, rsize


def all_small(iw, ih):
    """every pixel a label of its own and of size 1, but for six labels above the threshold: more undecided pixels than reccap = N / 4 - the fast path gives up"""
    region0 = np.arange(iw * ih, dtype=np.int32).reshape(ih, iw)
    rsize = np.ones(iw * ih, np.int32)
    for k, (fy, fx) in enumerate(((0.1, 0.2), (0.3, 0.8), (0.5, 0.5), (0.7, 0.1), (0.9, 0.6), (0.95, 0.95))):
        rsize[region0[int(fy * ih), int(fx * iw)]] = THRE + 1 + 3 * k
    return region0, rsize


def ties(seed, iw=24, ih=24):
    """labels of their own with sizes from a handful of values on both sides of the threshold: equal maxima under different labels in every position of the scan"""
    rng = np.random.default_rng(seed)
    region0 = np.arange(iw * ih, dtype=np.int32).reshape(ih, iw)
    rsize = rng.choice(np.array([1, 2, 3, THRE, THRE + 1, THRE + 1, 30, 30], np.int32), iw * ih).astype(np.int32)
    rsize[[0, 1, iw, iw + 1]] = (3, 3, 2, 1)      # (the centre itself can only win at the frame's first pixel: everywhere else a predecessor's neighbourhood holds it)
    big = THRE + 1
    rsize[region0[10:13, 10:13]] = ((big, big, big), (big, 1, big), (big, 30, 30))      # (S wins only over larger regions all around that are smaller than S and SE)
    return region0, rsize


def threshold():
    """two blocks inside one large region: the one whose size is the threshold is absorbed, the one a pixel larger is kept"""
    region0, rsize = _plane(32, 20)
    region0[4:8, 4:8] = 5
    rsize[5] = THRE
    region0[4:8, 16:20] = 6
    rsize[6] = THRE + 1
    return region0, rsize


def no_small():
    region0, rsize = _plane(70, 70)
    region0[:, 35:] = 9
    rsize[9] = 70 * 35
    rsize[BG] = 70 * 35
    return region0, rsize


def one_region():
    region0, rsize = _plane(70, 70)
    rsize[BG] = 70 * 70
    return region0, rsize


def zigzag(length):
    """a chain that changes direction at every link (predecessor NE, then NW, ..) down a narrow plane, the seed above it.  The tail's doubling follows W and N links only; along
    diagonal links a value moves one link per step, AT_SWEEPS sweeps of ceil(log2(side)) steps each; `length` is twice what they can cover, so the tail gives up"""
    iw, ih = MIN_SIDE, length + 8
    region0, rsize = _plane(iw, ih)
    for i in range(length):
        _own(region0, rsize, 3 + i, 6 + (i & 1), 1 + i % THRE)
    _own(region0, rsize, 2, 7, SEED_SIZE)
    return region0, rsize


def sweep_steps(iw, ih):
    n = 1
    while (1 << n) < max(iw, ih):
        n += 1
    return n


# ---------------------------------------------------------------------------------------------------------------- the cases
CASCADE_N = (9, 10, 11, 16, 17, 32, 33, 64, 65)      # 2n launches: one below, on and one past the first budget and every step of the ladder; 65 is the unsettled frame
CASCADE_H = (MIN_SIDE, 70)                           # 70 crosses the 32-row block of the rounds and the 64-row tile of the absorption
CASCADE_H_ORACLE = (12,) + CASCADE_H                 # (12: smaller than a detector accepts - the claim about the launches is checked there as well)
TWO_WAVE = dict(n=8, k=14, launches=30, lags=(7, 14, 21, 28))


def _two_wave(h):
    return cascade(TWO_WAVE["n"] + TWO_WAVE["k"], h, second=(TWO_WAVE["n"] - 1, 3))


def _undecided_counts():
    nt, cap = LIM["AT_NT"], LIM["AT_CAP"]
    steps = [nt] + [e * nt for e in LIM["EPT"] if e * nt < cap]
    return sorted({s + d for s in steps for d in (-1, 0, 1)} | {cap - 1, cap, cap + 1})


def all_cases():
    hk = LIM["AB_HK"]
    tw = LIM["absorb_tile"][0]
    cases = []
    for h in CASCADE_H:
        for n in CASCADE_N:
            cases.append(Case(f"cascade_n{n}_h{h}", f"the merge needs exactly {2 * n} launches", 0, cascade(n, h), needed=2 * n))
    for b in (2, 8, 20):
        cases.append(Case(f"cascade_n16_budget{b}", f"a budget of {b} launches keeps what that many launches made of the frame", 0, cascade(16, MIN_SIDE), launches=b, needed=32))
    for h in (MIN_SIDE, 70):
        cases.append(Case(f"two_wave_h{h}", "pixels change twice 1..28 launches apart: every distance at which a mark of k_region_round repeats", 0, _two_wave(h), needed=TWO_WAVE["launches"]))
    cases.append(Case("asym_edge", asym_edge.__doc__, 0, asym_edge()))
    cases.append(Case("mask_directions", mask_directions.__doc__, 0, mask_directions()))
    cases.append(Case("ring_parent", ring_parent.__doc__, 0, ring_parent()))
    for iw in (63, 64, 65, 127, 128, 129):
        cases.append(Case(f"word_straddle_w{iw}", word_straddle.__doc__, 0, word_straddle(iw)))
    cases.append(Case("junction_threshold", junction_threshold.__doc__, 0, junction_threshold()))
    # stage 1
    for kind in ("row", "last", "col", "diag", "anti"):
        for length in (hk - 1, hk, hk + 1, 200):
            for x0 in (tw - 1, tw):
                cases.append(Case(f"chain_{kind}_{length}_at{x0}", chain.__doc__, 1, chain(length, kind, x0), status0=0, slow=False, seed_reaches=length))
    for k in (LIM["AB_OWNED"] - 1, LIM["AB_OWNED"], LIM["AB_OWNED"] + 1):
        cases.append(Case(f"cells_per_tile_{k}", cells_per_tile.__doc__, 1, cells_per_tile(k), status0=0, slow=False, undecided=0 if k <= LIM["AB_OWNED"] else k))
    for n in _undecided_counts():
        over = n > LIM["AT_CAP"]
        cases.append(Case(f"undecided_{n}", stem_slab.__doc__, 1, stem_slab(n), status0=int(over), slow=over, undecided=n, seed_reaches=n))
    for iw, ih in ((128, 128), (120, 80), (64, 64)):
        cases.append(Case(f"all_small_{iw}x{ih}", all_small.__doc__, 1, all_small(iw, ih), status0=1, slow=True, undecided=iw * ih - 6))
    for seed in (4, 5):
        cases.append(Case(f"ties_seed{seed}", ties.__doc__, 1, ties(seed), status0=0, slow=False))
    cases.append(Case("threshold", threshold.__doc__, 1, threshold(), status0=0, slow=False, undecided=0))
    cases.append(Case("no_small", "no small region at all", 1, no_small(), status0=0, slow=False, undecided=0))
    cases.append(Case("one_region", "the plane is one region", 1, one_region(), status0=0, slow=False, undecided=0))
    zl = 1
    while zl != 2 * LIM["AT_SWEEPS"] * sweep_steps(*zigzag(zl)[0].shape[::-1]):      # twice what the sweeps cover on the plane the chain itself needs: to the fixed point
        zl = 2 * LIM["AT_SWEEPS"] * sweep_steps(*zigzag(zl)[0].shape[::-1])
    cases.append(Case("zigzag_sweeps", zigzag.__doc__, 1, zigzag(zl), status0=1, slow=True, sweeps=LIM["AT_SWEEPS"], seed_reaches=zl))
    return cases


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
