"""Crafted chains and boundary planes for the vote stage (rd_k_rect.hip: k_reduce_clean, k_reduce_claim, k_reduce_box) and the sampling kernel behind it
(k_sample_segments), with a restatement of the contract and what every case claims about it.  Asserted without a GPU by tests/test_cpu_votecases.py, run through
rd_votes_planes_device by tests/test_gpu_votecases.py.

The contract (oclrect.cl:427-464, reduceLS, in its canonical reading: SURVEY.md H9).  Pixels in raster order; a pixel that carries a segment id visits the cells of
its 7 x 7 window (clipped to the frame) in raster order; a cell holding a boundary id b > 0 is a TOUCH of slot ((id * b mod 2^32) & 0x7fffffff) % nentry, nentry =
iw * ih * 4 / 5.  A touch of a slot whose word 0 is 0 CLAIMS it (word 0 <- id) and does nothing else; a touch of a slot claimed by the pixel's own id WIDENS its box
(words 1..4 <- max with iw - x, x, ih - y, y of the PIXEL); a touch of a slot claimed by another id is dropped.  restate() below evaluates exactly that, one touch
after the other, and keeps a log of every touch; it shares no code with the oracle's rdo_reduce_ls.

A case is a mask (a few straight lines and outlines), the parameters of the polyline stage, and a painter that gets the oracle's id plane and list for the mask
(rdo_polyline) and returns the boundary plane: ids are painted freely, wherever the case needs them.  Every number a case is placed by comes from
rectdetect_amd.votes_limits(); tests/test_cpu_votecases.py also reads them out of the kernels' source."""
import numpy as np

import rectdetect_amd as ra
from tests import polycases as pc
from tests.postcases import probe_pixels

LIM = ra.votes_limits()
RB_MAX, CA_T, BA_T, BLOCK, GRID, MAXB, CLAIM_NONE = (LIM[k] for k in ("RB_MAX", "CA_T", "BA_T", "block", "grid", "MAXB", "CLAIM_NONE"))
SMALL, WIDE = (96, 64), (320, 64)      # (iw, ih)
GUARD = 0x5a5a5a5a


def nentry_of(iw, ih):
    return iw * ih * 4 // 5


def slot_of(i, b, nentry):
    """the slot of (segment i, boundary id b), both positive: the product wraps at 2^32, bit 31 is masked off"""
    return (((i * b) & 0xFFFFFFFF) & 0x7FFFFFFF) % nentry


# ---- the contract, restated
class Ref:
    """restate()'s result: table (nentry x 5), touches = [(pixel, id, b, slot, what)] in the order they happen (what: 'claim', 'widen', 'dropped'),
    owner = {slot: (pixel, id, b)} of the claiming touch"""

    def __init__(self, table, touches, owner):
        self.table, self.touches, self.owner = table, touches, owner
        self.table.setflags(write=False)

    def slots(self):
        return sorted(self.owner)


def restate(boundary, lsid):
    boundary, lsid = np.asarray(boundary), np.asarray(lsid)
    ih, iw = lsid.shape
    nentry = nentry_of(iw, ih)
    table = np.zeros((nentry, 5), np.int32)
    touches, owner = [], {}
    for p in np.flatnonzero(lsid.reshape(-1) > 0):
        y, x = divmod(int(p), iw)
        if x <= 0 or y <= 0 or x >= iw - 1 or y >= ih - 1:      # (oclrect.cl:429: the kernel leaves the frame's outermost pixels out)
            continue
        i = int(lsid[y, x])
        for yy in range(max(y - 3, 0), min(y + 4, ih)):
            for xx in range(max(x - 3, 0), min(x + 4, iw)):
                b = int(boundary[yy, xx])
                if b <= 0:
                    continue
                s = slot_of(i, b, nentry)
                e = table[s]
                if e[0] == 0:
                    e[0] = i
                    owner[s] = (int(p), i, b)
                    touches.append((int(p), i, b, s, "claim"))
                elif e[0] != i:
                    touches.append((int(p), i, b, s, "dropped"))
                else:
                    e[1], e[2], e[3], e[4] = max(e[1], iw - x), max(e[2], x), max(e[3], ih - y), max(e[4], y)
                    touches.append((int(p), i, b, s, "widen"))
    return Ref(table, touches, owner)


# ---- a case and what it resolves to
class Case:
    def __init__(self, name, size, mask, paint, ring=0, minerror=1.0, size_thre=10, claims=None):
        self.name, self.size, self.mask, self.paint, self.ring, self.minerror, self.size_thre, self.claims = name, size, mask, paint, ring, minerror, size_thre, claims or {}

    def __repr__(self):
        return self.name

    def params(self):
        return (self.size, self.ring, self.minerror, self.size_thre)


class Resolved:
    """mask, boundary (2-D), segs / ids (the oracle's list and id plane), live (pixel indices of the chains longer than size_thre, raster order: the vote kernels'
    work list), ref (restate's result)"""


_resolved = {}


def resolve(case):
    """computed once per case and shared by every test; nothing in it is writable"""
    if case.name not in _resolved:
        iw, ih = case.size
        r = Resolved()
        r.mask = np.ascontiguousarray(case.mask(), dtype=np.int32)
        assert r.mask.shape == (ih, iw), case.name
        r.segs, ids, info = pc.oracle_run(r.mask, case.ring, case.minerror, case.size_thre)
        r.ids = ids.reshape(ih, iw)
        r.live_count, r.chains = info["live"], info["chains"]
        r.boundary = np.ascontiguousarray(case.paint(r), dtype=np.int32)
        assert r.boundary.shape == (ih, iw), case.name
        r.nentry = nentry_of(iw, ih)
        r.ref = restate(r.boundary, r.ids)
        for a in (r.mask, r.ids, r.boundary, r.segs):
            a.setflags(write=False)
        _resolved[case.name] = r
    return _resolved[case.name]


# ---- what a case is, from the restatement's log
def facts(case):
    r = resolve(case)
    ih, iw = r.ids.shape
    ref = r.ref
    f = {}
    # distinct positive ids per window of a pixel with an id
    per_pixel = {}
    for p, i, b, s, what in ref.touches:
        per_pixel.setdefault(p, {}).setdefault(b, 0)
        per_pixel[p][b] += 1
    f["distinct"] = sorted({len(v) for v in per_pixel.values()})
    f["slots"] = len(ref.owner)
    f["zero_box_slots"] = int(np.count_nonzero((ref.table[:, 0] != 0) & (ref.table[:, 1:] == 0).all(axis=1)))
    # the vote kernels' blocks: BLOCK consecutive pixels with an id, raster order (pixels without an id on the work list do nothing); per block the distinct
    # slots it touches (the claim kernel's hash holds CA_T) and the distinct slots it widens (the box kernel's holds BA_T)
    order = {int(p): k for k, p in enumerate(np.flatnonzero(r.ids.reshape(-1) > 0))}
    touched, widened = {}, {}
    for p, i, b, s, what in ref.touches:
        blk = order[p] // BLOCK
        touched.setdefault(blk, set()).add(s)
        if what == "widen":
            widened.setdefault(blk, set()).add(s)
    f["touched_per_block"] = [len(touched[k]) for k in sorted(touched)]
    f["widened_per_block"] = [len(widened[k]) for k in sorted(widened)]
    # pairs per slot
    pairs, by_pixel = {}, {}
    for p, i, b, s, what in ref.touches:
        pairs.setdefault(s, set()).add((i, b))
        by_pixel.setdefault((s, p), set()).add(b)
    f["same_window"] = {s: sorted(v) for (s, p), v in by_pixel.items() if len(v) > 1}      # two ids of ONE window on one slot
    f["two_segments"] = {s: (ref.owner[s][1], sorted({i for i, _ in v} - {ref.owner[s][1]})) for s, v in pairs.items() if len({i for i, _ in v}) > 1}      # slot: (owner, losers)
    f["two_ids_apart"] = sorted(s for s, v in pairs.items() if len({i for i, _ in v}) == 1 and len({b for _, b in v}) > 1 and s not in f["same_window"])      # one segment, two ids, never in one window
    # how often the claiming pixel's own window touches the slot it claims (the first of them claims, the others widen)
    own = {}
    for p, i, b, s, what in ref.touches:
        if ref.owner[s][0] == p:
            own[s] = own.get(s, 0) + 1
    f["claimant_touches"] = sorted(set(own.values()))
    total = {}
    for p, i, b, s, what in ref.touches:
        total[s] = total.get(s, 0) + 1
    f["touched_once"] = sorted(s for s, n in total.items() if n == 1)
    prods = [i * b for _, i, b, _, _ in ref.touches]
    f["products_past_2_31"] = sum(1 for v in set(prods) if (1 << 31) <= v < (1 << 32))
    f["products_past_2_32"] = sum(1 for v in set(prods) if v >= (1 << 32))
    ys, xs = np.nonzero(r.ids > 0)
    f["rows"] = (int(ys.min()), int(ys.max())) if len(ys) else None
    f["cols"] = (int(xs.min()), int(xs.max())) if len(xs) else None
    f["clipped_windows"] = int(np.count_nonzero((ys < 3) | (ys > ih - 4) | (xs < 3) | (xs > iw - 4))) if len(ys) else 0
    f["live"], f["records"], f["invalid_records"] = r.live_count, int(r.segs.view("i4")[0]), int(np.count_nonzero(r.segs[1:]["polyid"] == 0))
    f["nonpositive_cells"] = sorted({int(v) for v in np.unique(r.boundary) if v <= 0})
    n = f["records"]
    probes, kinds = expected_probes(r, ref.table, n + 1, (n + 1) * LIM["PROBE_INTS"])
    f["probe_kinds"] = sorted(set(kinds))
    f["probe_nonpositive"] = sorted({int(v) for v in probes[LIM["PROBE_INTS"]::6] if v <= 0})
    return f


# ---- what the sampling kernel must write, from the list, the plane and a table
def expected_probes(r, table, max_records, probes_ints):
    """the probes buffer: RD_PROBE_INTS ints for every record 1 .. min(n, max_records - 1), everything else the guard word; also what each probe is
    ('outside', 'nonpositive', 'owned', 'other', 'unclaimed', 'invalid record') for the claims"""
    ih, iw = r.ids.shape
    out = np.full(probes_ints, GUARD, np.int32)
    kinds = []
    segs, n = r.segs, int(r.segs.view("i4")[0])
    for i in range(1, min(n, max_records - 1) + 1):
        px = probe_pixels(segs["x0"][i], segs["y0"][i], segs["x1"][i], segs["y1"][i], iw, ih) if segs["polyid"][i] != 0 else None
        for k in range(15):
            v = [0] * 6
            if px is None:
                kinds.append("invalid record")
            elif px[k][0] < 0:
                kinds.append("outside")
            else:
                v[0] = int(r.boundary[px[k][1], px[k][0]])
                if v[0] <= 0:
                    kinds.append("nonpositive")
                else:
                    e = table[slot_of(i, v[0], r.nentry)]
                    v[1:] = [int(w) for w in e]
                    kinds.append("unclaimed" if e[0] == 0 else "owned" if e[0] == i else "other")
            out[(i * 15 + k) * 6: (i * 15 + k) * 6 + 6] = v
    return out, kinds


def expected_pack(list_ints, ctr, rflags, probes, max_records, pack_records, pack_ints):
    """the hand-over block from the list as the device left it, the counters, the flags and the probes buffer: counters, region flags, status words, the header
    record, records 1 .. min(n, max_records - 1, pack_records - 1) and their probes; everything else the guard word"""
    L = LIM
    out = np.full(pack_ints, GUARD, np.int32)
    out[: L["PACK_FLAGS"]] = ctr[: L["PACK_FLAGS"]]
    out[L["PACK_FLAGS"]: L["PACK_FLAGS"] + L["PACK_FLAGS_INTS"]] = rflags[: L["PACK_FLAGS_INTS"]]
    out[L["PACK_STATUS"]: L["PACK_STATUS"] + L["PACK_STATUS_INTS"]] = rflags[L["RFLAGS_STATUS_AT"]: L["RFLAGS_STATUS_AT"] + L["PACK_STATUS_INTS"]]
    R, RI, PI = L["PACK_RECORDS"], L["REC_INTS"], L["PROBE_INTS"]
    n = int(list_ints[0])
    out[R: R + RI] = list_ints[:RI]
    for i in range(1, min(n, max_records - 1, pack_records - 1) + 1):
        out[R + i * RI: R + (i + 1) * RI] = list_ints[i * RI: (i + 1) * RI]
        at = R + pack_records * RI + i * PI
        out[at: at + PI] = probes[i * PI: (i + 1) * PI]
    return out


def rflags_pattern(frames):
    """(frames, 256) ints, every word different and none a guard word"""
    return (0x01000000 + 0x10000 * np.arange(frames)[:, None] + np.arange(ra.VOTES_RFLAGS_INTS)[None, :]).astype(np.int32)


# ---- masks and painters
def lines_mask(size, rows, x0=8, x1=88):
    """horizontal lines: pixels x0 .. x1 - 1 of each row.  The stage numbers a line from its left end, which belongs to no segment: line k (from the top) is segment
    k + 1 on the pixels x0 + 1 .. x1 - 1"""
    iw, ih = size
    m = np.zeros((ih, iw), np.int32)
    for y in rows:
        m[y, x0:x1] = 1
    return m


def cross_mask():
    """a vertical line (column 80, rows 5 .. 59: segment 1 on rows 6 .. 59, its first pixel is the first in raster order) and a horizontal one (row 30, columns
    8 .. 60: segment 2 on columns 9 .. 60)"""
    m = np.zeros((SMALL[1], SMALL[0]), np.int32)
    m[5:60, 80] = 1
    m[30, 8:61] = 1
    return m


def blank(r, fill=0):
    return np.full(r.ids.shape, fill, np.int32)


def window_cells(y, x):
    return [(y + dy, x + dx) for dy in range(-3, 4) for dx in range(-3, 4)]


def paint_distinct(k):
    """the window of the chain pixel (16, 48) holds exactly k distinct ids (cells beyond the k-th: 0 and -1 in turn); its neighbours' windows hold fewer"""
    def paint(r):
        b = blank(r)
        for j, (y, x) in enumerate(window_cells(16, 48)):
            b[y, x] = 1000 + 37 * j if j < k else -(j & 1)
        return b
    return paint


def paint_distinct_end(r):
    """RB_MAX + 1 ids in the window of line 1's last pixel, (16, 87), the largest of them in column 90, which no other window reaches: that slot's id is there
    only if the pixel's second pass of ids casts its votes as the first does"""
    b = blank(r)
    for j in range(RB_MAX):
        b[13 + j // 4, 85 + j % 4] = 300 + 11 * j
    b[16, 90] = 5000
    return b


def paint_unique(r):
    """b = 1 + p: every cell its own id"""
    return (1 + np.arange(r.ids.size, dtype=np.int32)).reshape(r.ids.shape)


def paint_sparse(r):
    b = blank(r, -1)
    b[18, 10:300:9] = 5
    b[22, 20:300:31] = 6
    b[38, 4:316] = 7
    return b


def paint_window_pair(extra):
    """the last pixel of line 1, (16, 87), is the only pixel whose window reaches column 90.  Two ids there that segment 1 maps to one slot (b and b + nentry: the
    product stays below 2^31), in 1 + 1 cells (extra = 0) or 1 + 2 (extra = 1): the pixel's second touch widens although no id of its window occurs twice (1 + 1).
    Line 2's last pixel (40, 87) meets one id in one cell: a slot claimed and never widened."""
    def paint(r):
        b = blank(r)
        b[14, 90], b[17, 90] = 11, 11 + r_nentry(r)
        if extra:
            b[19, 90] = 11 + r_nentry(r)
        b[40, 90] = 13
        return b
    return paint


def r_nentry(r):
    return nentry_of(r.ids.shape[1], r.ids.shape[0])


def paint_two_segments(r):
    """cross_mask.  Slot 14 = 1 * 14 = 2 * 7: segment 1 meets 14 near its top (rows 6 .. 11, before every pixel of row 30), segment 2 meets 7: the smaller id owns, 2's
    votes are dropped.  Slot 22 = 1 * 22 = 2 * 11: segment 1 meets 22 near its bottom (rows 52 .. 58), after segment 2 met 11 in row 30: the larger id owns."""
    b = blank(r, -1)
    b[8, 83], b[32, 20] = 14, 7
    b[55, 83], b[28, 40] = 22, 11
    return b


def paint_ids_apart(r):
    """segment 1 meets b around column 20 and b + nentry around column 60: one slot, claimed at column 17, widened up to column 63"""
    b = blank(r)
    b[14, 20], b[18, 60] = 9, 9 + r_nentry(r)
    return b


TOUCH_COLUMNS = {1: 30, 2: 40, 3: 50, 4: 60, 7: 70}


def paint_touches(r):
    """line 1 (row 16, ids on columns 9 .. 87).  A column c of the plane enters the windows with pixel c - 3, which therefore claims what it finds there: an id in
    n cells of column c is touched n times by its claimant (n = 1: the claimant does not widen, the box starts at column c - 2).  The line's first pixel (16, 9)
    sees its whole window at once: 49 cells of one id.  Line 2's first pixel (40, 9): 8 cells of one id; its last pixel: one cell, touched once by nobody else."""
    b = blank(r)
    for n, c in TOUCH_COLUMNS.items():
        b[13:13 + n, c] = 100 + n
    for y, x in window_cells(16, 9):
        b[y, x] = 149
    for y, x in window_cells(40, 9)[:8]:
        b[y, x] = 108
    b[40, 90] = 13
    return b


WRAP_IDS = (0x7fffffff, 0x7ffffffe, 0x40000001, 0x55555555, 0x7fff0001, 0x12345679)


def paint_wrap(r):
    """four lines, segments 1 .. 4: the products of 2, 3, 4 and ids near 2^31 pass 2^31 and 2^32"""
    b = blank(r)
    for row in (10, 22, 34, 46):
        for j, v in enumerate(WRAP_IDS):
            b[row - 2 + j % 3, 14 + 7 * j] = v
    return b


def edge_mask(ring):
    """lines along all four sides, as near the frame as the stage keeps a chain: rows 2 / 3 and ih - 3 / ih - 4, columns 2 / 3 and iw - 3 / iw - 4 (ring 0 / 1)"""
    iw, ih = SMALL
    d = 2 + ring
    m = np.zeros((ih, iw), np.int32)
    m[d, 10:86] = 1
    m[ih - 1 - d, 10:86] = 1
    m[10:54, d] = 1
    m[10:54, iw - 1 - d] = 1
    return m


def paint_edges(r):
    """an id of its own on every pixel of the seven outermost rows and columns: the whole window of a pixel in row 3 (49 cells), the clipped one of a pixel in
    row 2 (42 cells)"""
    b = blank(r)
    u = paint_unique(r)
    for sl in (np.s_[:7, :], np.s_[-7:, :], np.s_[:, :7], np.s_[:, -7:]):
        b[sl] = u[sl]
    return b


def paint_nonpositive(r):
    """0, -1, INT_MIN and a few ids mixed cell by cell"""
    ih, iw = r.ids.shape
    y, x = np.mgrid[:ih, :iw]
    k = (x + 3 * y) % 5
    ids = 1 + (x // 5 + 7 * (y // 5)) % 9
    return np.select([k == 0, k == 1, k == 2], [0, -1, -0x80000000], ids).astype(np.int32)


def short_mask():
    """one line of six pixels: no chain longer than size_thre, nothing for the votes to do"""
    m = np.zeros((SMALL[1], SMALL[0]), np.int32)
    m[20, 30:36] = 1
    return m


def sampling_mask():
    """two long lines, a line of two pixels (with size_thre 0 a chain of one pixel: its record is invalid, polyid 0), three vees, and a spike under the top edge: two
    columns of six pixels two apart, joined by one pixel in row 2.  Its two records are nearly parallel; the join moves their common end point to where their lines
    cross, several pixels above the frame, and most of their probes with it"""
    iw, ih = SMALL
    m = np.zeros((ih, iw), np.int32)
    m[50, 8:60] = 1
    m[58, 8:60] = 1
    m[40, 70:72] = 1
    for k in range(3):
        for i in range(-8, 9):
            m[22 + 8 - abs(i), 14 + 24 * k + i] = 1
    m[3:9, 83] = 1
    m[2, 84] = 1
    m[3:9, 85] = 1
    return m


def paint_sampling(r):
    """ids under probes of every kind: for each valid record, its probes 0, 1, 2 get -1, 0 and an id the record's own pixels vote for; line 2's middle probe gets an
    id whose slot line 1's segment claims first (line 1 lies above: b_other)"""
    ih, iw = r.ids.shape
    b = blank(r)
    segs, n = r.segs, int(r.segs.view("i4")[0])
    for i in range(1, n + 1):
        if segs["polyid"][i] == 0:
            continue
        px = probe_pixels(segs["x0"][i], segs["y0"][i], segs["x1"][i], segs["y1"][i], iw, ih)
        for k, v in ((5, -1), (6, 0), (7, 500 + i), (12, 700 + i)):
            if px[k][0] >= 0:
                b[px[k][1], px[k][0]] = v
    # the two long lines: the upper one's id u, the lower one's l (from the id plane); slot of (l, u * 3) = slot of (u, l * 3), which u's pixels claim first
    u, l = int(r.ids[50, 30]), int(r.ids[58, 30])
    px = probe_pixels(segs["x0"][l], segs["y0"][l], segs["x1"][l], segs["y1"][l], iw, ih)
    b[px[2][1], px[2][0]] = u * 3
    b[48, 12] = l * 3
    return b


# ---- the cases
def all_cases():
    two = lambda: lines_mask(SMALL, (16, 40))
    out = []
    for k in (RB_MAX, RB_MAX + 1, 2 * RB_MAX, 2 * RB_MAX + 1, 49):
        out.append(Case("distinct_%d" % k, SMALL, two, paint_distinct(k), claims=dict(max_distinct=k)))
    out.append(Case("distinct_%d_end" % (RB_MAX + 1), SMALL, two, paint_distinct_end, claims=dict(max_distinct=RB_MAX + 1, touched_once=1)))
    out.append(Case("hash_full", WIDE, lambda: lines_mask(WIDE, (20, 40), 5, 315), paint_unique,
                    claims=dict(hash_full=dict(touched=[1834, 1818], slots=4224, zero_box_slots=27), max_distinct=49)))
    out.append(Case("wide_sparse", WIDE, lambda: lines_mask(WIDE, (20, 40), 5, 315), paint_sparse, claims=dict(slots=3)))
    out.append(Case("window_pair_1p1", SMALL, two, paint_window_pair(0), claims=dict(same_window=1, claimant_touches=[1, 2], touched_once=1)))
    out.append(Case("window_pair_1p2", SMALL, two, paint_window_pair(1), claims=dict(same_window=1, claimant_touches=[1, 3], touched_once=1)))
    out.append(Case("two_segments", SMALL, cross_mask, paint_two_segments, claims=dict(two_segments={14: (1, [2]), 22: (2, [1])})))
    out.append(Case("ids_apart", SMALL, two, paint_ids_apart, claims=dict(two_ids_apart=1)))
    out.append(Case("touches", SMALL, two, paint_touches, claims=dict(claimant_touches=[1, 2, 3, 4, 7, 8, 49], touched_once=1)))
    out.append(Case("wrap", SMALL, lambda: lines_mask(SMALL, (10, 22, 34, 46), 8, 60), paint_wrap, claims=dict(wrap=True)))
    out.append(Case("edge_ring0", SMALL, lambda: edge_mask(0), paint_edges, ring=0, claims=dict(rows=(2, SMALL[1] - 3), cols=(2, SMALL[0] - 3), clipped=True, max_distinct=42)))
    out.append(Case("edge_ring1", SMALL, lambda: edge_mask(1), paint_edges, ring=1, claims=dict(rows=(3, SMALL[1] - 4), cols=(3, SMALL[0] - 4), clipped=False, max_distinct=49)))
    out.append(Case("nonpositive", SMALL, two, paint_nonpositive, claims=dict(nonpositive=[-0x80000000, -1, 0])))
    out.append(Case("empty", SMALL, short_mask, paint_unique, claims=dict(live=0, slots=0)))
    out.append(Case("sampling", SMALL, sampling_mask, paint_sampling, minerror=4.0, size_thre=0, claims=dict(sampling=True)))
    return out


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}
# frames of one launch share the stage's parameters: the cases a group is made of
GROUP = [c for c in CASES if c.params() == (SMALL, 0, 1.0, 10)]
