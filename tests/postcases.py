"""Crafted inputs of the post-process (line segments + boundary plane + vote table -> rectangles), one per path and capacity edge of the device
post-process.  Written from the reference's executeCPUTask (oclrect.c:1049-1226) as SURVEY.md and DESIGN.md describe it and from the layouts in
include/: a case is what the reference's host side reads back from the device - the linesegment_t list, the boundary-component plane, reduceLS's
vote table - and nothing else.

How the three fit together (oclrect.c:1066-1131):
  * every record with polyid != 0 has 15 probes (3 points along the segment x 5 offsets along its normal; rd_probe_pixels gives the pixels); the boundary
    ids > 0 under them are the components the segment is a MEMBER of (once per component, however many probes hit it);
  * a component with at least four members is a candidate.  For each member the vote-table slot ((i * b) & 0x7fffffff) % nentry of (segment i, id b) says
    what becomes of it: owner == i -> the segment clipped to the slot's box {iw - xmin, xmax, ih - ymin, ymax} (or nothing when the box rejects it),
    owner another segment -> the whole segment, owner 0 -> nothing;
  * every record with polyid != 0 and leftPtr <= 0 heads a polyline (rightPtr links): its segments longer than 32 are a candidate as well (status bit 2);
  * candidates come in the order (components in the iteration order of the reference's hash map, then polyline heads by index).

Every case is a function of a seed and of the device's limits (rectdetect_amd.post_device_limits(): the tests hard-code none of them).  The capacity cases
take `over`: False sits exactly on the limit, True is one past it."""
import numpy as np

import rectdetect_amd as ra
from rectdetect_amd import LS_DTYPE

TAN36 = float(np.tan(np.pi / 5))
TAN25 = float(np.tan(25.0 / 180.0 * np.pi))


class Case:
    def __init__(self, name, segs, boundary, table, iw, ih, tan_aov, **meta):
        self.name, self.segs, self.boundary, self.table, self.iw, self.ih, self.tan_aov, self.meta = name, segs, boundary, table, iw, ih, tan_aov, meta
        self._members = None

    def planes(self):
        return self.segs, self.boundary, self.table, self.iw, self.ih


def probe_pixels(x0, y0, x1, y1, iw, ih):
    """the 15 probe pixels (x, y) of a segment; (-1, -1): outside the frame"""
    out = np.zeros(30, np.int32)
    ra.lib().rd_probe_pixels(float(x0), float(y0), float(x1), float(y1), iw, ih, out.ctypes.data)
    return out.reshape(15, 2)


def slot_of(i, b, nentry):
    return (((i * b) & 0xFFFFFFFF) & 0x7FFFFFFF) % nentry


def memberships(case):
    """{component id: sorted member segments} as oclrect.c:1066-1098 collects them, in order of first insertion"""
    if case._members is not None:
        return case._members
    segs = case.segs
    n = int(segs.view("i4")[0])
    groups = case._members = {}
    for i in range(1, n + 1):
        if segs["polyid"][i] == 0:
            continue
        px = probe_pixels(segs["x0"][i], segs["y0"][i], segs["x1"][i], segs["y1"][i], case.iw, case.ih)
        for x, y in px:
            if x < 0:
                continue
            b = int(case.boundary[y, x])
            if b > 0:
                m = groups.setdefault(b, [])
                if i not in m:
                    m.append(i)
    return groups


def chain_heads(case):
    segs = case.segs
    n = int(segs.view("i4")[0])
    v = segs[1:n + 1]
    return [int(i) + 1 for i in np.nonzero((v["polyid"] != 0) & (v["leftPtr"] <= 0))[0]]


def candidate_count(case):
    """components with at least four distinct member segments + polyline heads: what the device counts in info[0]"""
    return sum(1 for m in memberships(case).values() if len(m) >= 4) + len(chain_heads(case))


def am_bucket(k):
    """bucket of a key in the reference's ArrayMap (helper.c:127-134), whose iteration order is (bucket, order of insertion)"""
    return (k ^ (k >> 10) ^ (k >> 20) ^ (k >> 30)) & 1023


class _Builder:
    def __init__(self, iw=640, ih=480):
        self.iw, self.ih, self.nentry = iw, ih, iw * ih * 4 // 5
        self.rows = [np.zeros((), LS_DTYPE)]
        self.boundary = np.zeros((ih, iw), np.int32)
        self.table = np.zeros((self.nentry, 5), np.int32)
        self.voted = {}          # slot -> (i, b)
        self.collision_ok = False

    def seg(self, x0, y0, x1, y1, polyid=1, left=0, right=0):
        r = np.zeros((), LS_DTYPE)
        r["x0"], r["y0"], r["x1"], r["y1"], r["polyid"], r["leftPtr"], r["rightPtr"] = x0, y0, x1, y1, polyid, left, right
        self.rows.append(r)
        return len(self.rows) - 1

    def pixels(self, i):
        r = self.rows[i]
        return probe_pixels(r["x0"], r["y0"], r["x1"], r["y1"], self.iw, self.ih)

    def paint(self, i, b, ks=range(15)):
        px = self.pixels(i)
        for k in ks:
            x, y = px[k]
            if x < 0:
                continue
            assert self.boundary[y, x] in (0, b), ("probe pixel already belongs to another component", i, k, int(self.boundary[y, x]), b)
            self.boundary[y, x] = b

    def vote(self, i, b, owner, box=(0, 0, 0, 0)):
        """box = (xmin, ymin, xmax, ymax) in pixels"""
        s = slot_of(i, b, self.nentry)
        assert self.collision_ok or self.voted.get(s, (i, b)) == (i, b), ("vote-table collision", (i, b), self.voted[s])
        self.voted[s] = (i, b)
        self.table[s] = (owner, self.iw - box[0], box[2], self.ih - box[1], box[3])

    def vote_self(self, i, b, margin=2):
        r = self.rows[i]
        xs, ys = (float(r["x0"]), float(r["x1"])), (float(r["y0"]), float(r["y1"]))
        self.vote(i, b, i, (int(np.floor(min(xs))) - margin, int(np.floor(min(ys))) - margin, int(np.ceil(max(xs))) + margin, int(np.ceil(max(ys))) + margin))

    def quad(self, corners, b, head=True, flips=(0, 0, 0, 0)):
        """four sides of one component, each its own slot owner with a box that contains it (the clip path, nothing clipped)"""
        ids = []
        for s in range(4):
            p, q = corners[s], corners[(s + 1) % 4]
            if flips[s]:
                p, q = q, p
            i = self.seg(p[0], p[1], q[0], q[1], left=0 if head else 1)
            self.paint(i, b)
            self.vote_self(i, b)
            ids.append(i)
        return ids

    def tiny(self, col, row, **kw):
        """a horizontal segment of length 6 whose 15 probes are the pixels (8 col + {1, 3, 5}, 6 row + {0..4}): cells of 8 x 6 never share a probe pixel"""
        x, y = 8 * col, 6 * row + 2
        return self.seg(x, y, x + 6, y, **kw)

    def finish(self, name, tan_aov=TAN36, **meta):
        segs = np.zeros(len(self.rows), LS_DTYPE)
        for i, r in enumerate(self.rows):
            segs[i] = r
        segs.view("i4")[0] = len(self.rows) - 1
        case = Case(name, segs, self.boundary, self.table, self.iw, self.ih, tan_aov, **meta)
        if not self.collision_ok:
            # no slot the post-process reads - that of a (member, candidate component) - holds the entry of another pair
            for b, members in memberships(case).items():
                if len(members) < 4:
                    continue
                for i in members:
                    s = slot_of(i, b, self.nentry)
                    assert self.voted.get(s, (i, b)) == (i, b), ("vote-table collision", name, (i, b), self.voted[s])
        return case


def _cells(x0, y0, x1, y1, nx, ny):
    w, h = (x1 - x0) / nx, (y1 - y0) / ny
    return [(x0 + (c + 0.5) * w, y0 + (r + 0.5) * h, min(w, h) / 2 - 6) for r in range(ny) for c in range(nx)]


def _convex_quad(rng, cx, cy, r, rmin=0.75, jitter=25.0):
    base = rng.uniform(0, 360)
    pts = []
    for k in range(4):
        a = np.deg2rad(base + 90 * k + rng.uniform(-jitter, jitter))
        rr = r * rng.uniform(rmin, 1.0)
        pts.append((np.float32(cx + rr * np.cos(a)), np.float32(cy + rr * np.sin(a))))
    return pts


def _ordinary_quads(B, rng, cells, first_id, head=True):
    """one convex quad per cell, ids first_id, first_id + 2, ...: the 'ordinary quads' the capacity cases stand among"""
    ids = []
    for q, (cx, cy, r) in enumerate(cells):
        ids.append(first_id + 2 * q)
        B.quad(_convex_quad(rng, cx, cy, r), ids[-1], head=head, flips=rng.integers(0, 2, 4))
    return ids


# ---------------------------------------------------------------------------------------------------------------- values and order
def quads(seed, lim):
    """24 convex quads at random poses, four segments each, one component per quad"""
    rng = np.random.default_rng(seed)
    B = _Builder()
    _ordinary_quads(B, rng, _cells(0, 0, 640, 480, 6, 4), 1009)
    return B.finish("quads", min_valid=24)


def axis_aligned(seed, lim):
    """16 upright rectangles with integer corners, every pattern of end-point orders of the four sides: the outward normals have a component that is
    exactly 0 or -0, atan2 in the angular sort sits at 0, +-pi/2, +-pi"""
    rng = np.random.default_rng(seed)
    B = _Builder()
    for q, (cx, cy, _) in enumerate(_cells(0, 0, 640, 480, 4, 4)):
        w, h = int(rng.integers(25, 60)), int(rng.integers(20, 45))
        x0, y0 = int(cx) - w, int(cy) - h
        x1, y1 = int(cx) + w, int(cy) + h
        B.quad([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], 2003 + 2 * q, flips=[(q >> s) & 1 for s in range(4)])
    return B.finish("axis_aligned", min_valid=8)


def near_parallel(seed, lim):
    """ties in the angular sort: quads with a fifth and sixth segment collinear with a side (direction vectors exact multiples of (4, 3)), and trapezoids
    whose parallel sides are (60, 80) and (30, 40) long - normals exact multiples of each other - in both end-point orders"""
    rng = np.random.default_rng(seed)
    B = _Builder()
    cells = _cells(0, 0, 640, 480, 3, 2)
    for q in range(3):
        cx, cy, _ = cells[q]
        a = (int(cx) - 20 + int(rng.integers(-8, 9)), int(cy) - 70 + int(rng.integers(-8, 9)))
        m, b = (a[0] + 40, a[1] + 30), (a[0] + 80, a[1] + 60)
        c = (b[0] - 45 + int(rng.integers(-4, 5)), b[1] + 60 + int(rng.integers(-4, 5)))
        d = (a[0] - 45 + int(rng.integers(-4, 5)), a[1] + 60 + int(rng.integers(-4, 5)))
        cid = 3001 + 2 * q
        B.quad([a, b, c, d], cid, flips=rng.integers(0, 2, 4))
        for p, r in ((a, m), (m, b)) if q != 1 else ((m, a), (b, m)):
            i = B.seg(p[0], p[1], r[0], r[1])
            B.paint(i, cid)
            B.vote_self(i, cid)
    for q in range(3):
        cx, cy, _ = cells[3 + q]
        p0 = (int(cx) - 10 + int(rng.integers(-8, 9)), int(cy) - 50 + int(rng.integers(-8, 9)))
        p1 = (p0[0] + 60, p0[1] + 80)
        p2 = (p1[0] - 70 + int(rng.integers(-3, 4)), p1[1] + 10)
        p3 = (p2[0] - 30, p2[1] - 40)
        B.quad([p0, p1, p2, p3], 3011 + 2 * q, flips=(0, 0, q & 1, 0))
    return B.finish("near_parallel", min_valid=6)


def branches(seed, lim):
    """one component whose members are in every state: clipped by their own box on one, two and three sides, rejected by it, taken whole (the slot belongs
    to another segment), dropped (empty slot); hit by 1, 7 and 15 of their probes; and a segment whose probes hit three components"""
    rng = np.random.default_rng(seed)
    B = _Builder()
    j = [int(v) for v in rng.integers(-6, 7, 8)]
    P = [(150 + j[0], 120 + j[1]), (500 + j[2], 100 + j[3]), (520 + j[4], 380 + j[5]), (130 + j[6], 360 + j[7])]
    cb, cc, cd = 7001, 7013, 7019

    def along(p, q, before, after):
        d = np.array(q, float) - np.array(p, float)
        u = d / np.hypot(*d)
        return tuple(np.array(p, float) - before * u), tuple(np.array(q, float) + after * u)

    # side 0: longer than the quad's side at both ends, its box cuts it left and right (two sides)
    e0, e1 = along(P[0], P[1], 40, 30)
    s0 = B.seg(e0[0], e0[1], e1[0], e1[1])
    B.paint(s0, cb)
    B.vote(s0, cb, s0, (P[0][0], 0, P[1][0], 479))
    # side 1: longer at its lower end, cut there (one side); its probes hit three components, five each
    e0, e1 = along(P[1], P[2], 0, 50)
    s1 = B.seg(e0[0], e0[1], e1[0], e1[1])
    B.paint(s1, cb, range(0, 5))
    B.paint(s1, cc, range(5, 10))
    B.paint(s1, cd, range(10, 15))
    B.vote(s1, cb, s1, (0, 0, 639, P[2][1]))
    # side 2: from beyond the lower right corner (outside the box in x and in y: two cuts at that end) to beyond the lower left one (a third cut)
    e0, e1 = along(P[2], P[3], 60, 40)
    s2 = B.seg(e0[0], e0[1], e1[0], e1[1])
    B.paint(s2, cb)
    B.vote(s2, cb, s2, (P[3][0], 0, P[2][0] - 5, P[2][1]))
    # side 3: the slot belongs to side 0 - taken whole; 7 of its probes hit the component
    s3 = B.seg(P[3][0], P[3][1], P[0][0], P[0][1])
    B.paint(s3, cb, range(0, 14, 2))
    B.vote(s3, cb, s0, (1, 2, 3, 4))
    # outside the quad on the right: its own box rejects it
    r = B.seg(570, 200, 610, 260)
    B.paint(r, cb)
    B.vote(r, cb, r, (20, 20, 60, 60))
    # outside the quad on the left: empty slot, dropped
    d = B.seg(40, 200, 80, 260)
    B.paint(d, cb)
    # inside the quad: one probe hits, taken whole
    o = B.seg(300, 220, 360, 240)
    B.paint(o, cb, [7])
    B.vote(o, cb, s1, (0, 0, 0, 0))
    return B.finish("branches", min_valid=1)


def threshold(seed, lim):
    """components with exactly 3 and exactly 4 member segments, records with polyid == 0 under whose probes a component lies, probe values 0 and -1"""
    rng = np.random.default_rng(seed)
    B = _Builder()
    cells = _cells(0, 0, 640, 480, 4, 3)
    four, three = [], []
    for q, (cx, cy, r) in enumerate(cells):
        cid = 4001 + 2 * q
        c = _convex_quad(rng, cx, cy, r)
        kind = q % 4
        if kind == 0:          # exactly four members; five probes of a side see -1, five see 0
            ids = B.quad(c, cid)
            px = B.pixels(ids[0])
            for k in range(10):
                B.boundary[px[k][1], px[k][0]] = -1 if k < 5 else 0
            for k in range(10, 15):      # (a corner's pixels may be shared with the next side: painted again)
                B.boundary[px[k][1], px[k][0]] = cid
            four.append(cid)
        elif kind == 1:        # four records, one of them with polyid == 0: three members
            ids = B.quad(c, cid)
            B.rows[ids[2]]["polyid"] = 0
            three.append(cid)
        elif kind == 2:        # five records, one of them (a diagonal) with polyid == 0: four members
            B.quad(c, cid)
            i = B.seg(c[0][0], c[0][1], c[2][0], c[2][1], polyid=0)
            px = B.pixels(i)
            for k in range(5, 10):
                B.boundary[px[k][1], px[k][0]] = cid
            four.append(cid)
        else:                  # three sides only: three members
            for s in range(3):
                i = B.seg(c[s][0], c[s][1], c[s + 1][0], c[s + 1][1])
                B.paint(i, cid)
                B.vote_self(i, cid)
            three.append(cid)
    case = B.finish("threshold", min_valid=6, four=four, three=three)
    m = memberships(case)
    assert all(len(m[c]) == 4 for c in four) and all(len(m[c]) == 3 for c in three), {c: len(v) for c, v in m.items()}
    return case


def bucket_order(seed, lim):
    """48 quads on a 1920x1080 plane whose component ids share buckets of the reference's hash map, differ only in bits 10-19 or only from bit 20 up: the
    list comes in (bucket, first insertion) order, which is neither the order of the ids nor the order of the segments"""
    rng = np.random.default_rng(seed)
    B = _Builder(1920, 1080)
    cells = _cells(0, 0, 1920, 1080, 8, 6)
    ids = [5, 4 | (1 << 10), 5 | (3 << 10) | (3 << 20), 1 | (4 << 20), 5 << 10, 5 << 20,                 # bucket 5, reached through every term
           7 | (1 << 10), 7 | (2 << 10), 7 | (3 << 10), 7 | (1 << 10) | (1 << 20),                       # differ only in bits 10-19 (and one in bit 20)
           9 | (1 << 20), 9 | (2 << 20), 9 | (5 << 20), 9 | (300 << 20),                                 # differ only from bit 20 up
           1023, 1023 | (1023 << 10), 1023 | (1023 << 20), 512, 512 | (512 << 10) | (1 << 20)]
    k = 11
    while len(ids) < len(cells):
        k += 37
        v = (k * 2654435761) & 0x3FFFFFFF
        v = v if len(ids) % 3 else v & 0xFFFFF
        if v > 0 and v not in ids:
            ids.append(v)
    ids = [int(v) for v in rng.permutation(np.array(ids, np.int64))]
    assert len(set(ids)) == len(ids) and min(ids) > 0
    for (cx, cy, r), cid in zip(cells, ids):
        B.quad(_convex_quad(rng, cx, cy, r), cid, head=False, flips=rng.integers(0, 2, 4))
    return B.finish("bucket_order", min_valid=40, ids=ids, cells=cells)


def chains(seed, lim):
    """polylines of 1, 4, 5 and 40 segments linked through leftPtr / rightPtr: heads with leftPtr 0 and < 0, segments of squared length exactly 1024 (left
    out) and just above (taken), a polyline whose last rightPtr points past the list.  No components: the boundary plane is empty."""
    rng = np.random.default_rng(seed)
    B = _Builder()
    ABOVE = -1.0      # a piece just longer than 32: it ends on the float after start + 32

    def end_of(start, length):
        return float(np.nextafter(np.float32(start + 32), np.float32(1e9))) if length == ABOVE else start + length

    def link(ids, head_left=0, tail_right=0):
        for k, i in enumerate(ids):
            B.rows[i]["leftPtr"] = ids[k - 1] if k else head_left
            B.rows[i]["rightPtr"] = ids[k + 1] if k + 1 < len(ids) else tail_right

    cells = _cells(0, 0, 640, 210, 7, 1)
    tails = []
    for q, (cx, cy, r) in enumerate(cells):
        c = _convex_quad(rng, cx, cy, r + 6, rmin=0.9, jitter=12.0)
        ids = [B.seg(c[s][0], c[s][1], c[(s + 1) % 4][0], c[(s + 1) % 4][1]) for s in range(4)]
        if q % 2:      # five segments: one of squared length exactly 1024 (q = 1, 5) or just above (q = 3) inside the quad
            ids.insert(2, B.seg(int(cx) - 16, int(cy), end_of(int(cx) - 16, ABOVE if q == 3 else 32.0), int(cy)))
        link(ids, head_left=-3 if q % 3 == 0 else 0)
        tails.append(ids[-1])
    B.seg(20, 215, 90, 222)                                     # a polyline of one segment
    B.seg(100, 215, 132, 215, left=-1)                          # one of one segment of squared length exactly 1024
    # 40 segments: a quad of four long sides, each followed by nine short pieces on the same line (two of them just above 32, the others at or below)
    x0, y0, x1, y1 = 60, 240, 580, 460
    ids = []
    for (ax, ay), (bx, by) in (((x0, y0), (x1, y0)), ((x1, y0), (x1, y1)), ((x1, y1), (x0, y1)), ((x0, y1), (x0, y0))):
        ux, uy = np.sign(bx - ax), np.sign(by - ay)
        full = abs(bx - ax) + abs(by - ay)
        pieces = [32.0, ABOVE, 8.0, 8.0, 32.0, 5.0, 8.0, 3.0, 8.0] if len(ids) in (0, 20) else [8.0] * 9
        at = full - sum(32.0 if p == ABOVE else p for p in pieces) - 1
        ids.append(B.seg(ax, ay, ax + ux * at, ay + uy * at))
        for p in pieces:
            nxt = end_of(at, p)
            ids.append(B.seg(ax + ux * at, ay + uy * at, ax + ux * nxt, ay + uy * nxt))
            at = nxt
    assert len(ids) == 40
    link(ids)
    n = len(B.rows) - 1
    B.rows[tails[0]]["rightPtr"] = n + 7                        # leaves 1..n: the walk ends there
    case = B.finish("chains", min_valid=6, min_status2=6)
    v = case.segs[1:]
    d2 = (v["x0"].astype("f8") - v["x1"]) ** 2 + (v["y0"].astype("f8") - v["y1"]) ** 2
    assert (d2 == 1024).sum() >= 4 and ((d2 > 1024) & (d2 < 1024.01)).sum() >= 3
    return case


# ---------------------------------------------------------------------------------------------------------------- capacity
TOP = (0, 0, 640, 112)          # where the ten ordinary quads of the capacity cases stand; tiny segments start at row 20 (y = 120)
ROW0 = 20


def _ten_quads(B, rng, head=True):
    return _ordinary_quads(B, rng, _cells(*TOP, 10, 1), 1009, head=head)


def _tiny_cells():
    return [(c, r) for r in range(ROW0, 80) for c in range(80)]


def cap_members_per_candidate(seed, lim, over=False):
    """one component with exactly POST_CAP members (over: one more), every one of them taken, among ten ordinary quads"""
    rng = np.random.default_rng(seed)
    B = _Builder()
    _ten_quads(B, rng)
    cid = 9001
    sides = B.quad([(40, 140), (600, 150), (590, 460), (50, 450)], cid)
    inner = [(c, r) for c, r in _tiny_cells() if 13 <= c <= 67 and 34 <= r <= 66]
    for c, r in inner[: lim["POST_CAP"] - 4 + (1 if over else 0)]:
        i = B.tiny(c, r)
        B.paint(i, cid, [int(rng.integers(0, 15))])
        B.vote(i, cid, sides[0])                                 # another segment's slot: taken whole
    case = B.finish("cap_members_per_candidate", min_valid=0)
    assert len(memberships(case)[cid]) == lim["POST_CAP"] + (1 if over else 0)
    return case


def maxc_chains(seed, lim, over=False):
    """exactly POST_MAXC polyline heads of one segment each (over: one more) and no component"""
    B = _Builder()
    for c, r in _tiny_cells()[: lim["POST_MAXC"] + (1 if over else 0)]:
        B.tiny(c, r)
    return B.finish("maxc_chains", min_valid=0)


def maxc_mixed(seed, lim, over=False):
    """ten components plus POST_MAXC - 10 polyline heads (over: one more head)"""
    rng = np.random.default_rng(seed)
    B = _Builder()
    _ten_quads(B, rng, head=False)
    for c, r in _tiny_cells()[: lim["POST_MAXC"] - 10 + (1 if over else 0)]:
        B.tiny(c, r)
    return B.finish("maxc_mixed", min_valid=10)


def waves(seed, lim, factor=1):
    """factor 1: POST_WAVES + 1 candidates, factor 3: 3 * POST_WAVES - the solver's waves take several candidates each.  Four components, then polylines:
    32 quads of four linked segments spread evenly among polylines of one segment"""
    rng = np.random.default_rng(seed)
    B = _Builder()
    total = lim["POST_WAVES"] + 1 if factor == 1 else factor * lim["POST_WAVES"]
    _ordinary_quads(B, rng, _cells(*TOP, 4, 1), 1009, head=False)
    nq, nch = 32, total - 4
    at = set((k * nch) // nq for k in range(nq))
    for k in range(nch):
        if k in at:
            c = _convex_quad(rng, rng.uniform(80, 560), rng.uniform(200, 400), rng.uniform(50, 70), rmin=0.85, jitter=15.0)
            ids = [B.seg(c[s][0], c[s][1], c[(s + 1) % 4][0], c[(s + 1) % 4][1]) for s in range(4)]
            for j, i in enumerate(ids):
                B.rows[i]["leftPtr"] = ids[j - 1] if j else 0
                B.rows[i]["rightPtr"] = ids[j + 1] if j < 3 else 0
        else:
            B.tiny(int(rng.integers(0, 80)), int(rng.integers(ROW0, 80)))
    return B.finish("waves", min_valid=30)


def _shared_groups(B, sizes, first_id, cells):
    """groups of sizes[g] tiny segments; probe k of every segment of group g lies on component first_id + 15 g + k: 15 components of sizes[g] members"""
    at = 0
    for g, size in enumerate(sizes):
        for _ in range(size):
            i = B.tiny(*cells[at], left=1)
            at += 1
            px = B.pixels(i)
            for k in range(15):
                B.boundary[px[k][1], px[k][0]] = first_id + 15 * g + k
    return at


def maxg(seed, lim, over=False):
    """components of four members (all slots empty): more than POST_MAXC and fewer than POST_MAXG of them - the ranks run out -, over: more than POST_MAXG"""
    B = _Builder()
    ng = (lim["POST_MAXG"] + 15) // 15 + 2 if over else (lim["POST_MAXC"] + lim["POST_MAXG"]) // 2 // 15
    _shared_groups(B, [4] * ng, 10000, _tiny_cells())
    case = B.finish("maxg", min_valid=0, components=15 * ng)
    assert (15 * ng > lim["POST_MAXG"]) if over else (lim["POST_MAXC"] < 15 * ng < lim["POST_MAXG"])
    return case


def ht(seed, lim, over=False):
    """exactly POST_HT distinct ids under the probes (over: one more): ten ordinary quads, every other id seen by one segment"""
    rng = np.random.default_rng(seed)
    B = _Builder()
    _ten_quads(B, rng)
    want = lim["POST_HT"] - 10 + (1 if over else 0)
    cells = _tiny_cells()
    nid = 0
    while nid < want:
        i = B.tiny(*cells[nid // 15], left=1)
        px = B.pixels(i)
        for k in range(min(15, want - nid)):
            B.boundary[px[k][1], px[k][0]] = 20000 + nid
            nid += 1
    case = B.finish("ht", min_valid=10)
    assert len(np.unique(case.boundary[case.boundary > 0])) == lim["POST_HT"] + (1 if over else 0)
    return case


def members_total(seed, lim, over=False):
    """at most POST_MAXC components whose member counts add up to POST_MEMBERS exactly (over: to one more)"""
    B = _Builder()
    ng = min(64, lim["POST_MAXC"] // 15)
    total = lim["POST_MEMBERS"] + (1 if over else 0)
    nseg, rest = divmod(total, 15)
    sizes = [nseg // ng + (1 if g < nseg % ng else 0) for g in range(ng)]
    cells = _tiny_cells()
    at = _shared_groups(B, sizes, 30000, cells)
    if rest:      # one more segment, `rest` of whose probes lie on components of group 0
        i = B.tiny(*cells[at], left=1)
        px = B.pixels(i)
        for k in range(rest):
            B.boundary[px[k][1], px[k][0]] = 30000 + k
    case = B.finish("members_total", min_valid=0)
    m = memberships(case)
    assert len(m) == 15 * ng <= lim["POST_MAXC"] and sum(len(v) for v in m.values()) == total and min(len(v) for v in m.values()) >= 4
    return case


def _polyline(B, ends):
    ids = [B.seg(p[0], p[1], q[0], q[1]) for p, q in ends]
    for k, i in enumerate(ids):
        B.rows[i]["leftPtr"] = ids[k - 1] if k else 0
        B.rows[i]["rightPtr"] = ids[k + 1] if k + 1 < len(ids) else 0
    return ids


def hull_deep(seed, lim, nseg=50):
    """one polyline of nseg segments over the points P_i = (4 * 2^i, 4 * 2.2^i): segment k runs from P_k to one of the three outermost points, so that no length is
    below 5 % of the longest (nothing is dropped before the hull; the squared lengths still fit a float), every end point lies on the hull, and for every chord
    from the first point the farthest point is the last but one (x doubles, y grows by g with g^2 / (g - 1) > 4): the hull's construction nests one level per
    point - its explicit stack goes as deep as there are points.  44 segments stay below RDP_HULL_DEPTH = 48, 50 go past it.  (No gentler growth nests that
    deep: x growing by r and y by g peel point by point only for 1 / r + 1 / g < 1, so the coordinates leave the range of an int and the probes of these
    segments are outside the frame by comparison of doubles.)  Among ten ordinary quads."""
    rng = np.random.default_rng(seed)
    B = _Builder()
    _ten_quads(B, rng)
    assert nseg <= lim["POST_CAP"]
    pts = [(np.float32(4 * 2.0 ** i), np.float32(4 * 2.2 ** i)) for i in range(nseg + 3)]
    ids = _polyline(B, [(pts[k], pts[len(pts) - 1 - k % 3]) for k in range(nseg)])
    return B.finish("hull_deep", min_valid=10, hull_segments=ids)


def hull_pool(seed, lim, nseg=None, outer=16):
    """one polyline of nseg segments (default: POST_CAP) whose end points lie on the curve y = x^log2(3) / 64: `outer` points at x = 64, 128, 256, ... (y
    trebles from one to the next) and a cluster of points at x = 1, 1.2, 1.4, ...  Every cluster point is joined to one of the three outermost points and
    every other outer point to the outermost (no length below 5 % of the longest).  As in hull_deep the farthest point from a chord that starts in the cluster
    is the outer point before the chord's end, so the construction peels the outer points off one by one - but each of its pending calls now holds the whole
    cluster, and the index lists of the pending calls outgrow 16 * POST_CAP entries after a few levels, long before RDP_HULL_DEPTH.  All coordinates are
    below 2^28.  Among ten ordinary quads."""
    rng = np.random.default_rng(seed)
    B = _Builder()
    _ten_quads(B, rng)
    nseg = lim["POST_CAP"] if nseg is None else nseg
    assert nseg <= lim["POST_CAP"]
    p = np.log2(3.0)
    curve = lambda x: (np.float32(x), np.float32(x ** p / 64))
    far = [curve(64.0 * 2 ** j) for j in range(outer)]
    ncl = nseg - (outer - 3)
    near = [curve(1 + 0.2 * k) for k in range(ncl)]
    ends = [(near[k], far[outer - 1 - k % 3]) for k in range(ncl)] + [(far[j], far[outer - 1]) for j in range(outer - 3)]
    ids = _polyline(B, ends)
    return B.finish("hull_pool", min_valid=10, hull_segments=ids)


def hull_nesting(case, cap, pool, depth):
    """What the quick hull (oclrect.c:658-734) does with the end points of the case's polyline `hull_segments`, in doubles: a call finds the point farthest
    from its chord, splits the others into those outside the two new chords and calls itself on each subset.  The device keeps the subsets of all pending calls
    in one list of `pool` entries that starts with 4 * cap entries for the two halves and asks for room for 2 * (subset size) entries before a split, and keeps
    at most `depth` pending calls.  Returns ("fits" | "pool" | "depth", deepest nesting reached, most entries asked for)."""
    segs = case.segs
    ids = case.meta["hull_segments"]
    sq = np.array([np.float32((float(segs["x0"][i]) - float(segs["x1"][i])) ** 2 + (float(segs["y0"][i]) - float(segs["y1"][i])) ** 2) for i in ids])
    assert len(ids) <= cap and sq.min() > 1024 and sq.min() / sq.max() > np.float32(0.05) * np.float32(0.05)      # all long, none dropped as short
    pts = []
    for i in ids:
        pts += [(float(segs["x0"][i]), float(segs["y0"][i])), (float(segs["x1"][i]), float(segs["y1"][i]))]
    left = right = pts[0]
    for q in pts:
        if q[0] > right[0]:
            right = q
        if q[0] < left[0]:
            left = q
    up = (left[1] - right[1], right[0] - left[0])
    rest = [q for q in pts if q != left and q != right]
    top = [q for q in rest if (q[0] - left[0]) * up[0] + (q[1] - left[1]) * up[1] > 0]
    bottom = [q for q in rest if not (q[0] - left[0]) * up[0] + (q[1] - left[1]) * up[1] > 0]
    seen = {"depth": 0, "pool": 0}

    class Full(Exception):
        pass

    def off_chord(l, r, q):
        l2 = (l[0] - r[0]) ** 2 + (l[1] - r[1]) ** 2
        if l2 == 0.0:
            return (q[0] - l[0]) ** 2 + (q[1] - l[1]) ** 2
        t = ((q[0] - l[0]) * (r[0] - l[0]) + (q[1] - l[1]) * (r[1] - l[1])) / l2
        return (l[0] + t * (r[0] - l[0]) - q[0]) ** 2 + (l[1] + t * (r[1] - l[1]) - q[1]) ** 2

    def side(sub, l, r, level, used):
        if not sub:
            return
        d = [off_chord(l, r, q) for q in sub]
        at = int(np.argmax(d))              # (the first of equals)
        if d[at] < 0.01:
            return
        seen["depth"], seen["pool"] = max(seen["depth"], level + 1), max(seen["pool"], used + 2 * len(sub))
        if used + 2 * len(sub) > pool:
            raise Full("pool")
        if level + 1 >= depth:
            raise Full("depth")
        f = sub[at]
        nr, nl = (f[1] - r[1], r[0] - f[0]), (l[1] - f[1], f[0] - l[0])
        others = sub[:at] + sub[at + 1:]
        rs = [q for q in others if (q[0] - f[0]) * nr[0] + (q[1] - f[1]) * nr[1] > 0]
        ls = [q for q in others if (q[0] - f[0]) * nl[0] + (q[1] - f[1]) * nl[1] > 0]
        used += len(rs) + len(ls)
        side(rs, f, r, level + 1, used)
        side(ls, l, f, level + 1, used)

    try:
        side(top, left, right, 0, 4 * cap)
        side(bottom, right, left, 0, 4 * cap)
    except Full as e:
        return str(e), seen["depth"], seen["pool"]
    return "fits", seen["depth"], seen["pool"]


VALUE_CASES = (quads, axis_aligned, near_parallel, branches, threshold, bucket_order, chains)
# (case, keyword arguments, fits the device's capacities)
CAPACITY_CASES = (
    (cap_members_per_candidate, {"over": False}, True), (cap_members_per_candidate, {"over": True}, False),
    (maxc_chains, {"over": False}, True), (maxc_chains, {"over": True}, False),
    (maxc_mixed, {"over": False}, True), (maxc_mixed, {"over": True}, False),
    (waves, {"factor": 1}, True), (waves, {"factor": 3}, True),
    (maxg, {"over": False}, False), (maxg, {"over": True}, False),
    (ht, {"over": False}, True), (ht, {"over": True}, False),
    (members_total, {"over": False}, True), (members_total, {"over": True}, False),
)
HULL_CASES = ((hull_deep, {"nseg": 44}), (hull_deep, {"nseg": 50}), (hull_pool, {}))


def case_id(fn, kw):
    return fn.__name__ + "".join("-%s%s" % (k, int(v)) for k, v in sorted(kw.items()))

SEED = 3
ALL_CASES = tuple((fn, {}) for fn in VALUE_CASES) + tuple((fn, kw) for fn, kw, _ in CAPACITY_CASES) + HULL_CASES
_built = {}


def get(fn, kw=None, seed=SEED):
    """the case, built once per process (the tests share it and leave it unchanged)"""
    kw = kw or {}
    key = (case_id(fn, kw), seed)
    if key not in _built:
        c = fn(seed, ra.post_device_limits(), **kw)
        for a in (c.segs, c.boundary, c.table):
            a.setflags(write=False)
        _built[key] = c
    return _built[key]


def planes_crc(case):
    import zlib
    return [zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in (case.segs, case.boundary, case.table)]
