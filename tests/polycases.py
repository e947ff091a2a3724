"""Crafted masks for the polyline stage (rd_k_poly.hip), each with what it claims about the oracle's run on it (rdo_polyline alone; asserted without a GPU by
tests/test_cpu_polycases.py, relied upon by tests/test_gpu_polycases.py).  Three families:

  ties      masks whose list holds an ORPHAN record.  When two pixels of a segment tie for its maximum distance in a subdivision round (the 13-bit hash does
            not always break the tie) both become candidates; the later one in raster order decides the shared fields, the earlier one leaves a record o with
            rightPtr = h whose neighbours do not point back: h.leftPtr is another record.  The end-point join (pl:772-809, ascending id) still runs o's step,
            which writes h's start before the step of h's left neighbour reads it.  A join that orders a step only behind its own leftPtr / rightPtr
            (old_schedule_join below: the schedule the HIP kernels had) runs both steps in one round and gives another list.
  capacity  masks that sit on each fixed capacity of the single-block kernel (rectdetect_amd.polyline_limits) and one past it, and lists that just fit / are
            one record short.
  values    thresholds, loops, the frame ring, several chain starts, an empty mask, plane sizes around the 64-column words of the bit planes.

A case's seed is committed here.  If a later change of the stage's arithmetic breaks a claim, pick another seed (python -m tests.polycases search): do not weaken the claim."""
import ctypes
import math
import sys

import numpy as np

from tests import helpers

LS_BYTES = 56


# ---- the oracle with its taps
class PolyDbg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("connect", "chain", "chain_label", "num", "sub_label", "ids0")] + \
               [("converged", ctypes.c_int), ("before_join", ctypes.c_void_p), ("candidates", ctypes.c_int * 15)]


def records(raw, nbytes):
    """header + the records a list of nbytes bytes has room for, as LS_DTYPE"""
    from rectdetect_amd import LS_DTYPE
    n = min(int(raw[0]), nbytes // LS_BYTES - 1)
    return raw[: 14 * (max(n, 0) + 1)].view(LS_DTYPE).copy()


def oracle_run(mask, ring_nonzero, minerror, size_thre, lslist_bytes=None):
    """rdo_polyline on a 2-D mask: (list, ids, info) - info: 'before_join' (the list as the join finds it), 'candidates' (per round), 'live' (pixels
    of chains longer than size_thre), 'chains' (K)"""
    mask = np.ascontiguousarray(mask, dtype=np.int32)
    ih, iw = mask.shape
    N = iw * ih
    nbytes = N * 16 if lslist_bytes is None else int(lslist_bytes)
    raw = np.zeros((nbytes + 3) // 4, np.int32)
    before = np.zeros_like(raw)
    ids = np.zeros(N, np.int32)
    ids0 = np.zeros(N, np.int32)
    dbg = PolyDbg()
    dbg.ids0 = ids0.ctypes.data
    dbg.before_join = before.ctypes.data
    helpers.oracle().rdo_polyline(helpers.P(raw), nbytes, helpers.P(ids), helpers.P(mask), int(ring_nonzero), float(minerror), int(size_thre), iw, ih, ctypes.byref(dbg))
    info = dict(before_join=records(before, nbytes), candidates=[int(c) for c in dbg.candidates], live=int(np.count_nonzero(ids0)), chains=int(ids0.max()))
    return records(raw, nbytes), ids, info


# ---- the join, restated: one step in float32 (pl:772-809), the serial order, and the schedule the HIP kernels had
def join_step(src, g):
    """step g on the records `src`: the point (x, y) that becomes g's end and its right neighbour's start - every operation rounded to float32, as the kernel's"""
    f = np.float32
    h = int(src["rightPtr"][g])
    v0, v1, v2, v3 = (f(src[k][g]) for k in ("x0", "y0", "x1", "y1"))
    u0, u1, u2, u3 = (f(src[k][h]) for k in ("x0", "y0", "x1", "y1"))
    with np.errstate(all="ignore"):
        d = f(f(f(v2 - v0) * f(u3 - u1)) - f(f(v3 - v1) * f(u2 - u0)))
        mid = (f(f(v2 + u0) * f(0.5)), f(f(v3 + u1) * f(0.5)))
        if float(abs(d)) < 1e-6:
            return mid
        nn = f(f(f(v1 - u1) * f(u2 - u0)) - f(f(v0 - u0) * f(u3 - u1)))
        q = f(nn / d)
        wx, wy = f(v0 + f(q * f(v2 - v0))), f(v1 + f(q * f(v3 - v1)))
        e0 = np.sqrt(f(f(f(wx - v2) * f(wx - v2)) + f(f(wy - v3) * f(wy - v3))))
        e1 = np.sqrt(f(f(f(wx - u0) * f(wx - u0)) + f(f(wy - u1) * f(wy - u1))))
        return mid if (e0 > 10 and e1 > 10) else (wx, wy)


def _apply(ls, g, w):
    h = int(ls["rightPtr"][g])
    ls["x1"][g], ls["y1"][g], ls["x0"][h], ls["y0"][h] = w[0], w[1], w[0], w[1]


def serial_join(before):
    ls = before.copy()
    for g in range(1, len(ls)):
        if ls["polyid"][g] != 0 and ls["rightPtr"][g] != 0:
            _apply(ls, g, join_step(ls, g))
    return ls


def old_schedule_join(before, descending=False):
    """The join as d_refine3 and k_poly_persistent scheduled it before the orphan records were understood: rounds; a step runs once its own leftPtr (if smaller)
    and its own rightPtr (if smaller) are finished; the steps of a round all read the list as the round found it.  Where two steps of a round write the same
    point the one applied last stays: ascending ids, or descending.  Returns (list, [steps of each round])."""
    ls = before.copy()
    n = len(ls) - 1
    done = [True] + [bool(ls["polyid"][g] == 0 or ls["rightPtr"][g] == 0) for g in range(1, n + 1)]
    rounds = []
    while True:
        run = []
        for g in range(1, n + 1):
            if done[g]:
                continue
            h, l = int(ls["rightPtr"][g]), int(ls["leftPtr"][g])
            if (l <= 0 or l > g or l > n or done[l]) and (h > g or h > n or done[h]):
                run.append(g)
        if not run:
            return ls, rounds
        snap = ls.copy()
        for g in (reversed(run) if descending else run):
            _apply(ls, g, join_step(snap, g))
        for g in run:
            done[g] = True
        rounds.append(run)


def orphans(ls):
    """[(o, h, t)]: valid records o whose right neighbour h has another record t as its left neighbour"""
    out = []
    for g in range(1, len(ls)):
        h = int(ls["rightPtr"][g])
        if ls["polyid"][g] != 0 and h != 0 and int(ls["leftPtr"][h]) != g:
            out.append((g, h, int(ls["leftPtr"][h])))
    return out


def tie_facts(ls, before):
    """what a tie fixture claims, from the oracle's list and the list before the join"""
    orph = orphans(ls)
    serial = serial_join(before)
    old_a, rounds = old_schedule_join(before)
    old_d, _ = old_schedule_join(before, descending=True)
    same_round = {g: k for k, r in enumerate(rounds) for g in r}
    kinds, across64 = set(), False
    for o, h, t in orph:
        # the sibling: the record the same round made out of the same segment (same leftPtr, same level)
        sib = [g for g in range(1, len(ls)) if g != o and ls["leftPtr"][g] == ls["leftPtr"][o] and ls["level"][g] == ls["level"][o] and ls["polyid"][g] == ls["polyid"][o]
               and ls["startIndex"][g] > ls["startIndex"][o]]
        kinds.add("sibling_left_of_h" if (sib and t in sib) else "sibling_split_again")
        if t > 0 and ls["rightPtr"][t] == h and same_round.get(o) == same_round.get(t) and o // 64 != t // 64:
            across64 = True
    return dict(orphans=orph, kinds=kinds, serial_is_oracle=helpers.segments_equal(serial, ls), old_differs=not helpers.segments_equal(old_a, ls),
                old_differs_either_order=not helpers.segments_equal(old_a, ls) and not helpers.segments_equal(old_d, ls), across64=across64)


# ---- generators
def _mix(x):
    """splitmix64: the parameters of a mask from its seed, the same on every numpy"""
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x, z ^ (z >> 31)


class Rand:
    def __init__(self, seed):
        self.x = int(seed)

    def u(self):
        self.x, z = _mix(self.x)
        return (z >> 11) / float(1 << 53)

    def between(self, a, b):
        return a + (b - a) * self.u()


TIE_W, TIE_H, TIE_MINERROR, TIE_SIZE = 160, 96, 1.0, 10


def wavy_mask(seed, iw=TIE_W, ih=TIE_H):
    """four chains y = y0 + A sin(2 pi x / P + phi) + A2 sin(2 pi x / P2 + phi2), A in 2..7, A2 in 0..2, one pixel per column, |dy| <= 1 from column to column"""
    r = Rand(seed)
    m = np.zeros((ih, iw), np.int32)
    for c in range(4):
        y0 = 12 + 24 * c
        A, A2 = r.between(2, 7), r.between(0, 2)
        P, P2 = r.between(24, 90), r.between(7, 24)
        ph, ph2 = r.between(0, 2 * math.pi), r.between(0, 2 * math.pi)
        prev = None
        for x in range(3, iw - 3):
            y = int(round(y0 + A * math.sin(2 * math.pi * x / P + ph) + A2 * math.sin(2 * math.pi * x / P2 + ph2)))
            if prev is not None:
                y = max(prev - 1, min(prev + 1, y))
            m[y, x] = 1
            prev = y
    return m


def small_mask(seed, iw, ih):
    """wavy chains from the first to the last interior column of a small plane: one per 16 rows"""
    r = Rand(seed)
    m = np.zeros((ih, iw), np.int32)
    for c in range(max(1, ih // 16)):
        y0 = 8 + 16 * c
        A, P, ph = r.between(1.5, 4), r.between(9, 30), r.between(0, 2 * math.pi)
        prev = None
        for x in range(1, iw - 1):
            y = int(round(y0 + A * math.sin(2 * math.pi * x / P + ph)))
            if prev is not None:
                y = max(prev - 1, min(prev + 1, y))
            m[y, x] = 1
            prev = y
    return m


def shapes_mask(iw, shapes):
    """shapes = [(kind, size)]: 'line' = size pixels in a row, 'vee' = two diagonal legs of `size` steps (2 * size + 1 columns, apex below).  Packed left to
    right in bands, three empty columns / rows between any two (the bridging step joins curve ends one pixel apart, never three)."""
    x, y, band, rows = 3, 3, 0, []
    placed = []
    for kind, size in shapes:
        w, h = (size, 1) if kind == "line" else (2 * size + 1, size + 1)
        if x + w > iw - 3:
            x, y, band = 3, y + band + 3, 0
        placed.append((kind, size, x, y))
        x, band = x + w + 3, max(band, h)
    m = np.zeros((y + band + 3, iw), np.int32)
    for kind, size, x, y in placed:
        if kind == "line":
            m[y, x:x + size] = 1
        else:
            for i in range(-size, size + 1):
                m[y + size - abs(i), x + size + i] = 1
    return m


def diamond_mask(iw, ih, r):
    m = np.zeros((ih, iw), np.int32)
    cx, cy = iw // 2, ih // 2
    for dx in range(-r, r + 1):
        m[cy + (r - abs(dx)), cx + dx] = 1
        m[cy - (r - abs(dx)), cx + dx] = 1
    return m


def arch_mask(width=474, rows=15, cut=179, gap=5):
    """One chain of about 14000 pixels with both ends in the top row: down the left half of the plane in rows four apart, across at the bottom, up the right
    half.  The 4 x 8-hop search for a chain's ends does not reach that far, so the pixels of the left half link towards the left end and those of the right
    half towards the right end; `cut` shortens the first row until both halves are equally long: the two numberings then meet without a jump, the chain
    stays one sub-chain, and it has two pixels with number 1 (startCount 2: pl:475-506 makes such a record invalid, its pixels keep their id)."""
    m = np.zeros((4 * rows + 3, 2 * width + gap + 6), np.int32)
    x, y, d = 3 + cut, 3, 1
    for half in range(2):
        for k in range(rows):
            for _ in range(width - 1 - (cut if half == 0 and k == 0 else 0)):
                m[y, x] = 1
                x += d
            m[y, x] = 1
            if k < rows - 1:
                dy = 1 if half == 0 else -1
                m[min(y, y + 3 * dy):max(y, y + 3 * dy) + 1, x] = 1
                y, d = y + 4 * dy, -d
            elif half == 0:
                m[y, x:x + gap + 1] = 1
                x += gap + 1
    return m


def frame_mask(iw, ih):
    """a chain through the outermost interior pixels (row 1, then column iw - 2) and a wavy one inside"""
    m = small_mask(7, iw, ih)
    m[:3] = 0
    m[1, 1:iw - 1] = 1
    m[1:ih - 1, iw - 2] = 1
    return m


# ---- the cases
class Case:
    """build() -> mask; lsbytes: None (16 bytes per pixel) or a function of the record count the full-length run ends with; flag1: the single-block form
    must flag overflow; claims: {name: expected} checked against facts() by the CPU test"""

    def __init__(self, name, build, ring=0, minerror=1.0, size_thre=10, lsbytes=None, flag1=False, claims=None, tie=False):
        self.name, self.build, self.ring, self.minerror, self.size_thre, self.lsbytes, self.flag1, self.claims, self.tie = name, build, ring, minerror, size_thre, lsbytes, flag1, claims or {}, tie

    def __repr__(self):
        return self.name


_resolved = {}


def resolve(case):
    """(mask, lslist bytes, (oracle list, oracle ids, info)) of a case: computed once, shared by every test"""
    if case.name not in _resolved:
        mask = case.build()
        nbytes = None
        if case.lsbytes is not None:
            full, _, _ = oracle_run(mask, case.ring, case.minerror, case.size_thre)
            nbytes = case.lsbytes(int(full.view("i4")[0]))
        want = oracle_run(mask, case.ring, case.minerror, case.size_thre, nbytes)
        for a in want[:2]:
            a.setflags(write=False)
        _resolved[case.name] = (mask, nbytes, want)
    return _resolved[case.name]


def facts(case):
    mask, nbytes, (ls, ids, info) = resolve(case)
    f = dict(live=info["live"], chains=info["chains"], header=int(ls.view("i4")[0]), records=len(ls) - 1, max_candidates=max(info["candidates"]),
             valid=int(np.count_nonzero(ls[1:]["polyid"])), max_start_count=int(ls[1:]["startCount"].max()) if len(ls) > 1 else 0, mask_pixels=int(np.count_nonzero(mask)))
    if case.tie:
        f.update(tie_facts(ls, info["before_join"]))
    return f


# seeds of wavy_mask whose list holds an orphan (python -m tests.polycases search), by what tie_facts says about them
TIE_SEEDS = {
    "sibling_left_of_h": [2893, 4098],      # the sibling is still h's left neighbour: two steps with one right neighbour, both written by the old schedule's round
    "sibling_split_again": [696, 2007],     # the sibling was split again later: a third record is h's left neighbour
    "benign": [1466, 7135],                 # an orphan whose step changes nothing the other steps read: the old schedule gives the serial list
    "across64": [2947, 37818],              # the two steps' ids lie on different sides of a multiple of 64 (different waves of the join's block)
}


def tie_cases():
    out = []
    for kind, seeds in TIE_SEEDS.items():
        for seed in seeds:
            claims = dict(serial_is_oracle=True)
            if kind == "benign":
                claims.update(old_differs=False)
            else:
                claims.update(old_differs_either_order=True)
                if kind == "across64":
                    claims.update(across64=True)
                else:
                    claims.update(kinds={kind})
            out.append(Case("tie_%s_%d" % (kind, seed), (lambda seed=seed: wavy_mask(seed)), 0, TIE_MINERROR, TIE_SIZE, claims=claims, tie=True))
    return out


def capacity_cases():
    import rectdetect_amd as ra
    lim = ra.polyline_limits()
    LIVE, MAXSEG, MAXCAND = lim["PP_LIVE"], lim["PP_MAXSEG"], lim["PP_MAXCAND"]
    assert MAXSEG <= 1 << lim["PP_ID_BITS"]
    out = []
    # live pixels: lines of 1025 pixels keep 1024 (the end a chain is numbered from carries number 0 and belongs to no segment)
    per = 1024
    lines = [("line", per + 1)] * (LIVE // per) + ([("line", LIVE % per + 1)] if LIVE % per else [])
    out.append(Case("live_fits", lambda: shapes_mask(1040, lines), claims=dict(live=LIVE, chains=len(lines))))
    over = [("line", per + 2)] + lines[1:]
    out.append(Case("live_over", lambda: shapes_mask(1040, over), flag1=True, claims=dict(live=LIVE + 1, chains=len(lines))))
    # initial chains
    out.append(Case("chains_fit", lambda: shapes_mask(1100, [("line", 5)] * (MAXSEG - 2)), size_thre=2, claims=dict(chains=MAXSEG - 2, header=MAXSEG - 2)))
    out.append(Case("chains_over", lambda: shapes_mask(1100, [("line", 5)] * (MAXSEG - 1)), size_thre=2, flag1=True, claims=dict(chains=MAXSEG - 1, header=MAXSEG - 1)))
    # the largest record id reached through splits: a vee splits once, at its apex, in the first round
    V = MAXCAND - 8
    S = MAXSEG - 1 - 2 * V
    out.append(Case("ids_fit", lambda: shapes_mask(1100, [("vee", 4)] * V + [("line", 5)] * S), size_thre=2, claims=dict(chains=V + S, header=MAXSEG - 1, max_candidates=V)))
    out.append(Case("ids_over", lambda: shapes_mask(1100, [("vee", 4)] * V + [("line", 5)] * (S + 1)), size_thre=2, flag1=True, claims=dict(chains=V + S + 1, header=MAXSEG, max_candidates=V)))
    # candidates in one round
    out.append(Case("candidates_fit", lambda: shapes_mask(1100, [("vee", 4)] * MAXCAND + [("line", 5)] * 5), size_thre=2, claims=dict(max_candidates=MAXCAND, header=2 * MAXCAND + 5)))
    out.append(Case("candidates_over", lambda: shapes_mask(1100, [("vee", 4)] * (MAXCAND + 1) + [("line", 5)] * 5), size_thre=2, flag1=True,
                    claims=dict(max_candidates=MAXCAND + 1, header=2 * MAXCAND + 7)))
    # list size.  FITS(g) (pl:456) wants more than (g + 1) records' bytes: a list of (n + 2) * 56 bytes holds ids up to n
    mixed = [("vee", 4)] * 20 + [("line", 5)] * 5
    out.append(Case("list_fits", lambda: shapes_mask(200, mixed), size_thre=2, lsbytes=lambda n: (n + 2) * LS_BYTES, claims=dict(header=45, records=45, valid=45)))
    out.append(Case("list_one_short", lambda: shapes_mask(200, mixed), size_thre=2, lsbytes=lambda n: (n + 1) * LS_BYTES, flag1=True, claims=dict(records=45, valid=44)))
    out.append(Case("list_odd_bytes", lambda: shapes_mask(200, [("line", 7)] * 12), size_thre=2, lsbytes=lambda n: (n + 1) * LS_BYTES + 8, flag1=True, claims=dict(header=12, valid=12)))
    out.append(Case("list_chains_short", lambda: shapes_mask(200, [("line", 7)] * 12), size_thre=2, lsbytes=lambda n: (n - 2) * LS_BYTES, flag1=True, claims=dict(header=8, valid=8)))
    return out


SIZE_THRE_LINES = [("line", k) for k in (8, 9, 10, 11, 12, 13, 14)]


def value_cases():
    out = []
    # a line of L pixels is a chain of L - 1: with size_thre 10 the lines of 12, 13 and 14 pixels stay (more than size_thre pixels)
    out.append(Case("size_thre_edge", lambda: shapes_mask(120, SIZE_THRE_LINES), size_thre=10, claims=dict(chains=3)))
    out.append(Case("size_thre_0", lambda: shapes_mask(120, [("line", k) for k in (2, 3, 4)] + [("vee", 5)]), size_thre=0, claims=dict(chains=4)))
    for me in (0.5, 1.0, 2.5, 4.0):
        out.append(Case("minerror_%g" % me, lambda: wavy_mask(5), minerror=me))
    out.append(Case("closed_loop", lambda: diamond_mask(64, 48, 14), size_thre=10, claims=dict(chains=1, live=4 * 14 - 2)))
    for ring in (0, 1):
        out.append(Case("frame_chain_ring%d" % ring, lambda: frame_mask(97, 49), ring=ring, size_thre=5))
    out.append(Case("two_starts", arch_mask, size_thre=10, claims=dict(chains=1, max_start_count=2, valid=0)))
    out.append(Case("empty", lambda: np.zeros((40, 70), np.int32), claims=dict(header=0, live=0)))
    for k, (iw, ih) in enumerate(((16, 16), (63, 17), (65, 33), (129, 65))):
        out.append(Case("size_%dx%d" % (iw, ih), (lambda k=k, iw=iw, ih=ih: small_mask(20 + k, iw, ih)), size_thre=3))
    return out


def all_cases():
    return tie_cases() + capacity_cases() + value_cases()


def _search_one(seed):
    ls, _, info = oracle_run(wavy_mask(seed), 0, TIE_MINERROR, TIE_SIZE)
    if not orphans(ls):
        return None
    f = tie_facts(ls, info["before_join"])
    return seed, sorted(f["kinds"]), f["old_differs"], f["old_differs_either_order"], f["across64"], len(ls) - 1


def search(first, count, procs=8):
    """python -m tests.polycases search [first [count]]: the seeds whose mask holds an orphan, with what tie_facts says about each"""
    import multiprocessing as mp
    with mp.Pool(procs) as pool:
        for r in pool.imap_unordered(_search_one, range(first, first + count), chunksize=256):
            if r:
                print(*r, flush=True)


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "search":
    search(int(sys.argv[2]) if len(sys.argv) > 2 else 0, int(sys.argv[3]) if len(sys.argv) > 3 else 96000)
