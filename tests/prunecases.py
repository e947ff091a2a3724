"""Crafted masks for the chain graph's prefilter and hop exits (rd_k_poly.hip: k_compact1<0>, k_find_ends1, k_number), in the manner of tests/polycases.py: each
case with what it claims about the oracle's run on it (rdo_polyline and its taps `chain`, `chain_label`, `num`; asserted without a GPU by
tests/test_cpu_prunecases.py, relied upon by tests/test_gpu_chain_prune.py).

The stage drops, before the chain graph, every chain pixel whose 8-connected component has at most size_thre pixels: the size filter counts the pixels of
SUB-chains, a sub-chain is part of one component, so such a component ends with id 0 whatever the graph computes for it.  `survivors` below is the number of
chain pixels in larger components (what the stage leaves in ctr[26]), `chain_pixels` all of them (ctr[0])."""
import ctypes

import numpy as np

from tests import helpers
from tests.polycases import Case, PolyDbg, diamond_mask, oracle_run, resolve, shapes_mask      # noqa: F401  (oracle_run, resolve: re-exported for the tests)
from tests import polycases as pc

RECT_SIZE_THRE = 20      # what the rect path passes


# ---- the oracle's taps and what they say about components
def taps_run(mask, ring, minerror, size_thre):
    """(chain mask before the loop roots are deleted, num tap) of rdo_polyline on a 2-D mask"""
    mask = np.ascontiguousarray(mask, dtype=np.int32)
    ih, iw = mask.shape
    N = iw * ih
    raw = np.zeros(N * 4, np.int32)
    ids = np.zeros(N, np.int32)
    chain, label, num = (np.zeros(N, np.int32) for _ in range(3))
    dbg = PolyDbg()
    dbg.chain, dbg.chain_label, dbg.num = chain.ctypes.data, label.ctypes.data, num.ctypes.data
    helpers.oracle().rdo_polyline(helpers.P(raw), N * 16, helpers.P(ids), helpers.P(mask), int(ring), float(minerror), int(size_thre), iw, ih, ctypes.byref(dbg))
    pre = chain != 0
    # a closed loop has lost its root pixel in the tap: its other pixels still carry the root as their label
    roots = np.unique(label[pre])
    pre[roots[roots >= 0]] = True
    return pre.reshape(ih, iw), num.reshape(ih, iw)


def component_sizes(on):
    """per chain pixel, in raster order: the number of pixels of its 8-connected component"""
    ih, iw = on.shape
    ys, xs = np.nonzero(on)
    index = {(int(y), int(x)): k for k, (y, x) in enumerate(zip(ys, xs))}
    parent = list(range(len(index)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for (y, x), k in index.items():
        for dy, dx in ((0, -1), (-1, -1), (-1, 0), (-1, 1)):
            j = index.get((y + dy, x + dx))
            if j is not None:
                a, b = find(k), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    root = np.array([find(k) for k in range(len(parent))], np.int64)
    return np.bincount(root, minlength=len(parent))[root] if len(parent) else np.zeros(0, np.int64)


_taps = {}


def facts(case):
    """polycases.facts plus what the taps say: chain_pixels, survivors, dead_share, components, max_num, at_max_num, mixed_waves (every full wave of 64
    consecutive chain pixels holds a dropped and a surviving one)"""
    f = pc.facts(case)
    if case.name not in _taps:
        mask = pc.resolve(case)[0]
        pre, num = taps_run(mask, case.ring, case.minerror, case.size_thre)
        _taps[case.name] = (component_sizes(pre), num)
    sizes, num = _taps[case.name]
    alive = sizes > case.size_thre
    n = len(sizes)
    f.update(chain_pixels=n, survivors=int(alive.sum()), dead_share=float((~alive).sum()) / max(n, 1), components=int((1.0 / sizes).sum().round()) if n else 0,
             max_num=int(num.max()), at_max_num=int((num == num.max()).sum()) if num.max() > 0 else 0)
    full = alive[: n // 64 * 64].reshape(-1, 64)
    f["mixed_waves"] = bool(len(full)) and bool(np.all(full.any(axis=1) & ~full.all(axis=1)))
    return f


# ---- generators
def dashes_and_lines(iw=283, ih=163, slot=56, lines=True):
    """Vertical lines of 40..150 pixels stacked in columns `slot` apart, and between them, every fourth row, horizontal dashes of 1..5 pixels three columns
    apart (a 1-pixel dash is an isolated pixel and goes in the tidy step).  A row then reads dashes, a line pixel, dashes, a line pixel, ...: in raster order
    the dropped and the surviving chain pixels alternate within every wave.  lines=False: the dashes alone."""
    m = np.zeros((ih, iw), np.int32)
    cols = list(range(3, iw - 3, slot))
    if lines:
        for c, x in enumerate(cols):
            y, k = 3, c
            while y + 40 <= ih - 3:
                n = min(40 + (37 * k) % 111, ih - 3 - y)
                m[y:y + n, x] = 1
                y, k = y + n + 3, k + 1
    for y in range(4, ih - 3, 4):
        k = y
        for x0 in cols:
            x = x0 + 4
            while True:
                n = 1 + k % 5
                if x + n > min(x0 + slot - 3, iw - 3):
                    break
                m[y, x:x + n] = 1
                x, k = x + n + 3, k + 1
    return m


def serpentine_mask(rows=90, width=474, step=4):
    """one chain: `rows` rows of `width` pixels, `step` rows apart, joined at alternating ends"""
    m = np.zeros((3 + step * (rows - 1) + 1 + 3, width + 6), np.int32)
    for k in range(rows):
        y = 3 + step * k
        m[y, 3:3 + width] = 1
        if k < rows - 1:
            m[y:y + step, 3 + width - 1 if k % 2 == 0 else 3] = 1
    return m


EDGE_T = 10
# lines of T - 1 .. T + 3 pixels, vees of 2 s + 1 = 9 .. 15 pixels
EDGE_SHAPES = [("line", EDGE_T + d) for d in (-1, 0, 1, 2, 3)] + [("vee", s) for s in (4, 5, 6, 7)] + [("line", EDGE_T + d) for d in (3, 1, 0, 2, -1)]
HOP_LINES = [("line", n) for n in (31, 32, 33, 34, 35, 65, 66, 67, 1055, 1056, 1057, 1088, 1089, 1090, 1091)]


def all_cases():
    import rectdetect_amd as ra
    LIVE = ra.polyline_limits()["PP_LIVE"]
    out = []
    # a line of L pixels is one component of L pixels and a chain of L - 1 (the end it is numbered from carries 0): with T = 10 the components of 9 and 10 pixels
    # are dropped before the graph, the lines and the vee of 11 go through it and the exact filter drops them (10 numbered pixels), those of 12 and more stay
    out.append(Case("prefilter_edge_lines", lambda: shapes_mask(120, EDGE_SHAPES), size_thre=EDGE_T,
                    claims=dict(components=14, chain_pixels=158, survivors=158 - 2 * 9 - 2 * 10 - 9, chains=6, live=2 * (11 + 12) + 12 + 14)))
    # a closed diamond of 12 pixels loses its root (11 left), its numbering starts at 0 (10 numbered): T = 10 and 11 send it through the graph, where the exact filter
    # drops it (10 > 10 is false); T = 12 drops it before the graph
    for T, surv in ((10, 12), (11, 12), (12, 0)):
        out.append(Case("prefilter_edge_diamond_T%d" % T, lambda: diamond_mask(40, 24, 3), size_thre=T, claims=dict(chain_pixels=12, components=1, survivors=surv, chains=0, live=0)))
    # (test_cpu_prunecases.py also asserts its shares: at least 600 chain pixels, at least 80 % of them in components of at most size_thre, like the bench stream's)
    out.append(Case("mixed_waves", dashes_and_lines, ring=1, minerror=4.0, size_thre=RECT_SIZE_THRE, claims=dict(mixed_waves=True, chain_pixels=5222, survivors=696)))
    out.append(Case("none_survive", lambda: dashes_and_lines(lines=False), ring=1, minerror=4.0, size_thre=RECT_SIZE_THRE, claims=dict(survivors=0, header=0, live=0)))
    # (with size_thre 0 every dash is a chain: 1305 of them, more than the single-block kernel's PP_MAXSEG, so that form flags and the multi-launch form is compared;
    #  the same pattern on a smaller plane stays below every capacity and is compared in both forms)
    MAXSEG = ra.polyline_limits()["PP_MAXSEG"]
    out.append(Case("all_survive", dashes_and_lines, ring=1, minerror=4.0, size_thre=0, flag1=1305 > MAXSEG - 2, claims=dict(chain_pixels=5222, survivors=5222, chains=1305)))
    out.append(Case("all_survive_small", lambda: dashes_and_lines(171, 83), ring=1, minerror=4.0, size_thre=0, flag1=379 > MAXSEG - 2, claims=dict(chain_pixels=1512, survivors=1512, chains=379)))
    # lengths around 33 and 33^2 = 1089 hops: where a pixel's walk ends in the first, the second round of k_number, and one hop before / behind.  The lines hold 7889
    # pixels together, fewer than a block of the compaction (8192): the second case adds one line, so that the survivor list's look-back crosses a block
    total = sum(n for _, n in HOP_LINES)
    out.append(Case("hop_edges", lambda: shapes_mask(1100, HOP_LINES), size_thre=10, claims=dict(chains=len(HOP_LINES), chain_pixels=total, survivors=total, max_num=1090)))
    out.append(Case("hop_edges_two_blocks", lambda: shapes_mask(1100, HOP_LINES + [("line", 700)]), size_thre=10,
                    claims=dict(chains=len(HOP_LINES) + 1, chain_pixels=total + 700, survivors=total + 700, max_num=1090)))
    assert total < 8192 < total + 700 < LIVE
    # 3 x 32 hops reach 33^3 = 35 937 pixels: behind that the numbering stays at the clamp, and that IS the reference's result
    out.append(Case("beyond_reach", serpentine_mask, size_thre=10, minerror=1.0, flag1=True,
                    claims=dict(chains=1, records=1, mask_pixels=42927, chain_pixels=42749, survivors=42749, max_num=35937, at_max_num=6812)))      # (the tidy step rounds the 178 corners)
    assert 42749 > LIVE      # (beyond_reach flags the single-block form: only the multi-launch form is compared)
    return out
