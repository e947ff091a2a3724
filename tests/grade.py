"""Graded quads for the tests: steps 2-5 of the contract of include/rectdetect_hip.h ("graded quads") restated in numpy from a G plane, written from the header's
text and not from the kernel - the Laplacian as shifted slices of an edge-padded plane in int64, the cell of a pixel as two index vectors, the sums with np.add.reduceat over the cells' rectangles,
the histogram with np.bincount.  Step 1 is tests/tensor.py's { U8, NHWC, GRAY, m } element on tests/rectify.py's patch."""
import numpy as np

import rectdetect_amd as ra
from tests import tensor

FIELDS = ("n", "lo", "hi", "ne", "sg", "sgg", "sl", "sll")
CELLS = (1, 2, 4, 8)


def name(spec):
    return "c%d-d%d-b%d-e%d-m%d%s" % (int(spec["cells"]), int(spec["dark"]), int(spec["bright"]), int(spec["edge"]), int(spec["oversample"]), "-hist" if int(spec["hist"]) else "")


def gray_spec(spec):
    """the tensor spec of step 1"""
    return ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, int(spec["oversample"]))


def nbytes(spec):
    return 48 * int(spec["cells"]) ** 2 + 1024 * int(spec["hist"])


def laplacian(G):
    """step 2 for every pixel of a (ph, pw) plane: int64"""
    P = np.pad(np.asarray(G, np.int64), 1, mode="edge")
    return P[1:-1, :-2] + P[1:-1, 2:] + P[:-2, 1:-1] + P[2:, 1:-1] - 4 * P[1:-1, 1:-1]


def laplacian_loop(G):
    """step 2 pixel by pixel, neighbour indices clamped: the check of laplacian()"""
    G = np.asarray(G, np.int64)
    ph, pw = G.shape
    L = np.zeros((ph, pw), np.int64)
    for j in range(ph):
        for i in range(pw):
            L[j, i] = G[j, max(i - 1, 0)] + G[j, min(i + 1, pw - 1)] + G[max(j - 1, 0), i] + G[min(j + 1, ph - 1), i] - 4 * G[j, i]
    return L


def cell_index(pw, ph, cells):
    """step 3: the (ph, pw) array of record numbers"""
    cx, cy = (np.arange(pw) * cells) // pw, (np.arange(ph) * cells) // ph
    return cy[:, None] * cells + cx[None, :]


def cells_of(G, spec):
    """steps 2-4 for one valid quad: a GRADE_CELL_DTYPE array of shape (cells, cells), indexed [cy, cx]"""
    G = np.asarray(G, np.int64)
    ph, pw = G.shape
    c = int(spec["cells"])
    L = laplacian(G)
    # cells are rectangles: the first column and the first row of each (no cell is empty), and sums over the blocks between them
    x0 = np.searchsorted((np.arange(pw) * c) // pw, np.arange(c))
    y0 = np.searchsorted((np.arange(ph) * c) // ph, np.arange(c))
    rec = np.zeros((c, c), ra.GRADE_CELL_DTYPE)
    terms = {"n": lambda: np.ones_like(G), "lo": lambda: G <= int(spec["dark"]), "hi": lambda: G >= int(spec["bright"]), "ne": lambda: np.abs(L) >= int(spec["edge"]),
             "sg": lambda: G, "sgg": lambda: G * G, "sl": lambda: L, "sll": lambda: L * L}
    for f in FIELDS:
        rec[f] = np.add.reduceat(np.add.reduceat(terms[f]().astype(np.int64), y0, axis=0), x0, axis=1)
    return rec


def cells_of_loop(G, spec):
    """steps 2-4 pixel by pixel: the check of cells_of()"""
    G = np.asarray(G, np.int64)
    ph, pw = G.shape
    c = int(spec["cells"])
    L = laplacian_loop(G)
    rec = np.zeros((c, c), ra.GRADE_CELL_DTYPE)
    for j in range(ph):
        for i in range(pw):
            at = ((j * c) // ph, (i * c) // pw)
            g, l = int(G[j, i]), int(L[j, i])
            for f, v in zip(FIELDS, (1, g <= int(spec["dark"]), g >= int(spec["bright"]), abs(l) >= int(spec["edge"]), g, g * g, l, l * l)):
                rec[f][at] += int(v)
    return rec


def quad_bytes(G, spec):
    """steps 2-5 for one valid quad: its nbytes(spec) output bytes"""
    out = cells_of(G, spec).tobytes()
    if int(spec["hist"]):
        out += np.bincount(np.asarray(G, np.int64).ravel(), minlength=256).astype(np.uint32).tobytes()
    return np.frombuffer(out, np.uint8)


def from_planes(planes, status, spec):
    """the (n, nbytes(spec)) uint8 output of a job from its (n, ph, pw) G planes (the tensor rectifier's output, or tensor.tensors'): zero bytes for an invalid quad"""
    planes = np.asarray(planes)
    n, ph, pw = planes.shape[:3]
    out = np.zeros((n, nbytes(spec)), np.uint8)
    for q in range(n):
        if status[q]:
            out[q] = quad_bytes(planes[q].reshape(ph, pw), spec)
    return out


def records(bgr, quads, pw, ph, spec):
    """(the (n, nbytes(spec)) uint8 output of n quads of an (ih, iw, 3) BGR image, uint8 status[n]): the full restatement"""
    planes, st = tensor.tensors(bgr, quads, pw, ph, gray_spec(spec))
    return from_planes(planes.reshape(len(st), ph, pw), st, spec), st


def sharpness(cell):
    """rd_grade_sharpness restated in numpy float64, operation by operation"""
    if int(cell["n"]) == 0:
        return 0.0
    n, sl, sll = np.float64(int(cell["n"])), np.float64(int(cell["sl"])), np.float64(int(cell["sll"]))
    return float((sll - (sl * sl) / n) / n)


def percentile(hist, num, den):
    """rd_grade_percentile restated in Python integers"""
    h = [int(v) for v in np.asarray(hist).reshape(256)]
    total = sum(h)
    if den < 1 or den > 1 << 20 or num < 0 or num > den or total == 0:
        return -1
    cum = 0
    for v in range(256):
        cum += h[v]
        if cum * den >= num * total:
            return v
    raise AssertionError("not reached")


def assert_records(got, status, want, wstatus, spec, what=""):
    """names the quad, the cell and the field - or the histogram's bin - that differ"""
    assert np.array_equal(status, wstatus), "%s: status %r, expected %r" % (what, np.asarray(status).tolist(), np.asarray(wstatus).tolist())
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, "%s: %r %r, expected %r %r" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if np.array_equal(got, want):
        return
    gc, gh = ra.grade_view(got, spec)
    wc, wh = ra.grade_view(want, spec)
    for q in range(len(wc)):
        for cy in range(wc.shape[1]):
            for cx in range(wc.shape[2]):
                for f in FIELDS:
                    if gc[q, cy, cx][f] != wc[q, cy, cx][f]:
                        raise AssertionError("%s: quad %d cell (cx %d, cy %d) field %s: got %d, expected %d (the record: got %r, expected %r)" % (what, q, cx, cy, f, gc[q, cy, cx][f], wc[q, cy, cx][f], gc[q, cy, cx], wc[q, cy, cx]))
        if wh is not None and not np.array_equal(gh[q], wh[q]):
            v = int(np.nonzero(gh[q] != wh[q])[0][0])
            raise AssertionError("%s: quad %d histogram differs in %d bins, first at %d: got %d, expected %d" % (what, q, int((gh[q] != wh[q]).sum()), v, gh[q][v], wh[q][v]))
    raise AssertionError("%s: bytes differ outside records and histogram" % what)
