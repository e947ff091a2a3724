"""Page components for the tests: steps 2-7 of the contract of include/rectdetect_hip.h ("page components") restated in numpy and Python integers, written from the
header's text and not from the C or the kernels.  Run-based, so that a 2048 x 2048 page takes well under a second: the runs of a row come from the differences of
the padded mask, the runs of neighbouring rows that touch from two sorted searches per row, the components from a union-find over run numbers that keeps the smallest
number as the root, and every sum from closed forms per run.  Step 1 composes tests/scan.py (the ink decision at radius >= 1) with tests/tensor.py (the G plane)."""
import numpy as np

import rectdetect_amd as ra
from tests import scan
from tests import tensor

HEAD = np.dtype([(n, "<i4") for n in ("ink", "all", "found", "written", "ink_kept", "largest", "flags", "reserved")])
REC = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("area", "<i4"), ("first", "<i4"), ("sx", "<i8"), ("sy", "<i8")])
assert HEAD.itemsize == 32 and REC.itemsize == 40


def name(spec):
    return "r%d-k%d-d%d-m%d%s-c%d-a%d..%d-b%d%s" % (int(spec["radius"]), int(spec["k"]), int(spec["d"]), int(spec["oversample"]), "-inv" if int(spec["invert"]) else "",
                                                  int(spec["connectivity"]), int(spec["min_area"]), int(spec["max_area"]), int(spec["max_blobs"]), "-page" if int(spec["page"]) else "")


def row_bytes(pw):
    return (pw + 7) >> 3


def nbytes(spec, pw, ph):
    """step 7"""
    return 32 + 40 * int(spec["max_blobs"]) + (((row_bytes(pw) * ph + 7) & ~7) if int(spec["page"]) else 0)


def pack(mask):
    """a (ph, pw) mask in the RD_SCAN_BITS layout: (ph, (pw + 7) // 8) bytes, pad bits 0"""
    return np.packbits(np.asarray(mask, bool), axis=1, bitorder="big")


def unpack(bits, pw):
    """the (ph, pw) mask of a page in the RD_SCAN_BITS layout, its pad bits ignored"""
    return np.unpackbits(np.asarray(bits, np.uint8), axis=1, bitorder="big")[:, :pw].astype(bool)


def runs_of(mask):
    """the runs of a mask in raster order: (j, x0, x1) as int64 arrays, x1 inclusive"""
    m = np.asarray(mask, bool)
    d = np.diff(np.pad(m, ((0, 0), (1, 1))).astype(np.int8), axis=1)
    s, e = np.argwhere(d == 1), np.argwhere(d == -1)
    return s[:, 0].astype(np.int64), s[:, 1].astype(np.int64), e[:, 1].astype(np.int64) - 1


def components(mask, connectivity):
    """step 2: (the components of a (ph, pw) mask in ascending `first` as a REC array, the component's number per run, the runs (j, x0, x1) in raster order)"""
    m = np.asarray(mask, bool)
    ph, pw = m.shape
    j, x0, x1 = runs_of(m)
    n = len(j)
    reach = 1 if connectivity == 8 else 0
    up = list(range(n))

    def root(a):
        r = a
        while up[r] != r:
            r = up[r]
        while up[a] != r:
            up[a], a = r, up[a]
        return r

    start = np.searchsorted(j, np.arange(ph + 1))      # the first run of every row
    for row in range(1, ph):
        a0, a1, b0, b1 = start[row - 1], start[row], start[row], start[row + 1]
        if a0 == a1 or b0 == b1:
            continue
        lo = a0 + np.searchsorted(x1[a0:a1], x0[b0:b1] - reach, "left")      # runs above that end at or behind where this one starts ...
        hi = a0 + np.searchsorted(x0[a0:a1], x1[b0:b1] + reach, "right")     # ... and start at or before where it ends
        for b, l, h in zip(range(b0, b1), lo.tolist(), hi.tolist()):
            for a in range(l, h):
                ra_, rb_ = root(a), root(b)
                if ra_ != rb_:
                    up[max(ra_, rb_)] = min(ra_, rb_)
    roots = np.array([root(a) for a in range(n)], np.int64)
    uniq, comp = np.unique(roots, return_inverse=True)      # ascending root = ascending first: runs are numbered in raster order
    out = np.zeros(len(uniq), REC)
    if n == 0:
        return out, np.zeros(0, np.int64), (j, x0, x1)
    ln = x1 - x0 + 1
    k = len(uniq)
    out["area"] = np.bincount(comp, ln, k).astype(np.int64)
    sx, sy = np.zeros(k, np.int64), np.zeros(k, np.int64)
    np.add.at(sx, comp, ln * x0 + ln * (ln - 1) // 2)
    np.add.at(sy, comp, ln * j)
    out["sx"], out["sy"] = sx, sy
    bx0, by0 = np.full(k, pw, np.int64), np.full(k, ph, np.int64)
    bx1, by1 = np.full(k, -1, np.int64), np.full(k, -1, np.int64)
    np.minimum.at(bx0, comp, x0)
    np.minimum.at(by0, comp, j)
    np.maximum.at(bx1, comp, x1)
    np.maximum.at(by1, comp, j)
    out["x0"], out["y0"], out["x1"], out["y1"] = bx0, by0, bx1, by1
    out["first"] = j[uniq] * pw + x0[uniq]
    return out, comp, (j, x0, x1)


def brute(mask, connectivity):
    """step 2 by flooding pixel by pixel, for small masks: the check of components().  (area, first, x0, y0, x1, y1, sx, sy) per component in ascending first"""
    m = np.asarray(mask, bool)
    ph, pw = m.shape
    seen = np.zeros_like(m)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (1, -1), (-1, 1), (1, 1)] if connectivity == 8 else [])
    out = []
    for jj in range(ph):
        for ii in range(pw):
            if not m[jj, ii] or seen[jj, ii]:
                continue
            todo, px = [(ii, jj)], []
            seen[jj, ii] = True
            while todo:
                x, y = todo.pop()
                px.append((x, y))
                for dx, dy in nb:
                    u, v = x + dx, y + dy
                    if 0 <= u < pw and 0 <= v < ph and m[v, u] and not seen[v, u]:
                        seen[v, u] = True
                        todo.append((u, v))
            xs, ys = [p[0] for p in px], [p[1] for p in px]
            out.append((len(px), jj * pw + ii, min(xs), min(ys), max(xs), max(ys), sum(xs), sum(ys)))
    return out


def kept_of(areas, spec):
    """step 3"""
    a = np.asarray(areas, np.int64)
    lo, hi = int(spec["min_area"]), int(spec["max_area"])
    return (a >= lo) & ((a <= hi) if hi else True)


def page(mask, spec):
    """steps 2-7 for one valid quad's ink mask: its nbytes(spec, pw, ph) bytes"""
    m = np.asarray(mask, bool)
    ph, pw = m.shape
    B = int(spec["max_blobs"])
    out = np.zeros(nbytes(spec, pw, ph), np.uint8)
    head = out[:32].view(HEAD)
    recs, comp, (j, x0, x1) = components(m, int(spec["connectivity"]))
    if len(recs) == 0:
        return out      # (no ink: everything is zero)
    kept = kept_of(recs["area"], spec)
    found = int(kept.sum())
    head["ink"], head["all"], head["found"], head["written"] = int(m.sum()), len(recs), found, min(found, B)
    head["ink_kept"], head["largest"], head["flags"] = int(recs["area"][kept].sum()), int(recs["area"].max()), int(found > B)
    out[32:32 + 40 * min(found, B)] = recs[kept][:B].view(np.uint8)
    if int(spec["page"]):
        clean = np.zeros((ph, pw), bool)
        for r in np.nonzero(kept[comp])[0].tolist():
            clean[j[r], x0[r]:x1[r] + 1] = True
        p = pack(clean).reshape(-1)
        out[32 + 40 * B:32 + 40 * B + len(p)] = p
    return out


def from_bits(bits, pw, spec):
    """steps 2-7 from a page in the RD_SCAN_BITS layout ((ph, (pw + 7) // 8) bytes, pad bits ignored)"""
    return page(unpack(bits, pw), spec)


def ink(G0, spec):
    """step 1 behind the G plane: the ink mask of a (ph, pw) plane G0"""
    G = np.asarray(G0, np.int64)
    if int(spec["invert"]):
        G = 255 - G
    r = int(spec["radius"])
    if r == 0:
        return G <= int(spec["k"])
    N, T = scan.window(G, r)
    return 256 * N * (G + int(spec["d"])) < (256 - int(spec["k"])) * T


def scan_spec(spec):
    """the RD_SCAN_BITS spec whose pages are a blob spec's ink at radius >= 1"""
    return ra.scan_spec(ra.SCAN_BITS, int(spec["radius"]), int(spec["k"]), int(spec["d"]), 230, int(spec["oversample"]), bool(int(spec["invert"])))


def gray_spec(spec):
    return ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, int(spec["oversample"]))


def from_planes(planes, status, spec):
    """a job's (n, nbytes) bytes from its (n, ph, pw) G planes: zero bytes for an invalid quad"""
    planes = np.asarray(planes)
    n, ph, pw = planes.shape[:3]
    out = np.zeros((n, nbytes(spec, pw, ph)), np.uint8)
    for q in range(n):
        if status[q]:
            out[q] = page(ink(planes[q].reshape(ph, pw), spec), spec)
    return out


def from_pages(bitpages, status, pw, spec):
    """a job's (n, nbytes) bytes from the (n, ph, rb) pages of the RD_SCAN_BITS rectifier on the same job"""
    bitpages = np.asarray(bitpages)
    n, ph = bitpages.shape[:2]
    out = np.zeros((n, nbytes(spec, pw, ph)), np.uint8)
    for q in range(n):
        if status[q]:
            out[q] = from_bits(bitpages[q], pw, spec)
    return out


def job(bgr, quads, pw, ph, spec):
    """((n, nbytes) bytes of n quads of an (ih, iw, 3) BGR image, uint8 status[n]): the full restatement"""
    planes, st = tensor.tensors(bgr, quads, pw, ph, gray_spec(spec))
    return from_planes(planes.reshape(len(st), ph, pw), st, spec), st


def view(arr, spec, pw, ph):
    """(heads (n,), records (n, max_blobs), pages (n, ph, rb) or None) of (n, nbytes) bytes"""
    B = int(spec["max_blobs"])
    a = np.ascontiguousarray(arr, np.uint8).reshape(-1, nbytes(spec, pw, ph))
    heads = np.ascontiguousarray(a[:, :32]).view(HEAD).reshape(-1)
    recs = np.ascontiguousarray(a[:, 32:32 + 40 * B]).view(REC).reshape(len(a), B)
    pages = np.ascontiguousarray(a[:, 32 + 40 * B:32 + 40 * B + row_bytes(pw) * ph]).reshape(len(a), ph, row_bytes(pw)) if int(spec["page"]) else None
    return heads, recs, pages


def explain(got, want, spec, pw, ph, what=""):
    """raises with the first difference between two quads' bytes named by part"""
    got, want = np.asarray(got, np.uint8).reshape(-1), np.asarray(want, np.uint8).reshape(-1)
    assert got.shape == want.shape, "%s: %d bytes, expected %d" % (what, got.size, want.size)
    if np.array_equal(got, want):
        return
    (gh, gr, gp), (wh, wr, wp) = view(got, spec, pw, ph), view(want, spec, pw, ph)
    if gh[0] != wh[0]:
        raise AssertionError("%s: head %r, expected %r" % (what, gh[0], wh[0]))
    bad = np.nonzero(gr[0] != wr[0])[0]
    if len(bad):
        raise AssertionError("%s: %d records differ, first is record %d: %r, expected %r" % (what, len(bad), bad[0], gr[0][bad[0]], wr[0][bad[0]]))
    if gp is not None and not np.array_equal(gp, wp):
        ys, xs = np.nonzero(gp[0] != wp[0])
        raise AssertionError("%s: the cleaned page differs in %d bytes, first at row %d byte %d: %#x, expected %#x" % (what, len(ys), ys[0], xs[0], gp[0][ys[0], xs[0]], wp[0][ys[0], xs[0]]))
    raise AssertionError("%s: padding bytes differ" % what)
