"""Crafted pages for the component stage ("page components" of include/rectdetect_hip.h): every case is a page of packed bits, a blob spec and a CLAIM - what the
page was built to show, asserted on the restatement's result (tests/blobs.py) without a GPU by check().  The same cases then go to rd_blob_page_host
(tests/test_cpu_blobs.py) and through the device's component stage (tests/test_gpu_blobs.py), byte for byte.  Sizes hang on the tile of the tile kernel, TW x TH
from blob_limits(): a border between tiles, a tile corner and "at least 3 x 3 tiles" are where the kernel's tiles put them."""
import functools

import numpy as np

import rectdetect_amd as ra
from tests import blobs

LIM = ra.blob_limits()
TW, TH = LIM["tile_w"], LIM["tile_h"]


class Case:
    def __init__(self, name, mask, claim, bits=None, **spec):
        self.name, self.mask, self.claim = name, np.asarray(mask, bool), claim
        self.ph, self.pw = self.mask.shape
        self.bits = blobs.pack(self.mask) if bits is None else np.ascontiguousarray(bits, np.uint8)
        spec.setdefault("page", True)
        self.spec = ra.blob_spec(**spec)
        assert ra.blob_spec_ok(self.spec, self.pw, self.ph), name
        assert self.bits.shape == (self.ph, blobs.row_bytes(self.pw)) and np.array_equal(blobs.unpack(self.bits, self.pw), self.mask), name

    def __repr__(self):
        return "%s[%dx%d %s]" % (self.name, self.pw, self.ph, blobs.name(self.spec))


@functools.lru_cache(maxsize=None)
def _want(k):
    c = cases()[k]
    out = blobs.from_bits(c.bits, c.pw, c.spec)
    out.setflags(write=False)
    return out


def want(case):
    """the restatement's bytes of a case, computed once and shared"""
    return _want(cases().index(case))


def check(case):
    """the case's own claim, on the restatement: no GPU"""
    heads, recs, pages = blobs.view(want(case), case.spec, case.pw, case.ph)
    h, r = heads[0], recs[0][:int(heads[0]["written"])]
    assert int(h["ink"]) == int(case.mask.sum()) and int(h["reserved"]) == 0, case
    assert int(h["written"]) == min(int(h["found"]), int(case.spec["max_blobs"])) and int(h["flags"]) == int(int(h["found"]) > int(case.spec["max_blobs"])), case
    assert np.all(np.diff(r["first"]) > 0) and not recs[0][len(r):].view(np.uint8).any(), case
    if not int(h["flags"]):
        assert int(r["area"].sum()) == int(h["ink_kept"]), case
    if pages is not None:
        clean = blobs.unpack(pages[0], case.pw)
        assert int(clean.sum()) == int(h["ink_kept"]) and not (clean & ~case.mask).any(), case
        assert np.array_equal(blobs.pack(clean), pages[0]), "%r: pad bits in the cleaned page" % case
    case.claim(h, r, None if pages is None else blobs.unpack(pages[0], case.pw))


def _counts(all_=None, found=None, largest=None, flag=None):
    def claim(h, r, clean):
        for name, v in (("all", all_), ("found", found), ("largest", largest), ("flags", flag)):
            assert v is None or int(h[name]) == v, "%s = %d, the case is built for %d" % (name, int(h[name]), v)
    return claim


def _one_rooted_at(first):
    def claim(h, r, clean):
        assert int(h["all"]) == 1 and int(r[0]["first"]) == first and int(r[0]["area"]) == int(h["ink"]), (h, r[:1], first)
    return claim


def comb(pw, ph, bar, rows, pitch=2):
    """teeth in every pitch-th column over `rows`, joined by a bar in row `bar`"""
    m = np.zeros((ph, pw), bool)
    m[rows[0]:rows[1], ::pitch] = True
    m[bar, :] = True
    return m


def spiral(pw, ph, offset, pitch):
    """a one-pixel rectangular spiral from (offset, offset) inwards, its arms `pitch` apart"""
    m = np.zeros((ph, pw), bool)
    l, t, r, b = offset, offset, pw - 1 - offset, ph - 1 - offset
    x, y = l, t
    m[y, x] = True
    while r - x >= pitch:      # a leg shorter than the pitch would come too near the arm it runs up to
        m[y, x:r + 1] = True
        x, t = r, t + pitch
        if b - y < pitch:
            break
        m[y:b + 1, x] = True
        y, r = b, r - pitch
        if x - l < pitch:
            break
        m[y, l:x + 1] = True
        x, b = l, b - pitch
        if y - t < pitch:
            break
        m[t:y + 1, x] = True
        y, l = t, l + pitch
    return m


def dots(pw, ph, count):
    """`count` single pixels on the even rows and columns, in raster order"""
    m = np.zeros((ph, pw), bool)
    sites = [(j, i) for j in range(0, ph, 2) for i in range(0, pw, 2)]
    assert count <= len(sites)
    for j, i in sites[:count]:
        m[j, i] = True
    return m


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    rng = np.random.default_rng(2026)

    # trivial pages
    add("empty", np.zeros((TH + 8, TW + 6), bool), _counts(all_=0, found=0, largest=0, flag=0))
    m = np.zeros((TH + 3, TW + 5), bool)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    def corners(h, r, clean, pw=TW + 5, ph=TH + 3):
        assert r["first"].tolist() == [0, pw - 1, (ph - 1) * pw, ph * pw - 1] and r["area"].tolist() == [1] * 4
    add("corners", m, corners)
    for conn in (4, 8):
        add("full", np.ones((TH + 1, TW + 1), bool), _one_rooted_at(0), connectivity=conn)

    # sizes: noise at every size at which the launch shape changes
    for pw, ph in ((1, 1), (7, 3), (64, 1), (65, 2), (TW, TH), (TW + 1, TH + 1), (2 * TW + 3, 3 * TH - 1)):
        for conn in (4, 8):
            add("size", rng.random((ph, pw)) < 0.55, _counts(), connectivity=conn, min_area=1 if pw * ph < 100 else 2)
    add("size-1x1-ink", np.ones((1, 1), bool), _one_rooted_at(0))

    # connectivity
    for pw, ph in ((9, 7), (TW + 2, TH + 2)):
        board = (np.add.outer(np.arange(ph), np.arange(pw)) & 1) == 0
        add("checker", board, _counts(all_=(pw * ph + 1) // 2, largest=1), connectivity=4, max_blobs=4096)
        add("checker", board, _one_rooted_at(0), connectivity=8)
    board = (np.add.outer(np.arange(130), np.arange(129)) & 1) == 0
    def overflow(h, r, clean):
        assert int(h["found"]) == 8385 and int(h["flags"]) == 1 and int(h["written"]) == 4096
        assert r["first"].tolist() == np.nonzero(board.reshape(-1))[0][:4096].tolist()
        assert int(clean.sum()) == 8385      # (the page keeps what the records have no room for)
    add("checker-overflow", board, overflow, connectivity=4, max_blobs=4096)
    j = np.arange(2 * TH)
    for what, i in (("diagonal", j + TW - TH), ("antidiagonal", TW + TH - 1 - j)):      # both pass from one tile to the one diagonally opposite, through the corner the four share
        m = np.zeros((2 * TH, 2 * TW), bool)
        m[j, i] = True
        assert m[TH - 1, TW - 1] == m[TH, TW] and m[TH - 1, TW] == m[TH, TW - 1] and m[TH - 1, TW - 1] != m[TH - 1, TW]
        add(what, m, _one_rooted_at(int(i[0])), connectivity=8)
        add(what, m, _counts(all_=2 * TH, largest=1), connectivity=4)

    # late joins: the root must still be the smallest index
    pw, ph = 2 * TW + 3, 2 * TH + 5
    for conn in (4, 8):
        add("comb-joined-at-the-bottom", comb(pw, ph, ph - 1, (0, ph)), _one_rooted_at(0), connectivity=conn)
        add("comb-joined-at-the-top", comb(pw, ph, 0, (0, ph)), _one_rooted_at(0), connectivity=conn)
        add("comb-bar-on-a-tile's-last-row", comb(pw, ph, TH - 1, (0, TH)), _one_rooted_at(0), connectivity=conn)
        add("comb-bar-on-the-next-tile's-first-row", comb(pw, ph, TH, (0, TH + 1)), _one_rooted_at(0), connectivity=conn)
        add("comb-teeth-in-three-tile-rows", comb(pw, ph, ph - 2, (3, ph - 1), pitch=TW // 2 + 1), _one_rooted_at(3 * pw), connectivity=conn)
        add("spiral", spiral(3 * TW + 2, 3 * TH + 2, 0, 2), _one_rooted_at(0), connectivity=conn)
        two = spiral(3 * TW + 2, 3 * TH + 2, 0, 4) | spiral(3 * TW + 2, 3 * TH + 2, 2, 4)
        def twins(h, r, clean, pw=3 * TW + 2):
            assert int(h["all"]) == 2 and r["first"].tolist() == [0, 2 * pw + 2] and min(r["area"].tolist()) > 6 * TW
        add("two-spirals", two, twins, connectivity=conn)

    # filter edges: areas min_area - 1, min_area, max_area, max_area + 1
    m = np.zeros((12, 40), bool)
    m[1:3, 1:5] = True; m[1:4, 8:11] = True; m[1:5, 14:18] = True; m[1:5, 22:26] = True; m[5, 22] = True
    def bounded(h, r, clean):
        assert int(h["all"]) == 4 and r["area"].tolist() == [9, 16] and int(h["largest"]) == 17 and int(h["ink_kept"]) == 25
    def unbounded(h, r, clean):
        assert int(h["all"]) == 4 and r["area"].tolist() == [9, 16, 17] and int(h["ink_kept"]) == 42
    add("filter", m, bounded, connectivity=4, min_area=9, max_area=16)
    add("filter", m, unbounded, connectivity=4, min_area=9, max_area=0)

    # capacity edges
    for B in (1, 64, 4096):
        for count in (B - 1, B, B + 1):
            add("capacity", dots(160, 112, count), _counts(all_=count, found=count, flag=int(count > B)), connectivity=8, max_blobs=B)

    # pad bits: set in the input, ignored; zero in the cleaned page
    for pw in (1, 7, 9):
        m = rng.random((5, pw)) < 0.6
        b = blobs.pack(m)
        b[:, -1] |= (1 << (8 * blobs.row_bytes(pw) - pw)) - 1
        assert b[:, -1].all()
        add("pad-bits", m, _counts(), bits=b, connectivity=4)

    # noise, percolating tangles included
    for density in (0.05, 0.2, 0.35, 0.5, 0.6, 0.65, 0.8, 0.95):
        m = rng.random((100, 150)) < density
        for conn in (4, 8):
            add("noise-%02d" % round(100 * density), m, _counts(), connectivity=conn, min_area=2, max_area=0 if conn == 8 else 5000, max_blobs=256)

    # the sums need 64 bits; many components on a large page
    def big(h, r, clean):
        assert int(h["all"]) == 1 and int(r[0]["area"]) == 2 ** 22 and int(r[0]["sx"]) == int(r[0]["sy"]) == 4292870144 > 2 ** 31
    add("int64-sums", np.ones((2048, 2048), bool), big, connectivity=4, max_blobs=2)
    m = np.zeros((2048, 2048), bool)
    m[::2] = True
    def stripes(h, r, clean):
        assert int(h["all"]) == int(h["found"]) == 1024 and set(r["area"].tolist()) == {2048} and r["y0"].tolist() == list(range(0, 2048, 2))
    add("many-components", m, stripes, connectivity=8, max_blobs=1024, page=False)
    return tuple(out)


SMALL = lambda c: c.pw * c.ph <= 1 << 16
