"""CPU tests of composited quads (include/rectdetect_hip.h, "composited quads"): the host taps - rd_composite_coefficients, rd_composite_covers,
rd_composite_tiles, rd_comp_limits - against the restatement of the header's text (tests/composite.py), bit for bit; coverage against an exact inside test in
rationals; the power-of-two round trip through tests/rectify.py; the host-only code under the sanitizers as a plain process.  No GPU, no tolerance."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import composite
from tests import helpers
from tests import rectify

IW, IH = 320, 200
QUADS = composite.seeded_quads(300, IW, IH)
LIM = ra.comp_limits()
TW, TH = LIM["tile_w"], LIM["tile_h"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_coefficients(quad, iw, ih):
    inv, box, status = ra.composite_coefficients(quad, iw, ih)
    winv, wbox, wstatus = composite.coefficients(quad, iw, ih)
    assert status == wstatus and tuple(int(v) for v in box) == tuple(wbox), (quad, box, wbox, status, wstatus)
    assert np.array_equal(bits(inv), bits(winv)), (quad, inv, winv)
    return status, wbox


def test_limits_and_the_item_layout():
    assert LIM == {"tile_w": 32, "tile_h": 16, "chunk": 64}
    assert ra.COMP_ITEM_DTYPE.itemsize == 72 and ra.COMP_ITEM_DTYPE.fields["patch"][1] == 64 and ra.COMP_ITEM_DTYPE.fields["b"][1] == 68


def test_coefficients_bit_for_bit():
    valid = empty = 0
    for q in QUADS:
        status, box = same_coefficients(q, IW, IH)
        assert status == 1
        assert ra.rectify_coefficients(q)[1] == 1      # (the forward coefficients the adjugate is made of are the rectifier's)
        valid += 1
        empty += box == composite.EMPTY_BOX
    assert valid == 300
    rng = np.random.default_rng(5)
    sq = np.array([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)])
    cases = []
    for m in (1e6, -1e6, 1e300, -1e300, 1e150, 1e-300):      # corners at the extremes: scaled, shifted, one corner only
        cases += [sq * m, sq * 50.0 + m, np.array([(10.0, 10.0), (100.0, 12.0), (m, m), (8.0, 90.0)]), np.array([(m, 10.0), (100.0, 12.0), (90.0, 80.0), (8.0, 90.0)])]
    cases += [np.array([(10.0, 10.0), (50.0, 10.0), (10.0, 50.0), (50.0, 50.0)]),      # a bow tie
              np.array([(10.0, 10.0), (50.0, 10.0), (20.0, 20.0), (10.0, 50.0)]),      # concave
              np.array([(10.0, 10.0), (30.0, 10.0), (50.0, 10.0), (10.0, 50.0)]),      # three corners on a line
              np.array([(10.0, 10.0), (10.0, 10.0), (50.0, 50.0), (10.0, 50.0)]),      # a repeated corner
              np.array([(np.nan, 10.0), (50.0, 10.0), (50.0, 50.0), (10.0, 50.0)]), np.array([(10.0, 10.0), (np.inf, 10.0), (50.0, 50.0), (10.0, 50.0)]),
              np.array([(10.0, 10.0), (50.0, 10.0), (50.0, -np.inf), (10.0, 50.0)]),
              sq * 40.0 + (-500.0, 50.0), sq * 40.0 + (900.0, 50.0), sq * 40.0 + (50.0, -500.0), sq * 40.0 + (50.0, 900.0),      # wholly outside: valid, empty box
              sq * 40.0 + (-41.5, 50.0), sq * 40.0 + (-42.5, 50.0), sq * 40.0 + (320.5, 50.0), sq * 40.0 + (321.5, 50.0),            # the box's own edge cases
              sq * 1000.0 - 300.0, sq * 0.25 + 7.3]
    cases += [composite.random_quad(rng, 160, 100, 80) * (-1 if k & 1 else 1) for k in range(20)]
    seen = set()
    for q in cases:
        for iw, ih in ((IW, IH), (1, 1), (65536, 65536), (96, 64)):
            status, box = same_coefficients(q, iw, ih)
            seen.add((status, box == composite.EMPTY_BOX))
            if not status:
                assert box == composite.EMPTY_BOX and not ra.composite_coefficients(q, iw, ih)[0].any()
                assert ra.composite_covers(q, iw, ih, 0, 0) == (False, 0.0, 0.0)
    assert seen == {(0, True), (1, True), (1, False)}
    # what the header says of the box at the frame's edge: ce = ceil(-1.5) + 1 = 0 is not < 0, ce = ceil(-2.5) + 1 = -1 is
    assert ra.composite_coefficients(sq * 40.0 + (-41.5, 50.0), IW, IH)[1][2] == 0 and ra.composite_coefficients(sq * 40.0 + (-42.5, 50.0), IW, IH)[1][2] == -1


@pytest.mark.parametrize("part", range(6))
def test_covers_on_every_pixel(part):
    """rd_composite_covers on all 64000 pixels of each of the 300 quads (50 per case) equals the restatement; s and t, bit for bit, on the first quads of each case"""
    L = ra.lib()
    st = np.zeros(2, np.float64)
    for k in range(50 * part, 50 * part + 50):
        q = np.ascontiguousarray(QUADS[k], np.float64).reshape(8)
        want, ws, wt, _ = composite.coverage(q, IW, IH)
        got = np.zeros((IH, IW), bool)
        f, qp, sp = L.rd_composite_covers, q.ctypes.data, st.ctypes.data
        full = k % 50 < 3
        _, box, _ = composite.coefficients(q, IW, IH)
        for y in range(IH):
            row = got[y]
            for x in range(IW):
                if f(qp, IW, IH, x, y, sp):
                    row[x] = True
                if full and box[0] <= x <= box[2] and box[1] <= y <= box[3]:
                    assert st[0].view(np.uint64) == ws[y, x].view(np.uint64) and st[1].view(np.uint64) == wt[y, x].view(np.uint64), (k, x, y)
        assert np.array_equal(got, want), (k, int((got != want).sum()))
        if want.any():      # no covered pixel outside the box
            ys, xs = np.nonzero(want)
            assert box[0] <= xs.min() and xs.max() <= box[2] and box[1] <= ys.min() and ys.max() <= box[3]


def _exact_inside(quad, x, y):
    """(inside?, far from every edge line?) of pixel centre (x, y) in rationals: far = the exact distance to each of the four lines exceeds 1e-6 pixel"""
    p = [(Fraction(float(a)), Fraction(float(b))) for a, b in np.asarray(quad).reshape(4, 2)]
    signs, far = [], True
    for i in range(4):
        (ax, ay), (bx, by) = p[i], p[(i + 1) % 4]
        cr = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
        signs.append(cr > 0)
        far = far and cr * cr > Fraction(1, 10 ** 12) * ((bx - ax) ** 2 + (by - ay) ** 2)
    return all(signs) or not any(signs), far


def test_coverage_is_the_exact_inside_test_away_from_the_edges():
    """Every pixel centre of the frame, for each of the 300 quads.  The distance to each edge line is first taken in float64: its error is below 1e-9 pixel here
    (products below 2.5e5 at 2^-53 relative error each, edges longer than half a pixel), so a pixel further than 1e-3 from all four lines is far from them exactly
    and its float signs are the exact ones.  The others go through fractions.Fraction.  Coverage must equal the exact inside test on every pixel that is exactly
    further than 1e-6 from every line, and at most 0.1 % of the pixels may be excluded."""
    Y, X = np.mgrid[0:IH, 0:IW].astype(np.float64)
    tested = excluded = 0
    for q in QUADS:
        cov, _, _, status = composite.coverage(q, IW, IH)      # (equal to rd_composite_covers on every pixel: the test above)
        assert status == 1
        p = np.asarray(q, np.float64).reshape(4, 2)
        pos, neg, near = np.ones((IH, IW), bool), np.ones((IH, IW), bool), np.zeros((IH, IW), bool)
        for i in range(4):
            (ax, ay), (bx, by) = p[i], p[(i + 1) % 4]
            length = np.hypot(bx - ax, by - ay)
            assert length > 0.5
            dist = ((bx - ax) * (Y - ay) - (by - ay) * (X - ax)) / length
            pos &= dist > 0
            neg &= dist < 0
            near |= np.abs(dist) <= 1e-3
        inside = pos | neg
        far = ~near
        assert np.array_equal(cov[far], inside[far]), "coverage differs from the inside test far from the edges"
        tested += IW * IH
        for y, x in zip(*np.nonzero(near)):
            ins, isfar = _exact_inside(q, int(x), int(y))
            if not isfar:
                excluded += 1
                continue
            assert bool(cov[y, x]) == ins, (q, x, y)
    assert excluded <= tested // 1000, (excluded, tested)


def test_the_axis_aligned_quad_covers_exactly_its_pixels_and_the_round_trip_is_the_identity():
    rng = np.random.default_rng(9)
    frame = rng.integers(0, 256, (IH, IW, 3), dtype=np.uint8)
    for n, x0, y0 in ((64, 10, 10), (64, 0, 0), (64, IW - 64, IH - 64), (32, 101, 57), (8, 33, 190), (128, 150, 40)):
        q = np.array([(x0 - 0.5, y0 - 0.5), (x0 + n - 0.5, y0 - 0.5), (x0 + n - 0.5, y0 + n - 0.5), (x0 - 0.5, y0 + n - 0.5)])
        cov, s, t, status = composite.coverage(q, IW, IH)
        want = np.zeros((IH, IW), bool)
        want[y0:y0 + n, x0:x0 + n] = True
        assert status == 1 and np.array_equal(cov, want)
        assert np.array_equal((s * n - 0.5)[cov].reshape(n, n), np.broadcast_to(np.arange(n, dtype=np.float64)[None, :], (n, n)))
        assert np.array_equal((t * n - 0.5)[cov].reshape(n, n), np.broadcast_to(np.arange(n, dtype=np.float64)[:, None], (n, n)))
        for y, x in ((y0, x0), (y0 + n - 1, x0 + n - 1)):
            assert ra.composite_covers(q, IW, IH, x, y)[0] and not ra.composite_covers(q, IW, IH, x0 + n, y)[0]
        patch, pst = rectify.patch(frame, q, n, n)
        assert pst == 1 and np.array_equal(patch, frame[y0:y0 + n, x0:x0 + n])
        blank = np.zeros_like(frame).reshape(IH, IW * 3)
        out, st = composite.draw(ra.PIX_BGR, [blank], IW, IH, composite.items([(q, 0, (0, 0, 0))]), patch[None])
        assert st.tolist() == [1]
        got = out[0].reshape(IH, IW, 3)
        assert np.array_equal(got[y0:y0 + n, x0:x0 + n], frame[y0:y0 + n, x0:x0 + n])
        got[y0:y0 + n, x0:x0 + n] = 0
        assert not got.any()


def test_tiles_against_the_restated_set():
    def check(item_array, iw, ih):
        got = ra.composite_tiles(item_array, iw, ih)
        want = composite.tiles(item_array, iw, ih, TW, TH)
        assert len(got) == len(want) and set(map(tuple, got.tolist())) == want
        assert got.tolist() == sorted(got.tolist(), key=lambda t: (t[1], t[0])), "the list is not in raster order"
        return got

    fill = lambda quads: ra.comp_items(quads)
    for k in range(0, 300, 10):
        check(fill(QUADS[k:k + 10]), IW, IH)
    assert len(check(fill(QUADS), IW, IH)) == (IW // TW) * ((IH + TH - 1) // TH)      # all 300: every tile, once
    outside = np.array([(400.0, 300.0), (460.0, 310.0), (450.0, 380.0), (395.0, 360.0)])
    assert len(check(fill([outside]), IW, IH)) == 0
    thin = np.array([(0.0, 0.0), (2.0, 0.0), (319.0, 198.0), (317.0, 198.0)])      # a thin diagonal across the frame: its box is the frame
    assert len(check(fill([thin]), IW, IH)) == (IW // TW) * ((IH + TH - 1) // TH)
    concave = np.array([(10.0, 10.0), (50.0, 10.0), (20.0, 20.0), (10.0, 50.0)])
    assert len(check(fill([concave, outside]), IW, IH)) == 0      # an invalid item reaches nothing
    one = np.array([(31.6, 15.6), (32.4, 15.6), (32.4, 16.4), (31.6, 16.4)])      # around the corner of four tiles: fl = 30, ce = 34
    assert check(fill([one]), 97, 61).tolist() == [[0, 0], [1, 0], [0, 1], [1, 1]]
    check(fill([thin, one, outside] + QUADS[:5]), 97, 61)
    assert len(check(fill([]), IW, IH)) == 0
    with pytest.raises(ValueError):
        ra.composite_tiles(fill([thin]), 0, IH)


def test_host_code_under_the_sanitizers_as_a_plain_process(tmp_path):
    """tests/native/comp_host_check.c with csrc/rd_comp_host.c, both compiled with -fsanitize=address,undefined, run as a process of its own"""
    csrc = os.path.join(helpers.ROOT, "rectdetect_amd", "csrc")
    exe = str(tmp_path / "comp_host_check")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", csrc, "-I", os.path.join(helpers.ROOT, "include"), os.path.join(helpers.ROOT, "tests", "native", "comp_host_check.c"),
           os.path.join(csrc, "rd_comp_host.c"), "-o", exe, "-lm"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode != 0 and "sanitize" in p.stderr and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip("this compiler has no address / undefined sanitizer runtime: %s" % p.stderr[-200:])
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "comp_host_check: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
