"""Decoded quads without a GPU: the header's declarations and the library's exports, sizeof(rd_code_spec) and sizeof(rd_code) with their offsets, the numpy dtypes
against them, rd_code_spec_ok on every side of every bound, rd_code_cell_of against the restatement (tests/code.py) for every pixel, the legality rule for inset by
brute force, the restatement two ways, every host helper against its restatement in Python integers, the bound that makes 256 * sg unsigned, the upright quad on a
rendered code, the host-only code under the sanitizers as a plain process - and what every crafted case of tests/code_cases.py claims about itself.  No tolerance."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import code
from tests import code_cases
from tests import helpers

FUNCTIONS = ("rd_code_spec_ok", "rd_code_bytes", "rd_code_cell_of", "rd_code_rotate", "rd_code_limits", "rd_code_distance", "rd_code_dictionary", "rd_code_render", "rd_code_upright",
             "rd_rectifier_create_code")
SPEC_FIELDS = ("n", "border", "inset", "polarity", "oversample", "contrast", "max_border", "max_hamming")
# per field: (legal values at its bounds, illegal values one past them) for n = 6, border = 1 (C = 8: 28 ring cells, 36 payload cells)
BOUNDS = {"n": ((3, 8), (2, 9, 0, -1)), "border": ((1, 2), (0, 3, -1)), "inset": ((0, 1, 2, 3), (-1, 4)), "polarity": ((0, 1), (-1, 2)), "oversample": ((1, 2, 4), (0, 3, 5, 8, -1)),
          "contrast": ((0, 1, 254, 255), (-1, 256)), "max_border": ((0, 1, 27, 28), (-1, 29)), "max_hamming": ((0, 1, 35, 36), (-1, 37))}


def header():
    return open(os.path.join(helpers.ROOT, "include", "rectdetect_hip.h")).read()


def test_header_declares_the_functions_and_structs():
    txt = header()
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    assert re.search(r"typedef struct \{ int32_t n, border, inset, polarity, oversample, contrast, max_border, max_hamming; \} rd_code_spec;", txt)
    assert re.search(r"typedef struct \{ uint64_t bits; int32_t id, rot, hamming, second, border_errors, lo, hi, margin, ok, reserved; \} rd_code;", txt)
    assert txt.index("scanned pages:") < txt.index("graded quads:") < txt.index("decoded quads:") < txt.index("annotated frames:")
    assert "rd_code_bytes" in txt[txt.index("size_t rd_rectifier_patch_bytes") - 300:txt.index("size_t rd_rectifier_patch_bytes")], "rd_rectifier_patch_bytes' comment names the new kind"
    assert (ra.CODE_BYTES, ra.CODE_MAX_DICT, ra.CODE_NONE) == (48, 4096, 65)
    for name in ("code_spec", "code_spec_ok", "code_bytes", "code_cell_of", "code_rotate", "code_limits", "code_distance", "code_dictionary", "code_render", "code_upright", "code_view", "CODE_SPEC_DTYPE", "CODE_DTYPE"):
        assert hasattr(ra, name), name


def test_library_exports_the_functions():
    L = ctypes.CDLL(ra.LIB_PATH)
    missing = [n for n in FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_sizeof_the_structs_and_the_numpy_dtypes(tmp_path):
    spec_off = {f: 4 * k for k, f in enumerate(SPEC_FIELDS)}
    rec_off = {"bits": 0, "id": 8, "rot": 12, "hamming": 16, "second": 20, "border_errors": 24, "lo": 28, "hi": 32, "margin": 36, "ok": 40, "reserved": 44}
    checks = " && ".join(["offsetof(rd_code_spec, %s) == %d" % kv for kv in spec_off.items()] + ["offsetof(rd_code, %s) == %d" % kv for kv in rec_off.items()])
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "rectdetect_hip.h"\nint main(void) { return sizeof(rd_code_spec) == 32 && sizeof(rd_code) == 48 && %s ? 0 : 1; }\n' % checks)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-DCL_TARGET_OPENCL_VERSION=120", "-I", os.path.join(helpers.ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    assert ra.CODE_SPEC_DTYPE.itemsize == 32 and ra.CODE_SPEC_DTYPE.names == SPEC_FIELDS and {f: ra.CODE_SPEC_DTYPE.fields[f][1] for f in spec_off} == spec_off
    assert ra.CODE_DTYPE.itemsize == 48 and ra.CODE_DTYPE.names == code.FIELDS and {f: ra.CODE_DTYPE.fields[f][1] for f in rec_off} == rec_off
    assert ra.CODE_DTYPE.fields["bits"][0] == np.dtype("<u8")


def test_limits_and_the_default_spec():
    lim = ra.code_limits()
    assert lim == {"min_n": 3, "max_n": 8, "max_border": 2, "max_inset": 3, "oversamplings": (1, 2, 4), "max_side": 1024, "max_dict": 4096, "code_bytes": 48}
    a = np.full(10, -7, np.int32)
    ra.lib().rd_code_limits(a.ctypes.data + 4)
    assert a[0] == a[9] == -7 and a[1:9].tolist() == [3, 8, 2, 3, 7, 1024, 4096, 48]
    s = ra.code_spec()
    assert [int(s[f]) for f in SPEC_FIELDS] == [6, 1, 2, 0, 1, 32, 0, 0] and ra.code_spec_ok(s, 128, 128)


def test_spec_ok_on_every_side_of_every_bound():
    ok = ra.code_spec(6, 1, 2, 0, 2, 32, 3, 4)
    assert ra.code_spec_ok(ok, 128, 96) and code.spec_ok(ok, 128, 96) and ra.code_bytes(ok, 128, 96) == 48
    for field, (legal, illegal) in BOUNDS.items():
        for v, want in [(v, True) for v in legal] + [(v, False) for v in illegal]:
            s = ok.copy()
            s[field] = v
            assert ra.code_spec_ok(s, 128, 96) == code.spec_ok(s, 128, 96) == want, (field, v)
            assert ra.code_bytes(s, 128, 96) == (48 if want else 0)
    for n in range(3, 9):
        for border in (1, 2):
            C = n + 2 * border
            s = ra.code_spec(n, border, inset=0, max_border=C * C - n * n, max_hamming=n * n)
            assert ra.code_spec_ok(s, C, C) and ra.code_spec_ok(s, C, 1024) and ra.code_spec_ok(s, 1024, C)
            assert not ra.code_spec_ok(s, C - 1, C) and not ra.code_spec_ok(s, C, C - 1) and not ra.code_spec_ok(s, 1025, C) and not ra.code_spec_ok(s, C, 1025)
            for field, v in (("max_border", C * C - n * n + 1), ("max_hamming", n * n + 1)):
                bad = s.copy()
                bad[field] = v
                assert not ra.code_spec_ok(bad, 64, 64) and not code.spec_ok(bad, 64, 64), (n, border, field)
            for inset in (1, 2, 3):
                s = ra.code_spec(n, border, inset=inset)
                assert ra.code_spec_ok(s, 4 * C, 4 * C) and ra.code_spec_ok(s, 1024, 4 * C)
                assert not ra.code_spec_ok(s, 4 * C - 1, 4 * C) and not ra.code_spec_ok(s, 4 * C, 4 * C - 1), "pw = 4C - 1 with an inset"
                for pw, ph in ((4 * C - 1, 100), (C, C), (0, 64), (64, -1)):
                    assert ra.code_spec_ok(s, pw, ph) == code.spec_ok(s, pw, ph) == False
    assert ra.lib().rd_code_spec_ok(None, 64, 64) == 0 and ra.lib().rd_code_bytes(None, 64, 64) == 0


def test_cell_of_equals_the_restatement_for_every_pixel():
    for n, border, inset, pw, ph in ((3, 1, 0, 5, 5), (3, 1, 0, 6, 5), (3, 1, 0, 65, 7), (6, 1, 2, 33, 35), (8, 2, 3, 100, 52), (5, 2, 1, 37, 36)):
        s = ra.code_spec(n, border, inset)
        C = n + 2 * border
        assert ra.code_spec_ok(s, pw, ph)
        cx, okx = code.axis(pw, C, inset)
        cy, oky = code.axis(ph, C, inset)
        counted = np.zeros(C * C, np.int64)
        for j in range(ph):
            for i in range(pw):
                got = ra.code_cell_of(s, pw, ph, i, j)
                assert got == code.cell_of(s, pw, ph, i, j) == (int(cy[j]) * C + int(cx[i]), bool(okx[i] and oky[j])), (pw, ph, i, j)
                counted[got[0]] += got[1]
        assert counted.min() >= 1, "no cell is without a counted pixel"
        for i, j in ((-1, 0), (pw, 0), (0, -1), (0, ph)):
            assert ra.code_cell_of(s, pw, ph, i, j) == (-1, False)
    assert ra.code_cell_of(ra.code_spec(6, 1, 2), 31, 64, 0, 0) == (-1, False)


def test_the_legality_rule_leaves_no_cell_empty_and_is_needed():
    """per axis: at and above the bound every cell has a counted pixel, for every C and inset; below 4C with an inset cells do come out empty, first at C + 1"""
    for C in range(5, 13):
        for inset in range(4):
            least = 4 * C if inset else C
            for p in list(range(least, 401)) + [1023, 1024]:
                c, ok = code.axis(p, C, inset)
                assert np.array_equal(np.unique(c[ok]), np.arange(C)), (C, inset, p)
                if inset == 0:
                    assert ok.all()
        c, ok = code.axis(C + 1, C, 3)
        assert len(np.unique(c[ok])) < C, C
        c, ok = code.axis(C, C, 3)
        assert ok.all(), "one pixel per cell sits on the cell's centre"


def test_restatement_two_ways():
    rng = np.random.default_rng(17)
    for n, border, inset, pw, ph in ((3, 1, 0, 5, 5), (3, 1, 0, 6, 5), (3, 1, 0, 37, 29), (6, 1, 2, 32, 35), (8, 2, 3, 100, 52), (4, 2, 1, 33, 32)):
        s = ra.code_spec(n, border, inset)
        G = rng.integers(0, 256, (ph, pw))
        (a, ac), (b, bc) = code.means(G, s), code.means_loop(G, s)
        assert np.array_equal(a, b) and np.array_equal(ac, bc) and ac.min() >= 1, (n, border, inset, pw, ph)
        for nd in (0, 1, 2, 7):
            d = rng.integers(0, 1 << (n * n), nd, dtype=np.uint64) if n < 8 else rng.integers(0, 1 << 63, nd, dtype=np.uint64) * 2 + 1
            if nd == 7:
                d[5] = d[2]      # a duplicate
            ra_, rb = code.decide(a, s, d), code.decide(a, s, d, find=code.search_loop)
            assert ra_.tobytes() == rb.tobytes(), (n, nd, ra_, rb)
    z = code.from_planes(np.zeros((2, 8, 8), np.uint8), [0, 1], ra.code_spec(6, 1, 0, contrast=0))
    assert not z[0].any() and ra.code_view(z)[1]["ok"] == 1 and ra.code_view(z)[1]["hamming"] == 65, "an invalid quad is zero bytes; a valid one never is (hamming or id)"


def test_256_sg_needs_unsigned_32_bits_and_has_them():
    """a 205 x 205 cell of 255s: the header's bound"""
    s = ra.code_spec(3, 1, 0)
    cx, ok = code.axis(1024, 5, 0)
    assert np.bincount(cx).max() == 205 and ok.all()
    assert 2 ** 31 < 205 * 205 * 255 * 256 == 2743392000 < 2 ** 32 and "2 743 392 000" in header()
    M, cnt = code.means(np.full((1024, 1024), 255, np.uint8), s)
    assert cnt.max() == 205 * 205 and (M == 65280).all()


def test_rotate_distance_dictionary_render_upright_equal_their_restatements():
    rng = np.random.default_rng(3)
    for n in range(3, 9):
        for _ in range(20):
            p = int(rng.integers(0, 1 << 62)) * 4 + int(rng.integers(0, 4))
            p &= (1 << (n * n)) - 1
            for k in range(-1, 6):
                assert ra.code_rotate(p, n, k) == code.rotate(p, n, k % 4), (n, p, k)
            assert ra.code_rotate(ra.code_rotate(ra.code_rotate(ra.code_rotate(p, n), n), n), n) == p, "four quarter turns"
            assert code.popcount(ra.code_rotate(p, n)) == code.popcount(p)
        assert ra.code_rotate(1, n, 1) == 1 << (n - 1), "the top-left cell turns to the top-right"
        want = code.dictionary(n, 12, n - 1, 7 + n, 4000)
        got = ra.code_dictionary(n, 12, n - 1, seed=7 + n, tries=4000)
        assert got.tolist() == want and len(want) == 12, (n, got, want)
        assert ra.code_dictionary(n, 12, n - 1, seed=7 + n, tries=4000).tolist() == want, "deterministic"
        assert ra.code_distance(got, n) == code.distance(want, n) >= n - 1, "honours min_dist"
        assert ra.code_dictionary(n, 12, n - 1, seed=8 + n, tries=4000).tolist() != want, "another seed, other codes"
        assert len(ra.code_dictionary(n, 12, n - 1, seed=7 + n, tries=3)) <= 3
        for k in (0, 1, 5, 12):
            assert ra.code_distance(got[:k], n) == code.distance(want[:k], n)
        turned = got.copy()
        turned[7] = ra.code_rotate(int(got[2]), n, 3)
        assert ra.code_distance(turned, n) == code.distance(turned.tolist(), n) == 0
        for border in (1, 2):
            for pol in (0, 1):
                s = ra.code_spec(n, border, polarity=pol)
                for px in (1, 3):
                    assert np.array_equal(ra.code_render(s, want[0], px), code.render(s, want[0], px)), (n, border, pol, px)
    assert ra.code_distance(None, 6) == 65 and ra.code_distance([5], 3) == code.distance([5], 3)
    for bad in (lambda: ra.code_distance([1 << 36], 6), lambda: ra.code_distance([1], 9), lambda: ra.code_dictionary(2, 1, 1), lambda: ra.code_dictionary(6, 4097, 1),
                lambda: ra.code_render(ra.code_spec(6), 1 << 36), lambda: ra.code_render(ra.code_spec(6), 1, 65), lambda: ra.code_render(ra.code_spec(6), 1, 0)):
        with pytest.raises(ValueError):
            bad()
    assert code.splitmix64(0)[1] == 0xE220A8397B1DCDAF, "splitmix64's first value of seed 0"
    q = np.arange(8, dtype=np.float64).reshape(4, 2)
    for rot in range(-4, 9):
        assert np.array_equal(ra.code_upright(q, rot), code.upright(q, rot % 4))
    assert np.array_equal(ra.code_upright(q, 1)[0], q[3]), "read a quarter turn off: the patch's top-left corner is the quad's last"


def test_upright_reads_the_code_with_rot_0_and_the_same_id():
    """a rendered code read through the identity quad (x comes out exactly X + i: the patch IS the image) and through the same corners started one, two and three
    corners on: rot tells, and the quad rd_code_upright makes of it reads rot 0 with the same id"""
    D = code_cases.big_dictionary()[:32]
    spec = code_cases.spec6()
    img = ra.code_render(spec, int(D[9]), code_cases.PX)
    frame, quads = code_cases.frame_with(img)
    from tests import tensor
    plane, st = tensor.tensors(frame, quads, 32, 32, code.gray_spec(spec))
    assert st.tolist() == [1] and np.array_equal(plane.reshape(32, 32), img), "sampling is the identity"
    for r in range(4):
        turned = np.array([[quads[0][(c + r) % 4] for c in range(4)]])
        rec = ra.code_view(code.records(frame, turned, 32, 32, spec, D)[0])[0]
        assert (int(rec["id"]), int(rec["rot"]), int(rec["hamming"]), int(rec["ok"])) == (9, r, 0, 1), (r, rec)
        assert int(rec["bits"]) == code.rotate(int(D[9]), 6, 4 - r)
        up = ra.code_upright(turned[0], int(rec["rot"]))
        assert np.array_equal(up, quads[0])
        again = ra.code_view(code.records(frame, up[None], 32, 32, spec, D)[0])[0]
        assert (int(again["id"]), int(again["rot"]), int(again["bits"])) == (9, 0, int(D[9]))


def test_the_big_dictionary_bears_what_the_cases_need():
    D = code_cases.big_dictionary()
    assert len(D) == 4096 and len(set(D.tolist())) == 4096 and int(D.max()) < 1 << 36
    assert ra.code_distance(D, 6) >= code_cases.MIN_DIST
    assert ra.code_distance(D[:200], 6) == code.distance(D[:200].tolist(), 6)
    assert D[:50].tolist() == code.dictionary(6, 50, code_cases.MIN_DIST, 2026, 1 << 16)
    S = code_cases.symmetric_code(6, 99)
    assert all(code.rotate(S, 6, k) == S for k in range(4)) and code.distance([S], 6) == 0 and 0 < S < (1 << 36) - 1


@pytest.mark.parametrize("case", code_cases.all_cases(), ids=repr)
def test_every_crafted_case_is_what_it_claims(case):
    """sampling is the identity, and the restatement's record has every field the case names - which the GPU test then only compares bytes with"""
    from tests import tensor
    assert ra.code_spec_ok(case.spec, case.pw, case.ph) and int(case.spec["oversample"]) == 1
    plane, st = tensor.tensors(case.frame, case.quads, case.pw, case.ph, code.gray_spec(case.spec))
    assert st.tolist() == [1] and np.array_equal(plane.reshape(case.ph, case.pw), case.frame[code_cases.Y0:code_cases.Y0 + case.ph, code_cases.X0:code_cases.X0 + case.pw, 0])
    want, st = code.records(case.frame, case.quads, case.pw, case.ph, case.spec, case.dictionary)
    rec = ra.code_view(want)[0]
    for f, v in case.claims.items():
        assert int(rec[f]) == v, (case.name, f, int(rec[f]), v, rec)
    assert int(rec["reserved"]) == 0
    if case.dictionary is not None and len(case.dictionary) <= 64:
        loop = code.decide(code.means_loop(plane.reshape(case.ph, case.pw), case.spec)[0], case.spec, case.dictionary, find=code.search_loop)
        assert loop.tobytes() == rec.tobytes()


def test_the_position_cases_cover_every_size_and_stride_boundary():
    names = [c.name for c in code_cases.position_cases()]
    for nd in code_cases.NDICTS[1:]:
        assert "ndict%d-at0-rot0" % nd in names and any(n.startswith("ndict%d-at%d-" % (nd, nd - 1)) for n in names)
    txt = open(os.path.join(helpers.ROOT, "rectdetect_amd", "csrc", "rd_k_code.hip")).read()
    assert "WAVES = RD_CODE_WAVES, NT = RD_WAVE * WAVES" in txt and "id += NT" in txt, "the kernel's search strides by the block that rd_code_tile.h names"
    assert code_cases.WAVE == 64 and code_cases.BLOCK == 1024 == 64 * 16
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257, 4096, code_cases.BLOCK - 1, code_cases.BLOCK, code_cases.BLOCK + 1} == set(code_cases.NDICTS)
    for at in (63, 64, 255, 256, code_cases.BLOCK - 1, code_cases.BLOCK):
        assert sum(("-at%d-" % at) in n for n in names) >= 2, at      # (as the last entry of a dictionary, and inside a larger one)
        assert ("ndict4096-at%d-rot%d" % (at, at % 4)) in names
    for nd in (code_cases.BLOCK - 1, code_cases.BLOCK, code_cases.BLOCK + 1):      # a dictionary that ends just before, on and just behind the block's stride
        assert any(n.startswith("ndict%d-at%d-" % (nd, nd - 1)) for n in names)
    assert {c.claims["rot"] for c in code_cases.position_cases()} == {0, 1, 2, 3}
    ties = {c.name: c for c in code_cases.tie_and_limit_cases()}
    for name in ("duplicate-one-stride-on-lowest-id-wins", "one-stride-on-nearer-than-the-first", "one-stride-on-is-the-runner-up", "tie-one-stride-apart-lowest-id-wins"):
        d = ties[name].dictionary
        assert len(d) > code_cases.BLOCK + 5, "entries 5 and BLOCK + 5 are one thread's"


def test_host_code_under_the_sanitizers_as_a_plain_process(tmp_path):
    """tests/native/code_host_check.c with csrc/rd_code_host.c, both compiled with -fsanitize=address,undefined, run as a process of its own"""
    csrc = os.path.join(helpers.ROOT, "rectdetect_amd", "csrc")
    exe = str(tmp_path / "code_host_check")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-DCL_TARGET_OPENCL_VERSION=120", "-I", csrc, "-I", os.path.join(helpers.ROOT, "include"),
           os.path.join(helpers.ROOT, "tests", "native", "code_host_check.c"), os.path.join(csrc, "rd_code_host.c"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode != 0 and "sanitize" in p.stderr and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip("this compiler has no address / undefined sanitizer runtime: %s" % p.stderr[-200:])
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "code_host_check: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
