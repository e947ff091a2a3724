"""Crafted inputs for decoded quads, shared by tests/test_cpu_code.py - which asserts from the restatement (tests/code.py) what each case claims about itself:
its id, its rotation, a tie, a distance or a count exactly at a limit - and tests/test_gpu_code.py, which runs the same cases on the GPU.  Every case is a
rendered code pasted into a gray 97 x 61 frame and read through the quad whose sampling is the identity (m = 1), so that bits, id and rot are known without the
restatement."""
import os
import re
from functools import lru_cache

import numpy as np

import rectdetect_amd as ra
from tests import code
from tests import helpers

IW, IH, X0, Y0, PX = 97, 61, 11, 9, 4
N, MIN_DIST = 6, 6
# the strides of the kernel's search: a wave is 64 threads, the block 64 * RD_CODE_WAVES (rd_code_tile.h, which rd_k_code.hip takes its block from): thread t looks at
# entries t, t + BLOCK, ... - entry BLOCK is the first that a thread merges with an entry it already holds
WAVE = 64
BLOCK = WAVE * int(re.search(r"#define RD_CODE_WAVES (\d+)", open(os.path.join(helpers.ROOT, "rectdetect_amd", "csrc", "rd_code_tile.h")).read()).group(1))
BOUNDARIES = tuple(sorted({WAVE - 1, WAVE, 255, 256, BLOCK - 1, BLOCK}))      # (255, 256: the sizes the issue names, a block's stride of a 4-wave kernel)
NDICTS = tuple(sorted({0, 1, 2, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 4096}))


@lru_cache(maxsize=None)
def big_dictionary():
    """4096 codes of 6 x 6 bits at distance >= 6 from each other in every rotation and from themselves turned (read only)"""
    d = ra.code_dictionary(N, 4096, MIN_DIST, seed=2026, tries=1 << 16)
    assert len(d) == 4096
    d.setflags(write=False)
    return d


def cells_image(v, polarity, dark=0, light=255):
    """the image of a (C, C) 0/1 matrix of v"""
    return np.kron(np.where(np.asarray(v) ^ polarity, light, dark).astype(np.uint8), np.ones((PX, PX), np.uint8))


def cells_of(spec, bits):
    """the (C, C) matrix of v of a code: the ring 0, the payload its bits"""
    n, b = int(spec["n"]), int(spec["border"])
    v = np.zeros((n + 2 * b, n + 2 * b), np.int64)
    for r in range(n):
        for c in range(n):
            v[b + r, b + c] = (bits >> (r * n + c)) & 1
    return v


def frame_with(img, bg=128):
    """a gray BGR frame with img at (X0, Y0), and the identity quad onto it"""
    h, w = img.shape
    assert X0 + w <= IW and Y0 + h <= IH
    f = np.full((IH, IW), bg, np.uint8)
    f[Y0:Y0 + h, X0:X0 + w] = img
    return np.repeat(f[..., None], 3, axis=2), code.identity_quad(X0, Y0, w, h)[None]


class Case:
    def __init__(self, name, spec, dictionary, img, claims):
        self.name, self.spec, self.dictionary, self.claims = name, spec, None if dictionary is None else np.array(dictionary, np.uint64), claims
        self.frame, self.quads = frame_with(img)
        self.pw = self.ph = img.shape[0]

    def __repr__(self):
        return self.name


def spec6(**kw):
    kw = dict(dict(n=N, border=1, inset=0, polarity=0, oversample=1, contrast=32, max_border=0, max_hamming=0), **kw)
    return ra.code_spec(**kw)


def rendered(name, spec, dictionary, bits, claims, flip_ring=0, dark=0, light=255):
    """the case of a rendered code; flip_ring: that many ring cells, spread round the ring, painted as v = 1"""
    v = cells_of(spec, bits)
    C, b = v.shape[0], int(spec["border"])
    ring = [(y, x) for y in range(C) for x in range(C) if x < b or x >= C - b or y < b or y >= C - b]
    for k in range(flip_ring):
        v[ring[(k * 7 + 3) % len(ring)]] = 1
    return Case(name, spec, dictionary, cells_image(v, int(spec["polarity"]), dark, light), dict(claims, bits=bits))


@lru_cache(maxsize=None)
def position_cases():
    """per dictionary size: the true code first, last and on both sides of a wave's stride (WAVE) and the block's (BLOCK; 255 and 256 too), each turned by another
    number of quarter turns"""
    D = big_dictionary()
    out = []
    for nd in NDICTS:
        spec = spec6()
        if nd == 0:
            out.append(rendered("ndict0", spec, None, int(D[0]), dict(id=-1, rot=0, hamming=65, second=65, ok=1)))
            continue
        for pos in sorted({p for p in (0, nd - 1) + BOUNDARIES if p < nd}):
            k = pos % 4
            claims = dict(id=pos, rot=k, hamming=0, ok=1)
            if nd == 1:
                claims["second"] = 65
            out.append(rendered("ndict%d-at%d-rot%d" % (nd, pos, k), spec, D[:nd], code.rotate(int(D[pos]), N, 4 - k), claims))
    return tuple(out)


def symmetric_code(n, seed):
    """a payload that looks like itself after every quarter turn"""
    x = code.splitmix64(seed)[1] & ((1 << (n * n)) - 1)
    return x | code.rotate(x, n, 1) | code.rotate(x, n, 2) | code.rotate(x, n, 3)


@lru_cache(maxsize=None)
def tie_and_limit_cases():
    D = big_dictionary()
    d = [int(v) for v in D[:64]]
    out = []
    dup = list(d[:20])
    dup[9] = d[5]
    out.append(rendered("duplicate-lowest-id-wins", spec6(), dup, d[5], dict(id=5, rot=0, hamming=0, second=0, ok=1)))
    out.append(rendered("duplicate-read-turned", spec6(), dup, code.rotate(d[5], N, 2), dict(id=5, rot=2, hamming=0, second=0, ok=1)))
    S = symmetric_code(N, 99)
    out.append(rendered("symmetric-rot0-wins", spec6(), [d[0], S, d[1]], S, dict(id=1, rot=0, hamming=0, ok=1)))
    out.append(rendered("two-ids-at-distance-1", spec6(max_hamming=1), [d[0] ^ 1, d[0] ^ 2], d[0], dict(id=0, rot=0, hamming=1, second=1, ok=1)))
    out.append(rendered("higher-id-nearer-in-a-later-rotation", spec6(max_hamming=36), [d[3] ^ 7, code.rotate(d[3], N, 1) ^ 1], d[3], dict(id=1, rot=1, hamming=1, second=3, ok=1)))
    # entries BLOCK apart are the SAME thread's: its own merge of best and second, not the shuffles', decides these
    full = [int(v) for v in D[:BLOCK + 40]]
    same = list(full)
    same[BLOCK + 5] = full[5]
    out.append(rendered("duplicate-one-stride-on-lowest-id-wins", spec6(), same, full[5], dict(id=5, rot=0, hamming=0, second=0, ok=1)))
    near = list(full)
    near[5] = full[BLOCK + 5] ^ 1
    out.append(rendered("one-stride-on-nearer-than-the-first", spec6(), near, full[BLOCK + 5], dict(id=BLOCK + 5, rot=0, hamming=0, second=1, ok=1)))
    far = list(full)
    far[BLOCK + 5] = full[5] ^ 1
    out.append(rendered("one-stride-on-is-the-runner-up", spec6(), far, full[5], dict(id=5, rot=0, hamming=0, second=1, ok=1)))
    tie = list(full)
    tie[5], tie[BLOCK + 5] = full[9] ^ 1, full[9] ^ 2
    tie[9] = full[BLOCK + 39]
    out.append(rendered("tie-one-stride-apart-lowest-id-wins", spec6(max_hamming=1), tie[:BLOCK + 39], full[9], dict(id=5, rot=0, hamming=1, second=1, ok=1)))
    flipped = d[7] ^ (1 << 4) ^ (1 << 30)
    for mh, ok in ((2, 1), (1, 0)):
        out.append(rendered("hamming2-max%d" % mh, spec6(max_hamming=mh), d, flipped, dict(id=7, rot=0, hamming=2, ok=ok)))
    for mb, ok in ((3, 1), (2, 0)):
        out.append(rendered("border3-max%d" % mb, spec6(max_border=mb), d, d[11], dict(id=11, rot=0, hamming=0, border_errors=3, ok=ok), flip_ring=3))
    for con, ok in ((160, 1), (161, 0)):
        out.append(rendered("contrast%d" % con, spec6(contrast=con), d, d[12], dict(id=12, rot=0, hamming=0, lo=40 * 256, hi=200 * 256, margin=160 * 256, ok=ok), dark=40, light=200))
    out.append(rendered("contrast255-on-0-and-255", spec6(contrast=255), d, d[13], dict(id=13, lo=0, hi=65280, margin=65280, ok=1)))
    for pol in (0, 1):      # a constant patch: every light = 0
        spec = spec6(polarity=pol, contrast=0, max_border=28, max_hamming=36)
        bits = (1 << 36) - 1 if pol else 0
        out.append(Case("constant-polarity%d" % pol, spec, d, np.full((8 * PX, 8 * PX), 93, np.uint8), dict(bits=bits, lo=93 * 256, hi=93 * 256, margin=0, border_errors=28 * pol, ok=1)))
    out.append(Case("constant-no-contrast", spec6(contrast=1), None, np.full((8 * PX, 8 * PX), 93, np.uint8), dict(bits=0, id=-1, ok=0)))
    return tuple(out)


@lru_cache(maxsize=None)
def shape_cases():
    """every n x border x polarity with a known payload and no dictionary; n = 8 with all 64 bits set (bit 63) against a dictionary of that one code"""
    out = []
    for n in range(3, 9):
        for border in (1, 2):
            for pol in (0, 1):
                bits = code.splitmix64(n * 100 + border * 10 + pol)[1] & ((1 << (n * n)) - 1)
                spec = ra.code_spec(n=n, border=border, inset=0, polarity=pol, contrast=200)
                out.append(rendered("n%d-b%d-p%d" % (n, border, pol), spec, None, bits, dict(id=-1, rot=0, hamming=65, second=65, border_errors=0, lo=0, hi=65280, ok=1)))
    for border in (1, 2):
        for pol in (0, 1):
            ones = (1 << 64) - 1
            spec = ra.code_spec(n=8, border=border, inset=0, polarity=pol, contrast=200)
            out.append(rendered("n8-ones-b%d-p%d" % (border, pol), spec, [ones], ones, dict(id=0, rot=0, hamming=0, second=65, border_errors=0, ok=1)))
            out.append(rendered("n8-bit63-b%d-p%d" % (border, pol), spec, [1 << 56, 1 << 63], 1 << 63, dict(id=0, rot=1, hamming=0, second=0, ok=1)))
    return tuple(out)


def all_cases():
    return position_cases() + tie_and_limit_cases() + shape_cases()
