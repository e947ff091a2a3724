"""What tests/test_gpu_votecases.py relies on, asserted without a GPU: every crafted case of tests/votecases.py is what it claims to be - computed from the
oracle's ids (rdo_polyline) and the numpy restatement of reduceLS alone -, the oracle's rdo_reduce_ls equals that restatement on every case, and the constants the
cases are placed by (rd_votes_limits) are the ones in the kernels' source.  A path of the vote kernels listed in votecases.py that no case reaches fails here."""
import os
import re

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers, votecases as vc

CASES = vc.CASES
LIM = vc.LIM


def test_limits_are_the_kernels_constants():
    csrc = os.path.join(helpers.ROOT, "rectdetect_amd", "csrc")
    src = open(os.path.join(csrc, "rd_k_rect.hip")).read()
    define = lambda n, text=src: int(re.search(r"#define %s (\d+)" % n, text).group(1))
    assert {k: LIM[k] for k in ("RB_MAX", "CA_T", "CA_PROBES", "BA_T", "BA_PROBES", "block", "grid")} == \
        dict(RB_MAX=define("RB_MAX"), CA_T=define("CA_T"), CA_PROBES=define("CA_PROBES"), BA_T=define("BA_T"), BA_PROBES=define("BA_PROBES"), block=define("RV_NT"), grid=define("RV_GRID"))
    # the kernels spell their block size out: launch bounds and strides
    for kernel in ("k_reduce_claim", "k_reduce_box"):
        assert re.search(r"__launch_bounds__\(%d\) void %s\(" % (LIM["block"], kernel), src), kernel
        assert re.search(r"hipLaunchKernelGGL\(%s, dim3\(RV_GRID, 1, nb\), dim3\(RV_NT\)" % kernel, src), kernel
    # the hashes index with the top bits of a 32-bit product: the shifts belong to the table sizes
    assert re.search(r"unsigned h = \(slot\[q\] \* 2654435761u\) >> %d;" % (32 - LIM["CA_T"].bit_length() + 1), src)
    assert re.search(r"unsigned h = \(slot \* 2654435761u\) >> %d;" % (32 - LIM["BA_T"].bit_length() + 1), src)
    assert LIM["CA_T"] & (LIM["CA_T"] - 1) == 0 and LIM["BA_T"] & (LIM["BA_T"] - 1) == 0
    assert LIM["MAXB"] == define("RD_MAXB", open(os.path.join(csrc, "rd_poly_scratch.h")).read())
    assert LIM["CLAIM_NONE"] == 0x7f7f7f7f and "hipMemsetAsync(claim, 0x7f," in src
    kh = open(os.path.join(csrc, "rd_kernels.h")).read()
    for name, macro in (("PACK_FLAGS", "RD_PACK_FLAGS"), ("PACK_FLAGS_INTS", "RD_REGION_FIRST_BUDGET"), ("PACK_STATUS", "RD_PACK_STATUS"), ("PACK_STATUS_INTS", "RD_PACK_STATUS_INTS"),
                        ("RFLAGS_STATUS_AT", "RD_REGION_STATUS_AT"), ("PACK_RECORDS", "RD_PACK_RECORDS"), ("REC_INTS", "RD_REC_INTS")):
        assert LIM[name] == define(macro, kh), name
    assert LIM["PROBE_INTS"] == 15 * 6 and "#define RD_PROBE_INTS (15 * 6)" in kh
    assert vc.GUARD != LIM["CLAIM_NONE"]


def test_the_slot_wraps_as_the_kernel_does():
    """unsigned 32-bit product, bit 31 masked off, modulo nentry (oclrect.cl:446) - against numpy's uint32 arithmetic"""
    nentry = vc.nentry_of(*vc.SMALL)
    with np.errstate(over="ignore"):
        for i in (1, 2, 3, 4, 77):
            for b in vc.WRAP_IDS + (1, 4915, 4916):
                want = int(((np.uint32(i) * np.uint32(b)) & np.uint32(0x7fffffff)) % np.uint32(nentry))
                assert vc.slot_of(i, b, nentry) == want, (i, b)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_oracle_equals_the_restatement(case):
    r = vc.resolve(case)
    ih, iw = r.ids.shape
    table = np.zeros((r.nentry, 5), np.int32)
    helpers.oracle().rdo_reduce_ls(helpers.P(table), helpers.P(r.boundary), helpers.P(r.ids), iw, ih, r.nentry)
    bad = np.flatnonzero((table != r.ref.table).any(axis=1))
    assert bad.size == 0, f"{case.name}: slot {int(bad[0])}: oracle {table[bad[0]].tolist()}, restatement {r.ref.table[bad[0]].tolist()}"
    # the log accounts for the table: a slot is claimed exactly once, by its first touch
    first = {}
    for p, i, b, s, what in r.ref.touches:
        if s not in first:
            first[s] = what
            assert what == "claim" and r.ref.owner[s] == (p, i, b)
        else:
            assert what != "claim"
    assert sorted(first) == [int(s) for s in np.flatnonzero(r.ref.table[:, 0])]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_is_what_it_claims(case):
    f = vc.facts(case)
    r = vc.resolve(case)
    print(case.name, {k: (v if len(str(v)) < 120 else str(v)[:120] + "...") for k, v in f.items()})
    c = dict(case.claims)
    if "max_distinct" in c:
        assert max(f["distinct"]) == c.pop("max_distinct")
    if "hash_full" in c:
        h = c.pop("hash_full")
        # the work list is the pixels with an id, BLOCK per block: more distinct slots than a block's hash holds, so some go straight to memory - in both kernels
        assert r.live_count == int(np.count_nonzero(r.ids > 0)) and r.live_count > 2 * vc.BLOCK
        assert f["touched_per_block"][:2] == h["touched"] and min(h["touched"]) > vc.CA_T
        assert min(f["widened_per_block"][:2]) > vc.BA_T
        assert f["slots"] == h["slots"] and f["zero_box_slots"] == h["zero_box_slots"]
        assert f["claimant_touches"] == [1]
    if "same_window" in c:
        assert len(f["same_window"]) == c.pop("same_window")
        for s, ids in f["same_window"].items():
            assert len(ids) == 2 and ids[1] - ids[0] == r.nentry
    if "claimant_touches" in c:
        assert f["claimant_touches"] == c.pop("claimant_touches")
    if "touched_once" in c:
        assert len(f["touched_once"]) == c.pop("touched_once")
        for s in f["touched_once"]:
            assert r.ref.table[s][0] != 0 and not r.ref.table[s][1:].any()
    if "two_segments" in c:
        assert f["two_segments"] == c.pop("two_segments")
        for s, (owner, losers) in f["two_segments"].items():
            assert r.ref.table[s][0] == owner
            assert any(what == "dropped" and s2 == s and i in losers for _, i, _, s2, what in r.ref.touches)
    if "two_ids_apart" in c:
        assert len(f["two_ids_apart"]) == c.pop("two_ids_apart")
    if c.pop("wrap", False):
        assert f["products_past_2_31"] > 0 and f["products_past_2_32"] > 0 and int(r.boundary.max()) == 0x7fffffff
    if "rows" in c:
        assert f["rows"] == c.pop("rows") and f["cols"] == c.pop("cols")
        assert (f["clipped_windows"] == f["live"]) if c.pop("clipped") else f["clipped_windows"] == 0
    if "nonpositive" in c:
        assert f["nonpositive_cells"] == c.pop("nonpositive") and f["slots"] > 0
    if "live" in c:
        assert f["live"] == c.pop("live") and not r.ref.table.any()
    if "slots" in c:
        assert f["slots"] == c.pop("slots")
    if c.pop("sampling", False):
        assert f["probe_kinds"] == ["invalid record", "nonpositive", "other", "outside", "owned"] and f["probe_nonpositive"] == [-1, 0]
        assert f["invalid_records"] >= 1 and f["records"] >= 8
    assert not c, f"claims nobody checks: {c}"


def test_every_listed_path_has_a_case():
    """the union of the cases' facts covers what the vote kernels branch on"""
    fs = {c.name: vc.facts(c) for c in CASES}
    distinct = set().union(*(f["distinct"] for f in fs.values()))
    assert {vc.RB_MAX, vc.RB_MAX + 1, 2 * vc.RB_MAX, 2 * vc.RB_MAX + 1, 49} <= distinct
    touches = set().union(*(f["claimant_touches"] for f in fs.values()))
    assert {1, 2, 3, 4} <= touches and max(touches) >= 8
    owners = [(o, l) for f in fs.values() for o, l in f["two_segments"].values()]
    assert any(o < min(l) for o, l in owners) and any(o > max(l) for o, l in owners)
    assert any(f["live"] == 0 for f in fs.values())
    assert len(vc.GROUP) >= vc.MAXB and len({c.size for c in vc.GROUP}) == 1


def test_expected_blocks_of_the_sampling_case():
    """the expectations' own shape: what lies where in the probes buffer and the block for limits below, at and above the record count"""
    case = vc.BY_NAME["sampling"]
    r = vc.resolve(case)
    n = int(r.segs.view("i4")[0])
    PI, RI, R = LIM["PROBE_INTS"], LIM["REC_INTS"], LIM["PACK_RECORDS"]
    raw = np.zeros(vc.SMALL[0] * vc.SMALL[1] * 4, np.int32)
    raw[: r.segs.view("i4").size] = r.segs.view("i4")
    ctr, rflags = np.arange(64, dtype=np.int32) + 7, vc.rflags_pattern(1)[0]
    for max_records, pack_records in ((64, 64), (n, 64), (n + 1, n), (64, n + 1), (64, 1), (5, 3)):
        probes, _ = vc.expected_probes(r, r.ref.table, max_records, max_records * PI + 256)
        last = min(n, max_records - 1)
        assert (probes[:PI] == vc.GUARD).all() and (probes[(last + 1) * PI:] == vc.GUARD).all() and not (probes[PI: (last + 1) * PI] == vc.GUARD).any()
        pack = vc.expected_pack(raw, ctr, rflags, probes, max_records, pack_records, R + pack_records * (RI + PI) + 256)
        lastp = min(last, pack_records - 1)
        assert pack[R] == n and (pack[R + (lastp + 1) * RI: R + pack_records * RI] == vc.GUARD).all()
        F, FN, S, SN, AT = (LIM[k] for k in ("PACK_FLAGS", "PACK_FLAGS_INTS", "PACK_STATUS", "PACK_STATUS_INTS", "RFLAGS_STATUS_AT"))
        assert (pack[R + pack_records * RI + (lastp + 1) * PI:] == vc.GUARD).all() and (pack[S + SN: R] == vc.GUARD).all()
        assert np.array_equal(pack[:F], ctr[:F]) and np.array_equal(pack[F: F + FN], rflags[:FN]) and np.array_equal(pack[S: S + SN], rflags[AT: AT + SN]) and F + FN == S


def test_wrapper_refuses_mismatched_planes():
    m = np.zeros((16, 16), np.int32)
    with pytest.raises(ValueError):
        ra.votes_planes_device([dict(frames=[(m, m)]), dict(frames=[(m, m), (m, m)])])
    with pytest.raises(ValueError):
        ra.votes_planes_device([dict(frames=[(m, np.zeros((16, 17), np.int32))])])
