"""The vote stage and the sampling kernel behind it (rd_votes_planes_device: rdk::polyline, rdk::polyline_ids, rdk::reduce_ls, rdk::sample_segments, the frame path's own
calls) on the crafted cases of tests/votecases.py, for both forms of the polyline stage.  The ids and the list equal the oracle's - the precondition -; the table, the
touched-slot list as a set, claim's empty entries, the probes buffer and the hand-over block equal what the numpy restatement of reduceLS gives, every int of every
buffer, guard words behind the last record included.  Then the tables' reuse from step to step under both ways of undoing a step, groups of frames in one launch, and
the sampling kernel's two limits below, at and above the record count.  What each case reaches is asserted without a GPU by tests/test_cpu_votecases.py."""
import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers, votecases as vc

CASES = vc.CASES
FORMS = (0, 1)
LIM = vc.LIM


def step_of(cases, form):
    c = cases[0]
    assert all(k.params() == c.params() for k in cases)
    return dict(frames=[(vc.resolve(k).mask, vc.resolve(k).boundary) for k in cases], ring=c.ring, minerror=c.minerror, size_thre=c.size_thre, form=form)


def pairs_on(r, slot):
    return sorted({(i, b) for _, i, b, s, _ in r.ref.touches if s == slot})


def check_frame(case, got, what, rflags, max_records, pack_records):
    """one frame of one step against the case's expectation; `what` names the run in every message"""
    r = vc.resolve(case)
    tag = f"{case.name} ({what})"
    # the precondition: the polyline stage gave the oracle's list and ids
    assert int(got.ctr[25]) == 0, f"{tag}: the single-block polyline kernel gave up"
    assert int(got.ctr[24]) == r.live_count, f"{tag}: live pixels {int(got.ctr[24])}, oracle {r.live_count}"
    assert helpers.segments_equal(got.segs, r.segs), f"{tag}: {int(got.segs.view('i4')[0])} records, oracle {int(r.segs.view('i4')[0])}"
    assert np.array_equal(got.ids, r.ids), f"{tag}: id plane"
    want = r.ref.table
    print(tag, "slots", len(r.ref.owner), "tlist", got.tlist_count, "records", int(got.segs.view("i4")[0]))
    # the table
    bad = np.flatnonzero((got.table != want).any(axis=1))
    if bad.size:
        s = int(bad[0])
        pytest.fail(f"{tag}: {bad.size} slots differ; slot {s} holds {got.table[s].tolist()}, expected {want[s].tolist()}; pairs (segment, boundary id) on it: {pairs_on(r, s)[:8]}, "
                    f"claimed by {r.ref.owner.get(s)}")
    assert np.array_equal(got.table, want)
    # tlist: exactly the slots with an id, each once
    slots = np.flatnonzero(want[:, 0])
    assert got.tlist_count == slots.size, f"{tag}: tlist counts {got.tlist_count} slots, {slots.size} are claimed"
    assert np.array_equal(np.sort(got.tlist), slots), f"{tag}: tlist is not the set of claimed slots (first difference: {np.setxor1d(got.tlist, slots)[:4].tolist()})"
    # claim: the empty word everywhere else, and nowhere on a claimed slot
    empty = got.claim == LIM["CLAIM_NONE"]
    assert np.array_equal(np.flatnonzero(~empty), slots), f"{tag}: claim's empty entries (first difference: slot {np.setxor1d(np.flatnonzero(~empty), slots)[:4].tolist()})"
    # the probes, every int of the buffer
    probes, _ = vc.expected_probes(r, want, max_records, got.probes.size)
    bad = np.flatnonzero(got.probes != probes)
    if bad.size:
        j = int(bad[0])
        i, k = j // LIM["PROBE_INTS"], j % LIM["PROBE_INTS"] // 6
        pytest.fail(f"{tag}: probes differ at int {j} (record {i}, probe {k}, word {j % 6}): {got.probes[j - j % 6: j - j % 6 + 6].tolist()}, expected {probes[j - j % 6: j - j % 6 + 6].tolist()}"
                    f"{'' if probes[j - j % 6] <= 0 else ', slot %d' % vc.slot_of(i, int(probes[j - j % 6]), r.nentry)}")
    assert np.array_equal(got.probes, probes)
    # the hand-over block, every int of it: from the list as the device left it (records with polyid 0 included), its own counters, the flags, the probes
    pack = vc.expected_pack(got.list_ints, got.ctr, rflags, probes, max_records, pack_records, got.pack.size)
    bad = np.flatnonzero(got.pack != pack)
    assert bad.size == 0, f"{tag}: the block differs at int {int(bad[0])}: {int(got.pack[bad[0]])}, expected {int(pack[bad[0]])} ({bad.size} ints differ)"
    assert np.array_equal(got.pack, pack)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(case, form):
    rflags = vc.rflags_pattern(1)
    got = ra.votes_planes_device([step_of([case], form)], clean=0, max_records=64, pack_records=64, rflags=rflags, guard=vc.GUARD)
    check_frame(case, got[0][0], f"form {form}", rflags[0], 64, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("clean", (0, 1))
def test_tables_are_reused(clean, form):
    """busy, sparse, busy again on one frame's tables: every step's table is that step's alone, whichever kernel undoes the step before"""
    order = [vc.BY_NAME[n] for n in ("hash_full", "wide_sparse", "hash_full", "wide_sparse")]
    rflags = vc.rflags_pattern(1)
    got = ra.votes_planes_device([step_of([c], form) for c in order], clean=clean, max_records=64, pack_records=64, rflags=rflags, guard=vc.GUARD)
    for s, case in enumerate(order):
        check_frame(case, got[s][0], f"step {s}, clean {clean}, form {form}", rflags[0], 64, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("clean", (0, 1))
@pytest.mark.parametrize("nb", (2, vc.MAXB))
def test_groups(nb, clean, form):
    """nb different cases as the frames of one launch, then the same cases on other frames' tables: each equals its single run"""
    first = vc.GROUP[-nb:]
    second = first[1:] + first[:1]
    rflags = vc.rflags_pattern(nb)
    got = ra.votes_planes_device([step_of(first, form), step_of(second, form)], clean=clean, max_records=64, pack_records=64, rflags=rflags, guard=vc.GUARD)
    for s, cases in enumerate((first, second)):
        for z, case in enumerate(cases):
            check_frame(case, got[s][z], f"step {s}, frame {z} of {nb}, clean {clean}, form {form}", rflags[z], 64, 64)


def sampling_limits():
    n = int(vc.resolve(vc.BY_NAME["sampling"]).segs.view("i4")[0])
    # (max_records, pack_records): records 0 .. n exist.  max_records below n + 1 (the last records get no probes), equal, above, the least the tap takes;
    # pack_records below, equal to and above the record count, and the header record alone
    return n, [(n, 64), (n + 1, 64), (n + 2, 64), (5, 64), (64, n), (64, n + 1), (64, n + 2), (64, 1), (6, 3), (n, n - 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_sampling_limits(form):
    case = vc.BY_NAME["sampling"]
    n, limits = sampling_limits()
    assert n >= 8
    rflags = vc.rflags_pattern(1)
    for max_records, pack_records in limits:
        got = ra.votes_planes_device([step_of([case], form)], clean=0, max_records=max_records, pack_records=pack_records, rflags=rflags, guard=vc.GUARD)
        check_frame(case, got[0][0], f"form {form}, max_records {max_records}, pack_records {pack_records}", rflags[0], max_records, pack_records)


@pytest.mark.gpu
def test_invalid_arguments():
    L = ra.lib()
    iw, ih = 16, 16
    n, nentry = iw * ih, iw * ih * 4 // 5
    m = np.zeros((2 * vc.MAXB + 2, n), np.int32)
    one, onef = np.ones(4, np.int32), np.ones(4, np.float32)
    zero = np.zeros(4, np.int32)
    rflags = np.zeros((vc.MAXB + 1) * 256, np.int32)
    P, R = LIM["PROBE_INTS"], LIM["PACK_RECORDS"] + (LIM["REC_INTS"] + LIM["PROBE_INTS"])
    outs = [np.zeros(k * (2 * vc.MAXB + 2), np.int32) for k in (n, n * 4, 64, nentry * 5, nentry + 1, nentry, 8 * P, 8 * P + R)]

    def call(iw=iw, ih=ih, nsteps=1, nb=1, form=zero, size_thre=one, clean=0, max_records=5, pack_records=1, probes_ints=5 * P, pack_ints=R, masks=m):
        return L.rd_votes_planes_device(0, iw, ih, nsteps, nb, masks.ctypes.data if masks is not None else None, m.ctypes.data, zero.ctypes.data, onef.ctypes.data, size_thre.ctypes.data,
                                        form.ctypes.data, clean, max_records, pack_records, rflags.ctypes.data, vc.GUARD, probes_ints, pack_ints, *[o.ctypes.data for o in outs])
    assert call() == 0 and call(nsteps=2, nb=vc.MAXB, clean=1) == 0
    assert call(iw=15) == -1 and call(ih=8) == -1 and call(nsteps=0) == -1 and call(nb=0) == -1 and call(nb=vc.MAXB + 1) == -1 and call(clean=2) == -1
    assert call(form=one * 2) == -1 and call(size_thre=-one) == -1 and call(masks=None) == -1
    assert call(max_records=4) == -1 and call(pack_records=0) == -1 and call(probes_ints=5 * P - 1) == -1 and call(pack_ints=R - 1) == -1
    assert call(max_records=6, probes_ints=5 * P) == -1 and call(pack_records=2, pack_ints=R) == -1
