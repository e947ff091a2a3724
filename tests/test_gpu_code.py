"""Decoded quads on the GPU (rd_rectifier_create_code): every byte equals the restatement of the header's contract (tests/code.py on tests/tensor.py's gray plane) -
for patch sizes from one pixel per cell over both sides of the 64-lane row to 1024 x 1024, every inset at its smallest legal sizes, every n, border, polarity and
oversampling, dictionaries of every size round a wave's stride (64) and the block's (1024: tests/code_cases.py takes it from rd_code_tile.h; 255 to 257 too) with the true code
first, last and on both sides of each, duplicates and ties between entries one stride apart (one thread's), a code that looks
like itself turned, distances and counts exactly at max_hamming, max_border and contrast and one past them, a constant frame, rendered codes whose id, rot and bits
are known without the restatement (tests/code_cases.py; what each case claims is asserted in tests/test_cpu_code.py), all six pixel formats, host / device / pinned
frames, device / pinned output, invalid quads, outputs reused by later jobs, jobs in flight, empty and full jobs, argument errors, behind the poll of both detector
kinds, into memory that torch allocated, from the example program, and a code the compositor pasted into a device frame.  Every case also runs the
{ U8, NHWC, GRAY, m } tensor rectifier on the same job and compares the records with the restatement's steps 2-9 applied to THAT plane, so that a failure names the
launch at fault.  Every device output lies between guard bytes that must not change.  No tolerance anywhere."""
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import code
from tests import code_cases
from tests import composite
from tests import helpers
from tests import pixfmt
from tests import rectjobs
from tests.rectjobs import L, Out, STATUS, case, gray_job, gray_planes, mem, run_job      # (mem: the fixture)

pytestmark = pytest.mark.gpu
# inset 0, n = 3, border 1 (C = 5): one pixel per cell; one more column; one short of the 64-lane row, the row, one more; sizes that are no multiple of anything; the
# largest side against the smallest, both ways
SIZES0 = ((5, 5), (6, 5), (63, 6), (64, 5), (65, 7), (37, 29), (1024, 5), (5, 1024))


def reference(fmt, pw, ph, spec, dictionary=None, sel=None, seed=0):
    """(the bytes of the case's quads - or of those in sel -, status) from the shared planes"""
    g, st = gray_planes(fmt, pw, ph, int(spec["oversample"]), seed)
    sel = list(range(len(st))) if sel is None else list(sel)
    return code.from_planes(g[sel], st[sel], spec, dictionary), st[sel].copy()


@lru_cache(maxsize=None)
def noise_dictionary(n, ndict, seed=3):
    """ndict random payloads (read only).  At n = 3 there are 512 payloads: a large dictionary holds every one several times, and ties are the rule"""
    rng = np.random.default_rng(seed + 10 * n)
    d = rng.integers(0, 1 << 62, ndict, dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, ndict, dtype=np.uint64)
    d &= np.uint64((1 << (n * n)) - 1)
    d.setflags(write=False)
    return d


def test_shared_reference_is_the_restatement():
    spec = ra.code_spec(3, 1, 0, oversample=2, max_hamming=2)
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    d = noise_dictionary(3, 9)
    a, b = reference(ra.PIX_BGR, 9, 5, spec, d), code.records(bgr, quads, 9, 5, spec, d)
    code.assert_records(a[0], a[1], b[0], b[1])
    assert a[1].tolist() == STATUS.tolist() and a[0].shape == (4, 48)


def localise(got, status, gpu_plane, want, wstatus, spec, dictionary, what):
    """(a) the records against steps 2-9 of the restatement on the plane the GPU's first launch made - a difference here is the code kernel's -, (b) against the
    full restatement - a difference here alone is the tensor kernel's"""
    code.assert_records(got, status, code.from_planes(gpu_plane, status, spec, dictionary), wstatus, what + ": rdk::code, from the GPU's own G plane")
    code.assert_records(got, status, want, wstatus, what + ": the full restatement")


def check_specs(mem, fmt, pw, ph, specs, kinds=(("device", "device", 0),), seed=0):
    """every (spec, dictionary) on the case's job, with the tensor rectifier's plane of the same job (one per oversampling)"""
    iw, ih, planes, bgr, quads = case(fmt, seed)
    plane_of = {}
    for spec, d in specs:
        m = int(spec["oversample"])
        if m not in plane_of:
            plane_of[m], pstatus = gray_job(mem, fmt, planes, iw, ih, quads, pw, ph, m)
            assert pstatus.tolist() == STATUS.tolist()
        want, wstatus = reference(fmt, pw, ph, spec, d, seed=seed)
        rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=2, code=spec, dictionary=d)
        try:
            assert rect.patch_bytes == ra.code_bytes(spec, pw, ph) == 48 and rect.dtype == np.uint8 and rect.shape(len(quads)) == want.shape
            for kind, out_kind, pad in kinds:
                got, status = run_job(rect, mem, fmt, planes, iw, ih, quads, kind, out_kind, pad)
                localise(got, status, plane_of[m], want, wstatus, spec, d, "%s %s %dx%d %s frame, %s output, pad %d" % (ra.PIX_NAMES[fmt], code.name(spec, 0 if d is None else len(d)), pw, ph, kind, out_kind, pad))
                assert not got[1].any(), "an invalid quad gives zero bytes"
                assert got[[0, 2, 3]].any(axis=1).all(), "a valid quad never does"
        finally:
            rect.close()


# ---------------------------------------------------------------------------------------------- sizes; every n, border, polarity, oversampling
@pytest.mark.parametrize("k", range(len(SIZES0)), ids=["%dx%d" % s for s in SIZES0])
def test_every_size_without_inset(k, mem):
    pw, ph = SIZES0[k]
    d = noise_dictionary(3, (0, 5, 64, 300)[k % 4])
    check_specs(mem, ra.PIX_BGR, pw, ph, [(ra.code_spec(3, 1, 0, polarity=k % 2, oversample=(1, 2, 4)[k % 3], contrast=k, max_border=k % 5, max_hamming=k % 3), d if len(d) else None)])
    for bad in ((4, ph), (pw, 4), (1025, ph), (pw, 1025)):
        with pytest.raises(ValueError):
            ra.Rectifier(*bad, code=ra.code_spec(3, 1, 0))


def test_the_largest_patch_carries_256_sg_past_31_bits(mem):
    """one quad of 1024 x 1024 at m = 1 over a rendered code: a light cell is 205 x 205 pixels of 255 at most, 256 * sg = 2 743 392 000.  Step 1 is asserted on the
    GPU's own plane (a gray frame: G is the frame's value or a blend of two neighbours), the records from it"""
    spec = ra.code_spec(3, 1, 0, contrast=255, max_hamming=0)
    bits = 0b101110011
    frame, quad = code_cases.frame_with(ra.code_render(spec, bits, 8))      # 40 x 40 pixels stretched to 1024 x 1024
    plane, pstatus = gray_job(mem, ra.PIX_BGR, [frame], code_cases.IW, code_cases.IH, quad, 1024, 1024, 1)
    assert pstatus.tolist() == [1] and plane.min() == 0 and plane.max() == 255
    rect = ra.Rectifier(1024, 1024, max_quads=1, njobs=1, code=spec, dictionary=[bits, 0])
    try:
        got, status = run_job(rect, mem, ra.PIX_BGR, [frame], code_cases.IW, code_cases.IH, quad)
    finally:
        rect.close()
    want = code.from_planes(plane, pstatus, spec, [bits, 0])
    code.assert_records(got, status, want, [1], "1024 x 1024")
    rec = ra.code_view(got)[0]
    M, cnt = code.means(plane[0], spec)
    assert cnt.max() == 205 * 205 and int((M * cnt).max()) > 2 ** 31, "a cell whose 256 * sg does not fit int32"
    assert (int(rec["bits"]), int(rec["id"]), int(rec["rot"]), int(rec["hamming"]), int(rec["border_errors"])) == (bits, 0, 0, 0, 0)


def inset_specs(n, border, k):
    return [(ra.code_spec(n, border, inset, polarity=(k + inset) % 2, oversample=(1, 2, 4)[(k + inset) % 3], contrast=40, max_border=2, max_hamming=n), noise_dictionary(n, (2, 65, 257)[(k + inset) % 3]))
            for inset in (1, 2, 3)]


@pytest.mark.parametrize("n,border,pw,ph", [(3, 1, 20, 20), (3, 1, 21, 23), (4, 2, 32, 32), (4, 2, 33, 35), (8, 2, 48, 48), (8, 2, 49, 51), (8, 2, 100, 52)])
def test_every_inset_at_its_smallest_sizes(n, border, pw, ph, mem):
    check_specs(mem, ra.PIX_BGR, pw, ph, inset_specs(n, border, pw))
    C = n + 2 * border
    if pw == 4 * C:
        for bad in ((pw - 1, ph), (pw, ph - 1)):
            with pytest.raises(ValueError):
                ra.Rectifier(*bad, code=ra.code_spec(n, border, 1))


@pytest.mark.parametrize("n", range(3, 9))
def test_every_n_border_polarity_and_oversampling(n, mem):
    specs = [(ra.code_spec(n, border, (n + border + pol) % 4, polarity=pol, oversample=m, contrast=16, max_border=4, max_hamming=n * n // 3), noise_dictionary(n, 65 + 64 * pol))
             for border in (1, 2) for pol in (0, 1) for m in (1, 2, 4)]
    check_specs(mem, ra.PIX_BGR, 53, 49, specs)


# ---------------------------------------------------------------------------------------------- dictionaries
@pytest.mark.parametrize("ndict", code_cases.NDICTS)
def test_every_dictionary_size_on_noise(ndict, mem):
    """random payloads against random dictionaries: at n = 3 every distance is tied many times over (the lowest id, then the lowest k), at n = 6 and 8 hardly any"""
    specs = [(ra.code_spec(n, 1, 1, contrast=8, max_border=3, max_hamming=n), noise_dictionary(n, ndict) if ndict else None) for n in (3, 6, 8)]
    check_specs(mem, ra.PIX_BGR, 44, 41, specs)
    if ndict >= 4096:
        want = ra.code_view(reference(ra.PIX_BGR, 44, 41, specs[0][0], specs[0][1])[0][[0, 2, 3]])
        assert (want["hamming"] == 0).all() and (want["second"] == 0).all(), "4096 draws of 512 payloads: every payload is there, and more than once"


def run_case(c, mem):
    plane, pstatus = gray_job(mem, ra.PIX_BGR, [c.frame], code_cases.IW, code_cases.IH, c.quads, c.pw, c.ph, 1)
    rect = ra.Rectifier(c.pw, c.ph, max_quads=1, njobs=1, code=c.spec, dictionary=c.dictionary)
    try:
        got, status = run_job(rect, mem, ra.PIX_BGR, [c.frame], code_cases.IW, code_cases.IH, c.quads)
    finally:
        rect.close()
    want, wstatus = code.records(c.frame, c.quads, c.pw, c.ph, c.spec, c.dictionary)
    localise(got, status, plane, want, wstatus, c.spec, c.dictionary, c.name)
    rec = ra.code_view(got)[0]
    for f, v in c.claims.items():      # known without the restatement
        assert int(rec[f]) == v, (c.name, f, int(rec[f]), v)


@pytest.mark.parametrize("c", code_cases.position_cases(), ids=repr)
def test_the_true_code_at_every_position_of_every_dictionary_size(c, mem):
    run_case(c, mem)


@pytest.mark.parametrize("c", code_cases.tie_and_limit_cases(), ids=repr)
def test_ties_and_limits(c, mem):
    run_case(c, mem)


@pytest.mark.parametrize("c", code_cases.shape_cases(), ids=repr)
def test_rendered_codes_of_every_shape_read_their_own_bits(c, mem):
    run_case(c, mem)


def test_contrast_at_and_one_past_what_noise_has(mem):
    pw, ph = 44, 41
    base = ra.code_spec(6, 1, 1, contrast=0, max_border=28)
    rec = ra.code_view(reference(ra.PIX_BGR, pw, ph, base)[0])[0]
    c = (int(rec["hi"]) - int(rec["lo"])) // 256
    assert 0 < c < 255
    specs = [(ra.code_spec(6, 1, 1, contrast=v, max_border=28), None) for v in (c, c + 1)]
    check_specs(mem, ra.PIX_BGR, pw, ph, specs)
    oks = [int(ra.code_view(reference(ra.PIX_BGR, pw, ph, s)[0])[0]["ok"]) for s, _ in specs]
    assert oks == [1, 0]


# ---------------------------------------------------------------------------------------------- formats, frame kinds, output kinds
@pytest.mark.parametrize("fmt", pixfmt.FORMATS, ids=[ra.PIX_NAMES[f] for f in pixfmt.FORMATS])
def test_every_format_frame_kind_and_output_kind(fmt, mem):
    kinds = [(kind, out_kind, 13 if kind == "device" else 0) for kind in ("host", "device", "pinned") for out_kind in ("device", "pinned")]
    n = 3 + fmt
    check_specs(mem, fmt, 65, 49, [(ra.code_spec(n, 1 + fmt % 2, 2, oversample=2, contrast=8, max_hamming=n), noise_dictionary(n, 100))], kinds)


# ---------------------------------------------------------------------------------------------- reuse, jobs in flight, empty and full jobs, argument errors
POLL_DICT = noise_dictionary(6, 300)


def test_the_same_output_reused_by_consecutive_jobs(mem):
    pw, ph = 65, 33
    spec = ra.code_spec(6, 1, 2, max_hamming=8)
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    for out_kind in ("device", "pinned"):
        rect = ra.Rectifier(pw, ph, max_quads=4, njobs=2, code=spec, dictionary=POLL_DICT)
        out = Out(mem, out_kind, 4 * rect.patch_bytes)
        try:
            for rnd, sel in enumerate(([0, 1, 2, 3], [0, 1, 2, 3], [2, 0], [1], [3, 2, 0])):      # (a shorter job leaves the rest of the buffer as the job before left it)
                got, status = run_job(rect, mem, ra.PIX_BGR, planes, iw, ih, quads[sel], out_kind=out_kind, out=out)
                want, wstatus = reference(ra.PIX_BGR, pw, ph, spec, POLL_DICT, sel)
                code.assert_records(got, status, want, wstatus, "%s output, job %d" % (out_kind, rnd))
                after = out.fetch()
                assert rnd == 0 or np.array_equal(after[got.size:], before[got.size:]), "job %d wrote behind its last byte" % rnd
                before = after
        finally:
            rect.close()


def test_four_jobs_in_flight_over_two_rounds_into_the_same_outputs(mem):
    pw, ph, njobs = 65, 33, 4
    spec = ra.code_spec(6, 1, 2, oversample=2, max_hamming=8)
    rect = ra.Rectifier(pw, ph, max_quads=4, njobs=njobs, code=spec, dictionary=POLL_DICT)
    outs = [Out(mem, "device" if k % 2 == 0 else "pinned", 4 * rect.patch_bytes) for k in range(njobs)]
    try:
        for rnd in range(2):      # (the second round reuses every slot's G plane, every staging buffer and every output)
            pending = []
            for k in range(njobs):
                iw, ih, planes, bgr, quads = case(ra.PIX_BGR, seed=k)
                sel = list(range(4))[k % 2:4 - k // 2] if rnd else list(range(4))
                args, pitches, kw = mem.place("device", planes, 5)
                assert rect.enqueue(ra.PIX_BGR, args, pitches, iw, ih, quads[sel], outs[k].ptr, out_pinned=k % 2 == 1, **kw) == rnd * njobs + k
                pending.append((k, sel))
            for k, sel in pending:
                status = rect.wait()
                want, wstatus = reference(ra.PIX_BGR, pw, ph, spec, POLL_DICT, sel, seed=k)
                code.assert_records(outs[k].fetch()[:len(sel) * rect.patch_bytes].reshape(rect.shape(len(sel))), status, want, wstatus, "round %d job %d" % (rnd, k))
        with pytest.raises(RuntimeError):
            rect.wait()      # nothing in flight
    finally:
        rect.close()


def test_empty_job_and_full_job_of_64_quads(mem):
    """n = 0; n = max_quads = 64 quads of 5 x 5 - one pixel per cell, 64 blocks; one quad too many"""
    iw, ih, planes, bgr, quads4 = case(ra.PIX_RGBA)
    rng = np.random.default_rng(41)
    base = np.array([(0.0, 0.0), (30.0, 2.0), (28.0, 26.0), (-3.0, 22.0)])
    quads = np.array([base + rng.uniform(0, 60, 2) * (1.0, 0.5) + rng.uniform(-2, 2, (4, 2)) for _ in range(64)])
    quads[17] = quads4[1]      # an invalid one
    pw = ph = 5
    spec = ra.code_spec(3, 1, 0, oversample=4, contrast=4, max_hamming=1)
    d = noise_dictionary(3, 64)
    want, wstatus = code.records(bgr, quads, pw, ph, spec, d)
    assert wstatus.sum() == 63 and not wstatus[17]
    rect = ra.Rectifier(pw, ph, max_quads=64, njobs=2, code=spec, dictionary=d)
    try:
        got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.zeros((0, 4, 2)))      # n = 0: nothing written, nothing returned
        assert got.shape == (0, 48) and len(status) == 0
        assert rect.enqueue(ra.PIX_RGBA, planes, None, iw, ih, np.zeros((0, 8)), None) == 1      # (no output buffer needed either)
        assert len(rect.wait()) == 0
        plane, pstatus = gray_job(mem, ra.PIX_RGBA, planes, iw, ih, quads, pw, ph, 4)
        for kind, out_kind in (("device", "device"), ("host", "pinned")):
            got, status = run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, quads, kind, out_kind)      # n = max_quads
            localise(got, status, plane, want, wstatus, spec, d, "full job, %s output" % out_kind)
        with pytest.raises(ValueError):
            run_job(rect, mem, ra.PIX_RGBA, planes, iw, ih, np.concatenate([quads, quads[:1]]))      # one more
        conv = rect.rectify(bgr, quads[:5])      # the convenience call
        code.assert_records(conv, wstatus[:5], want[:5], wstatus[:5], "rectify()")
        assert ra.code_view(conv).shape == (5,) and (ra.code_view(conv)["reserved"] == 0).all()
    finally:
        rect.close()


def test_argument_errors_return_minus_one_and_the_next_job_is_correct(mem):
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = 65, 33
    spec = ra.code_spec(6, 1, 2, oversample=2, max_hamming=8)
    d = np.array(POLL_DICT)
    want, wstatus = reference(ra.PIX_BGR, pw, ph, spec, d)
    create = lambda *a: L().rd_rectifier_create_code(*a)
    assert not create(0, pw, ph, 4, 1, None, d.ctypes.data, len(d))      # a NULL spec
    for field, v in (("n", 2), ("n", 9), ("border", 0), ("border", 3), ("inset", -1), ("inset", 4), ("polarity", 2), ("polarity", -1), ("oversample", 3), ("oversample", 0), ("contrast", -1),
                     ("contrast", 256), ("max_border", -1), ("max_border", 29), ("max_hamming", -1), ("max_hamming", 37)):
        bad = spec.copy()
        bad[field] = v
        assert not create(0, pw, ph, 4, 1, bad.ctypes.data, d.ctypes.data, len(d)), field
        with pytest.raises(ValueError):
            ra.Rectifier(pw, ph, code=bad, dictionary=d)
    for other in (dict(tensor=ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_GRAY, 2)), dict(scan=ra.scan_spec(ra.SCAN_FLAT)), dict(grade=ra.grade_spec())):
        with pytest.raises(ValueError):
            ra.Rectifier(pw, ph, code=spec, **other)      # one or the other
    with pytest.raises(ValueError):
        ra.Rectifier(pw, ph, dictionary=d)      # a dictionary without a code spec
    for args in ((0, 0, ph, 4, 1), (0, pw, 0, 4, 1), (0, 31, ph, 4, 1), (0, pw, 31, 4, 1), (0, 1025, ph, 4, 1), (0, pw, 1025, 4, 1), (0, pw, ph, 0, 1), (0, pw, ph, 4, 0), (99, pw, ph, 4, 1)):
        assert not create(*args, spec.ctypes.data, d.ctypes.data, len(d)), args      # rd_rectifier_create's bad arguments (pw < 4C and pw > 1024 among them)
    big = np.zeros(4097, np.uint64)
    high = d.copy()
    high[len(d) - 1] = 1 << 36
    for dp, nd in ((None, 1), (d.ctypes.data, -1), (big.ctypes.data, 4097), (high.ctypes.data, len(high))):
        assert not create(0, pw, ph, 4, 1, spec.ctypes.data, dp, nd), nd      # a NULL dictionary with entries, ndict out of range, bits at or above n * n
    h = create(0, pw, ph, 4, 1, spec.ctypes.data, None, 0)      # no dictionary at all is legal
    assert h and L().rd_rectifier_patch_bytes(h) == 48
    L().rd_rectifier_destroy(h)
    rect = ra.Rectifier(pw, ph, max_quads=len(quads), njobs=1, code=spec, dictionary=d)
    out = Out(mem, "device", len(quads) * rect.patch_bytes + 8)
    pinned = mem.out("pinned", len(quads) * rect.patch_bytes + 8)
    try:
        q = rectjobs.refused_enqueues(mem, rect, planes, iw, ih, quads, out, {"out misaligned by 4": dict(out_p=out.ptr + 4), "out misaligned by 1": dict(out_p=out.ptr + 1),
                                                                               "pinned out misaligned by 4": dict(out_p=pinned + 4, out_kind=2)})
        status = rect.wait()
        code.assert_records(out.fetch()[:len(q) * rect.patch_bytes].reshape(rect.shape(len(q))), status, want, wstatus, "the job after the refused ones")
        assert (out.fetch()[len(q) * rect.patch_bytes:] == 0xA5).all()
    finally:
        rect.close()


# ---------------------------------------------------------------------------------------------- behind the detector's poll
POLL_SPEC = ra.code_spec(6, 1, 2, oversample=2, contrast=8, max_border=2, max_hamming=10)


@pytest.mark.parametrize("kind", ["rect-host", "rect-device", "poly-host", "poly-device", "scaled"])
def test_rectify_polled_behind_every_poll(kind, mem):
    """after Detector.poll and PolylineDetector.poll, on host frames (the detector's own copy) and device frames, and on a frame that came in at scale 2 - quads in
    detector coordinates, the records from the full-size source (X = 2x + 0.5)"""
    rectjobs.polled_behind_a_poll(mem, kind, dict(code=POLL_SPEC, dictionary=POLL_DICT), lambda bgr, quads: code.records(bgr, quads, rectjobs.PW, rectjobs.PH, POLL_SPEC, POLL_DICT),
                                  lambda got, status, plane, want, wstatus, what: localise(got, status, plane, want, wstatus, POLL_SPEC, POLL_DICT, what), beside=dict(tensor=code.gray_spec(POLL_SPEC)),
                                  misaligned_refused=True, out_reused=True)


# ---------------------------------------------------------------------------------------------- memory that torch allocated
TORCH_CHILD = """
import sys
import torch                      # first: the process then holds ONE HIP runtime, torch's (INTEGRATION.md, section 3)
import numpy as np
import rectdetect_amd as ra
d = np.load(sys.argv[1])
frame, quads, pw, ph, dictionary = d["frame"], d["quads"], int(d["pw"]), int(d["ph"]), d["dictionary"]
ih, iw, n = frame.shape[0], frame.shape[1], len(quads)
dframe = ra.lib().rd_device_alloc(frame.nbytes)
ra.lib().rd_upload(dframe, frame.ctypes.data, frame.nbytes)
for name, dic in (("raw", None), ("dict", dictionary)):
    rect = ra.Rectifier(pw, ph, max_quads=n, njobs=1, code=ra.code_spec(6, 1, 2, oversample=2, max_hamming=8), dictionary=dic)
    t = torch.empty(rect.shape(n), dtype=torch.uint8, device="cuda")
    assert rect.patch_bytes * n == t.numel() and t.data_ptr() % 8 == 0
    t.fill_(7)
    torch.cuda.synchronize()      # the caller's own streams are done with the memory before the enqueue
    rect.enqueue(ra.PIX_BGR, (dframe,), (iw * 3,), iw, ih, quads, t.data_ptr(), on_device=True)
    status = rect.wait()          # after which the data is visible to every stream
    np.save(sys.argv[2] + name + ".npy", t.cpu().numpy())
    np.save(sys.argv[2] + name + "_status.npy", status)
    print(name, "sum", int(t.sum().item()), flush=True)      # a torch op on the tensor afterwards
    rect.close()
ra.lib().rd_device_free(dframe)
print("done", flush=True)
"""


def test_torch_tensors_are_written_through_data_ptr(tmp_path):
    """torch.uint8 tensors of records, with and without a dictionary, allocated by torch on the device and written through data_ptr(), read back with t.cpu(): the
    restatement's bytes.  In a child process, because what is tested is a process that imports torch first and so holds one HIP runtime."""
    iw, ih, planes, bgr, quads = case(ra.PIX_BGR)
    pw, ph = 65, 33
    dictionaries = {"raw": None, "dict": POLL_DICT}
    child = rectjobs.torch_child(tmp_path, TORCH_CHILD, dictionaries, frame=bgr, quads=quads, pw=pw, ph=ph, dictionary=np.array(POLL_DICT))
    spec = ra.code_spec(6, 1, 2, oversample=2, max_hamming=8)
    for name, dic in dictionaries.items():
        want, wstatus = reference(ra.PIX_BGR, pw, ph, spec, dic)
        got, status, total = child[name]
        code.assert_records(got, status, want, wstatus, name)
        assert int(total) == int(want.astype(np.int64).sum()), "torch summed the bytes the job wrote"


# ---------------------------------------------------------------------------------------------- the example program
def test_rdcodes_prints_the_records_of_the_restatement(tmp_path):
    """examples/rdcodes writes the frame it made: the rectangles the detector finds in it, read by the restatement with the same dictionary, are the lines it
    prints; the four codes of the frame are among them with their ids, each as many quarter turns off as it was drawn - whichever corner the detector starts at,
    the upright quad's first corner is the code's own top-left"""
    side = 64
    res = subprocess.run([os.path.join(helpers.ROOT, "examples", "rdcodes"), "0", str(tmp_path / "frame.ppm"), str(side)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path, timeout=60)
    assert res.returncode == 0, res.stderr.decode()
    text = res.stdout.decode()
    raw = open(tmp_path / "frame.ppm", "rb").read()
    assert raw.startswith(b"P6\n640 480\n255\n")
    img = np.ascontiguousarray(np.frombuffer(raw[len(b"P6\n640 480\n255\n"):], np.uint8).reshape(480, 640, 3)[..., ::-1])
    D = ra.code_dictionary(6, 50, 9, seed=1, tries=1 << 20)
    assert len(D) == 50 and ("dictionary 50 codes of 6 x 6 distance %d\n" % ra.code_distance(D, 6)) in text
    ctx = ra.Context(0)
    det = ra.RectDetector(ctx, 640, 480)
    rects = det.execute_once(img, np.tan(72.0 / 2 / 180.0 * np.pi))
    det.close()
    ctx.close()
    n = len(rects)
    assert n > 0 and ("%d rectangle(s)" % n) in text
    spec = ra.code_spec(6, 1, 2, 0, 1, 32, 0, 2)
    quads = ra.rect_quads(rects)
    want, st = code.records(img, quads, side, side, spec, D)
    recs = ra.code_view(want)
    found = {}
    for k in range(n):
        r = recs[k]
        line = "rect %d status %d : id %d rot %d hamming %d second %d border_errors %d lo %d hi %d margin %d ok %d bits %016x" % (
            k, rects[k]["status"], r["id"], r["rot"], r["hamming"], r["second"], r["border_errors"], r["lo"], r["hi"], r["margin"], r["ok"], int(r["bits"]))
        assert line in text, line
        up = ra.code_upright(quads[k], int(r["rot"])).reshape(8)
        line = "  rect %d upright : %s\n" % (k, "  ".join("%.17g %.17g" % (up[2 * c], up[2 * c + 1]) for c in range(4)))
        assert line in text, line
        if int(r["ok"]):
            found[int(r["id"])] = up.reshape(4, 2)
    placed = {3: (60, 50, 96, 0), 17: (330, 40, 128, 1), 29: (90, 300, 80, 2), 41: (400, 270, 112, 3)}      # id: x, y, side, quarter turns off
    assert sorted(found) == sorted(placed), (sorted(found), text)
    for i, (x, y, s, k) in placed.items():
        corners = np.array([(x, y), (x + s, y), (x + s, y + s), (x, y + s)], np.float64) - 0.5
        nearest = int(np.argmin(((corners - found[i][0]) ** 2).sum(1)))
        assert nearest == (4 - k) % 4, "the corner of the drawn square where the code's own top-left is: %r" % ((i, found[i], corners),)


# ---------------------------------------------------------------------------------------------- device only: the compositor writes a code, the decoder reads it
def test_a_code_the_compositor_pasted_is_read_back_from_the_device_frame(mem):
    """one device frame, never on the host in between: the compositor pastes rd_code_render's image into a quad in perspective (in place), the code rectifier reads
    that quad from the same memory.  Expected bytes: tests/composite.py, then tests/code.py"""
    iw, ih, planes, bgr, _ = case(ra.PIX_BGR)
    D = code_cases.big_dictionary()[:300]
    spec = ra.code_spec(6, 1, 2, oversample=2, contrast=64, max_hamming=2)
    img = ra.code_render(spec, ra.code_rotate(int(D[77]), 6, 3), 8)      # 64 x 64, shown a quarter turn off
    patch = np.repeat(img[..., None], 3, axis=2)[None]
    quad = np.array([[(14.0, 6.5), (80.5, 10.0), (76.0, 56.0), (9.5, 50.25)]])
    items = ra.comp_items(quad, patch=0)
    (dframe,), (pitch,), kw = mem.place("device", planes, 7)
    comp = ra.Compositor(64, 64, max_items=4, njobs=1)
    rect = ra.Rectifier(48, 48, max_quads=1, njobs=1, code=spec, dictionary=D)
    try:
        comp.enqueue(ra.PIX_BGR, (dframe,), (pitch,), iw, ih, items, patches=patch, **kw)
        assert comp.wait().tolist() == [1]
        out = Out(mem, "device", 48)
        rect.enqueue(ra.PIX_BGR, (dframe,), (pitch,), iw, ih, quad, out.ptr, **kw)
        status = rect.wait()
        got = out.fetch().reshape(1, 48)
    finally:
        comp.close()
        rect.close()
    drawn, cstatus = composite.draw(ra.PIX_BGR, [np.ascontiguousarray(bgr).reshape(ih, iw * 3)], iw, ih, items, patch)
    want, wstatus = code.records(drawn[0].reshape(ih, iw, 3), quad, 48, 48, spec, D)
    code.assert_records(got, status, want, wstatus, "composited, then decoded")
    rec = ra.code_view(got)[0]
    assert (int(rec["id"]), int(rec["rot"]), int(rec["hamming"]), int(rec["ok"])) == (77, 1, 0, 1), rec
