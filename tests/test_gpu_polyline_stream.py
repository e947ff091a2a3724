"""The polyline kind of rd_detector (rd_polyline_detector_create / rd_detector_poll_segments, rectdetect_amd.PolylineDetector): poly.cpp /
vidpoly.cpp per frame with frames in flight.  Against the reference's own lists (tests/golden/poly_*.npz, polystream_*.npz from
tools/make_golden_polystreams.py) and against the operator path (rectdetect_amd.poly_frame) frame by frame."""
import ctypes
import glob
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

import rectdetect_amd as ra
from rectdetect_amd import synth
from tests import helpers

TAN36 = float(np.tan(36.0 / 180.0 * np.pi))
VID, POLY = (2000, 1.0, 10), (500, 1.0, 20)
STREAM_GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(helpers.GOLDEN, "polystream_*.npz")))


def golden(name):
    return np.load(os.path.join(helpers.GOLDEN, name + ".npz"))


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def params(g):
    return int(g["strength_thre"]), float(g["minerror"]), int(g["size_thre"])


def stream_frames(g):
    """(input, reference segment list, CRC of the reference's id plane) of every frame of a polystream golden"""
    iw, ih = int(g["iw"]), int(g["ih"])
    offs = g["offsets"]
    for i, (kind, seed, t) in enumerate(zip(g["kinds"], g["seeds"], g["ts"])):
        img = synth.frame(int(seed), iw, ih, int(t)) if str(kind) == "frame" else synth.hard_frame(str(kind), int(seed), iw, ih)
        assert crc(img) == int(g["input_crc"][i])
        yield img, g["segments"][offs[i]:offs[i + 1]], int(g["ids_crc"][i])


def run(det, frames, pattern="window", ids_every=0, enqueue=None):
    """every frame through the detector, polled in sequence order: 'each' = poll after every enqueue, 'fill' = fill all slots, then poll them all,
    'window' = keep the slots full (poll the oldest once they are); ids requested on every ids_every-th frame.  Returns [(segments, ids or None)]."""
    enqueue = enqueue or (lambda i, f: det.enqueue(f))
    nslots = det.nslots
    out, inflight = [], 0
    for i, f in enumerate(frames):
        if pattern == "fill" and inflight == nslots or pattern == "window" and inflight == nslots:
            while inflight:
                k = len(out)
                out.append(det.poll(ids=bool(ids_every) and k % ids_every == 0))
                inflight -= 1
                if pattern == "window":
                    break
        enqueue(i, f)
        inflight += 1
        if pattern == "each":
            out.append(det.poll(ids=bool(ids_every) and i % ids_every == 0))
            inflight -= 1
    while inflight:
        k = len(out)
        out.append(det.poll(ids=bool(ids_every) and k % ids_every == 0))
        inflight -= 1
    return out


def detector(iw, ih, nslots, p, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        det = ra.PolylineDetector(iw, ih, nslots=nslots, strength_thre=p[0], minerror=p[1], size_thre=p[2])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    det.nslots = nslots
    return det


@pytest.fixture(scope="module")
def ctx():
    c = ra.Context(0)
    yield c
    c.close()


# ---- arguments (no GPU needed: the arguments are checked before the device is looked at)
@pytest.mark.parametrize("args", [dict(iw=0), dict(iw=-5), dict(ih=0), dict(nslots=0), dict(minerror=0.0), dict(minerror=-1.0), dict(size_thre=-1), dict(strength_thre=-1)],
                         ids=lambda a: "-".join("%s=%s" % kv for kv in a.items()))
def test_invalid_arguments_return_null(args):
    a = dict(device=0, iw=640, ih=480, nslots=4, strength_thre=500, minerror=1.0, size_thre=20)
    a.update(args)
    L = ra.lib()
    assert L.rd_polyline_detector_create(a["device"], a["iw"], a["ih"], a["nslots"], a["strength_thre"], a["minerror"], a["size_thre"]) is None
    with pytest.raises(ValueError):
        ra.PolylineDetector(a["iw"], a["ih"], device=a["device"], nslots=a["nslots"], strength_thre=a["strength_thre"], minerror=a["minerror"], size_thre=a["size_thre"])


# ---- 1. the reference's single-frame goldens
@pytest.mark.gpu
@pytest.mark.parametrize("nslots", [1, 8])
@pytest.mark.parametrize("name", ["poly_640x480_s0", "poly_333x217_s2", "poly_1280x720_s1_vid"])
def test_single_frame_goldens(name, nslots):
    g = golden(name)
    iw, ih = int(g["iw"]), int(g["ih"])
    img = synth.frame(int(g["seed"]), iw, ih, 0)
    det = detector(iw, ih, nslots, params(g))
    det.enqueue(img)
    segs, ids = det.poll(ids=True)
    det.close()
    assert helpers.segments_equal(segs, g["segments"])
    assert crc(ids) == int(g["ids_crc"])


# ---- 2. the reference's streams, every frame
@pytest.mark.gpu
@pytest.mark.parametrize("name,nslots", [(n, k) for n in STREAM_GOLDENS for k in (1, 2, 8, 64) if not ("3840x2160" in n and k > 8)])      # (the 8-frame 3840x2160 stream: 64 slots would be 64 x 2 GB for 8 frames)
def test_stream_goldens(ctx, name, nslots):
    """every frame the reference's list (valid records bit-identical, same count) and id plane - the frames with orphan records included (frame 53 of the
    1280x720 stream, frame 3 of the 3840x2160 one: tests/polycases.py), on which the end-point join once departed from the reference's ascending order"""
    g = golden(name)
    iw, ih = int(g["iw"]), int(g["ih"])
    data = list(stream_frames(g))
    det = detector(iw, ih, nslots, params(g))
    got = run(det, [d[0] for d in data], "window", ids_every=8)
    print(name, "nslots", nslots, "frames per group launch", det.counter(15), "multi-launch repeats", det.counter(0), "long lists", det.counter(30))
    det.close()
    whole = 0
    for i, ((segs, ids), (img, want, ids_crc)) in enumerate(zip(got, data)):
        if i % 8 != 0:
            assert ids is None
        assert helpers.segments_equal(segs, want), f"{name} frame {i}: {int(segs.view('i4')[0])} records, reference {int(want.view('i4')[0])}"
        whole += segs.tobytes() == want.tobytes()
        if i % 8 == 0:
            assert crc(ids) == ids_crc, f"{name} frame {i}: id plane"
    print(name, "lists identical in every byte, records with polyid == 0 included:", whole, "of", len(data))


# ---- 3. shapes: groups, polling patterns, frame kinds - against the operator path frame by frame
@pytest.fixture(scope="module")
def small_stream(ctx):
    iw, ih = 640, 480
    frames = [synth.frame(synth.SEED0 + 9, iw, ih, t) for t in range(20)]
    return iw, ih, frames, [ra.poly_frame(ctx, f, *VID) for f in frames]


@pytest.mark.gpu
@pytest.mark.parametrize("nslots,pattern,kind", [(1, "each", "host"), (3, "window", "host"), (7, "fill", "pinned"), (7, "window", "device"), (13, "each", "device"),
                                                 (13, "window", "host"), (13, "fill", "host"), (32, "window", "pinned"), (37, "fill", "device"), (64, "window", "host")])
def test_shapes_equal_operator_path(small_stream, nslots, pattern, kind):
    iw, ih, frames, want = small_stream
    L = ra.lib()
    det = detector(iw, ih, nslots, VID)
    bufs = []
    if kind == "host":
        enq = None
    else:
        nb = iw * ih * 3
        alloc, free = (L.rd_device_alloc, L.rd_device_free) if kind == "device" else (L.rd_host_alloc, L.rd_host_free)
        bufs = [(alloc(nb), free) for _ in range(len(frames))]      # (one buffer per frame: each stays unchanged until its poll)
        for (p, _), f in zip(bufs, frames):
            if kind == "device":
                L.rd_upload(p, f.ctypes.data, nb)
            else:
                ctypes.memmove(p, f.ctypes.data, nb)
        enq = lambda i, f: det.enqueue(bufs[i][0], ws=iw * 3, on_device=kind == "device", pinned=kind == "pinned")
    got = run(det, frames, pattern, ids_every=5, enqueue=enq)
    zb = det.counter(15)
    if kind == "pinned":
        assert det.counter(18) == len(frames)
    det.close()
    for p, free in bufs:
        free(p)
    print("nslots", nslots, "frames per group launch", zb)
    assert zb == (8 if nslots >= 32 else 4 if nslots >= 12 else 2 if nslots >= 6 else 1)
    for i, ((segs, ids), (wsegs, wids)) in enumerate(zip(got, want)):
        assert helpers.segments_equal(segs, wsegs), f"frame {i}"
        if ids is not None:
            assert np.array_equal(ids, wids), f"frame {i}: id plane"


# ---- 4. overflow of the single-block kernel, lists longer than the hand-off block
@pytest.mark.gpu
def test_hard_frames_overflow_and_long_lists():
    """dense chains: frames beyond the single-block kernel's on-chip tables (repeated in multi-launch form, counter 0) and lists longer than the
    2048 records handed off (fetched by the poll, counter 30) - nothing dropped, every list the reference's"""
    g = golden("polystream_1920x1080_hard_vid")
    data = list(stream_frames(g))
    det = detector(int(g["iw"]), int(g["ih"]), 4, params(g))
    got = run(det, [d[0] for d in data], "fill", ids_every=1)
    redo, longl = det.counter(0), det.counter(30)
    det.close()
    print("multi-launch repeats", redo, "long lists", longl, "records", [int(s.view("i4")[0]) for s, _ in got])
    assert redo > 0 and longl > 0
    for (segs, ids), (_, want, ids_crc) in zip(got, data):
        assert helpers.segments_equal(segs, want) and crc(ids) == ids_crc


@pytest.mark.gpu
@pytest.mark.parametrize("env,counter", [({"RD_POLY_MULTILAUNCH": "1"}, None), ({"RD_POLY_FORCE_REDO": "1"}, 0), ({"RD_POLY_HANDOFF": "16"}, 30),
                                         ({"RD_NO_GRAPH": "1"}, None), ({"RD_ZBATCH": "3"}, None)], ids=lambda v: str(v))
def test_hooks_change_nothing(small_stream, env, counter):
    iw, ih, frames, want = small_stream
    det = detector(iw, ih, 12, VID, env)
    got = run(det, frames, "window", ids_every=3)
    c = det.counter(counter) if counter is not None else None
    if "RD_ZBATCH" in env:
        assert det.counter(15) == 3
    det.close()
    if counter is not None:
        print(env, "counter", counter, "=", c)
        assert c == len(frames) if counter == 0 else c > 0
    for i, ((segs, ids), (wsegs, wids)) in enumerate(zip(got, want)):
        assert helpers.segments_equal(segs, wsegs), f"frame {i}"
        if ids is not None:
            assert np.array_equal(ids, wids)


# ---- 5. a rectangle and a polyline detector side by side
@pytest.mark.gpu
def test_rect_and_polyline_detectors_coexist(ctx):
    g = golden("rect_1280x720_s1")
    iw, ih = int(g["iw"]), int(g["ih"])
    frames = [synth.frame(int(g["seed"]), iw, ih, t) for t in range(int(g["nframes"]))]
    alone = ra.Detector(iw, ih, nslots=1)
    base = []
    for f in frames:
        alone.enqueue(f)
        base.append((alone.poll(TAN36), alone.last_segments()))
    alone.close()
    rect = ra.Detector(iw, ih, nslots=1)
    poly = detector(iw, ih, 8, POLY)
    for t, f in enumerate(frames):
        poly.enqueue(f)
        rect.enqueue(f)
        poly.enqueue(frames[-1 - t])
        rects, segs = rect.poll(TAN36), rect.last_segments()
        assert helpers.rects_equal(rects, base[t][0]) and helpers.segments_equal(segs, base[t][1])
        assert helpers.segments_equal(segs, g[f"f{t}_segments"])
        for want in (f, frames[-1 - t]):
            psegs, _ = poly.poll()
            assert helpers.segments_equal(psegs, ra.poly_frame(ctx, want, *POLY)[0])
    rect.close()
    poly.close()


# ---- 6. the wrong poll is refused (fatal, with a message) - in a child process
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["poll_on_polyline", "poll_segments_on_rect"])
def test_wrong_poll_is_refused(kind):
    code = ("import numpy as np, rectdetect_amd as ra\nfrom rectdetect_amd import synth\nL = ra.lib()\n"
            "img = synth.frame(synth.SEED0, 640, 480, 0)\n"
            + ("d = ra.PolylineDetector(640, 480, nslots=2)\nd.enqueue(img)\nL.rd_detector_poll(d.h, 0.5)\n" if kind == "poll_on_polyline" else
               "d = ra.Detector(640, 480, nslots=2)\nd.enqueue(img)\nL.rd_detector_poll_segments(d.h, None)\n")
            + "print('NOT REFUSED')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=helpers.ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode not in (0, -6, -11, 134, 139), (r.returncode, r.stderr)
    assert "NOT REFUSED" not in r.stdout
    want = "rd_detector_poll: this is a polyline detector" if kind == "poll_on_polyline" else "rd_detector_poll_segments: this is a rectangle detector"
    assert want in r.stderr, r.stderr


# ---- 7. rate, loose
@pytest.mark.gpu
def test_rate_against_operator_path(ctx):
    iw, ih, n = 1920, 1080, 32
    frames = [synth.frame(synth.SEED0 + 3, iw, ih, t) for t in range(n)]
    L = ra.lib()
    nb = iw * ih * 3
    dev = [L.rd_device_alloc(nb) for _ in frames]
    for p, f in zip(dev, frames):
        L.rd_upload(p, f.ctypes.data, nb)
    det = detector(iw, ih, 64, VID)
    for rep in range(2):      # (the first pass captures the graphs)
        t0 = time.perf_counter()
        for p in dev:
            det.enqueue(p, ws=iw * 3, on_device=True)
        segs = [det.poll()[0] for _ in dev]
        t_det = time.perf_counter() - t0
    det.close()
    for p in dev:
        L.rd_device_free(p)
    ra.poly_frame(ctx, frames[0], *VID)
    t0 = time.perf_counter()
    ops = [ra.poly_frame(ctx, f, *VID)[0] for f in frames]
    t_ops = time.perf_counter() - t0
    print("detector %.0f frames/s, operator path %.0f frames/s" % (n / t_det, n / t_ops))
    for a, b in zip(segs, ops):
        assert helpers.segments_equal(a, b)
    assert t_ops >= 2.0 * t_det


# ---- the example program
@pytest.mark.gpu
def test_vidpoly_example_matches_binding(tmp_path):
    iw, ih, n = 640, 480, 6
    exe = os.path.join(helpers.ROOT, "examples", "rdvidpoly")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(helpers.ROOT, "examples")], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe, "0", "%dx%d" % (iw, ih), str(n), "4"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("frame ")]
    det = detector(iw, ih, 4, VID)
    got = run(det, [synth.frame(synth.SEED0, iw, ih, t) for t in range(n)], "window")
    det.close()
    assert len(lines) == n
    for (segs, _), l in zip(got, lines):
        m = segs[1:][segs[1:]["polyid"] != 0]
        assert int(l[3]) == int(segs.view("i4")[0]) and int(l[5]) == len(m)
        assert int(l[7], 16) == crc(m.tobytes())
