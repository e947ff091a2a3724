"""Model-ready tensors for the tests: the contract of include/rectdetect_hip.h ("model-ready tensors") restated in numpy, written from the header's text and not from
the kernel - tests/rectify.py's patch at (pw*m) x (ph*m), the channel values, int64 box sums, np.float32 operations one at a time, astype(np.float16), and the
bfloat16 bit formula on the uint32 view.  Frames in the other pixel formats go through tests/rectify.contract_bgr first."""
import numpy as np

import rectdetect_amd as ra
from tests import rectify

DTYPES = (ra.TENSOR_U8, ra.TENSOR_F16, ra.TENSOR_BF16, ra.TENSOR_F32)
LAYOUTS = (ra.TENSOR_NHWC, ra.TENSOR_NCHW)
CHANNELS = (ra.TENSOR_BGR, ra.TENSOR_RGB, ra.TENSOR_GRAY)
OVERSAMPLINGS = (1, 2, 4)
DTYPE_NAMES = {ra.TENSOR_U8: "u8", ra.TENSOR_F16: "f16", ra.TENSOR_BF16: "bf16", ra.TENSOR_F32: "f32"}
LAYOUT_NAMES = {ra.TENSOR_NHWC: "nhwc", ra.TENSOR_NCHW: "nchw"}
CHANNEL_NAMES = {ra.TENSOR_BGR: "bgr", ra.TENSOR_RGB: "rgb", ra.TENSOR_GRAY: "gray"}


def name(spec):
    return "%s-%s-%s-m%d" % (DTYPE_NAMES[int(spec["dtype"])], LAYOUT_NAMES[int(spec["layout"])], CHANNEL_NAMES[int(spec["channels"])], int(spec["oversample"]))


def nchannels(spec):
    return 1 if int(spec["channels"]) == ra.TENSOR_GRAY else 3


def numpy_dtype(spec):
    """bfloat16 as its bits"""
    return {ra.TENSOR_U8: np.uint8, ra.TENSOR_F16: np.float16, ra.TENSOR_BF16: np.uint16, ra.TENSOR_F32: np.float32}[int(spec["dtype"])]


def f32_value(S, m, scale, bias):
    """step 4's v: (float)S * (1.0f/(m*m)), times scale, plus bias - binary32, one rounded operation after the other"""
    with np.errstate(all="ignore"):
        v = np.asarray(S, np.int64).astype(np.float32) * (np.float32(1.0) / np.float32(m * m))
        v = v * np.float32(scale)
        v = v + np.float32(bias)
    return v.astype(np.float32)


def bf16_bits(v):
    """the upper 16 bits of u + 0x7FFF + ((u >> 16) & 1), u the bits of the binary32 values v"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16).astype(np.uint16)


def elements(spec, c, S):
    """step 4 for an array of box sums of output channel c: an array of numpy_dtype(spec)"""
    m, dt = int(spec["oversample"]), int(spec["dtype"])
    S = np.asarray(S, np.int64)
    if dt == ra.TENSOR_U8:
        return ((S + (m * m) // 2) >> {1: 0, 2: 2, 4: 4}[m]).astype(np.uint8)
    v = f32_value(S, m, spec["scale"][c], spec["bias"][c])
    if dt == ra.TENSOR_F32:
        return v
    if dt == ra.TENSOR_F16:
        with np.errstate(all="ignore"):
            return v.astype(np.float16)
    return bf16_bits(v)


def box_sums(patch, spec, pw, ph):
    """steps 2 and 3: the (ph, pw, C) int64 sums S of a (ph*m, pw*m, 3) BGR patch, in OUTPUT channel order"""
    m, ch = int(spec["oversample"]), int(spec["channels"])
    p = patch.astype(np.int64)
    if ch == ra.TENSOR_BGR:
        v = p
    elif ch == ra.TENSOR_RGB:
        v = p[..., ::-1]
    else:
        v = ((29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8)[..., None]
    return v.reshape(ph, m, pw, m, v.shape[-1]).sum(axis=(1, 3))


def shape(spec, n, pw, ph):
    C = nchannels(spec)
    return (n, C, ph, pw) if int(spec["layout"]) == ra.TENSOR_NCHW else (n, ph, pw, C)


def tensors(bgr, quads, pw, ph, spec):
    """(the array of shape(spec, n, pw, ph) and numpy_dtype(spec) of n quads of an (ih, iw, 3) BGR image - zero BYTES for an invalid quad -, uint8 status[n])"""
    m = int(spec["oversample"])
    q = np.asarray(quads, np.float64).reshape(-1, 8)
    out, st = np.zeros(shape(spec, len(q), pw, ph), numpy_dtype(spec)), np.zeros(len(q), np.uint8)
    for k in range(len(q)):
        patch, st[k] = rectify.patch(bgr, q[k], pw * m, ph * m)
        if not st[k]:
            continue
        S = box_sums(patch, spec, pw, ph)
        for c in range(S.shape[-1]):
            e = elements(spec, c, S[..., c])
            if int(spec["layout"]) == ra.TENSOR_NCHW:
                out[k, c] = e
            else:
                out[k, :, :, c] = e
    return out, st


def assert_tensors(got, status, want, wstatus, what=""):
    """bit equality, whatever the dtype (a float array is compared by its bytes: -0.0 is not 0.0, an infinity is an infinity)"""
    assert np.array_equal(status, wstatus), "%s: status %r, expected %r" % (what, np.asarray(status).tolist(), np.asarray(wstatus).tolist())
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %r %r, expected %r %r" % (what, got.shape, got.dtype, want.shape, want.dtype)
    g, w = np.ascontiguousarray(got).view(np.uint8).reshape(len(want), -1), np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)
    bad = [k for k in range(len(want)) if not np.array_equal(g[k], w[k])]
    assert not bad, "%s: quads %r differ (quad %d in %d bytes, first at byte %d)" % (what, bad[:10], bad[0], int((g[bad[0]] != w[bad[0]]).sum()), int(np.nonzero(g[bad[0]] != w[bad[0]])[0][0]))
