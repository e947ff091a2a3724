"""Pixel formats of rd_detector_enqueue_planes for the tests: the conversion contract of include/rectdetect_hip.h restated in numpy (YUV -> BGR), a forward
BGR -> YUV that makes inputs (any 4:2:0 approximation will do: the detector is checked against the BGR frame the CONTRACT gives for those planes), and a
YUV4MPEG2 writer for examples/rdy4m."""
import numpy as np

import rectdetect_amd as ra

FORMATS = (ra.PIX_BGR, ra.PIX_RGB, ra.PIX_BGRA, ra.PIX_RGBA, ra.PIX_NV12, ra.PIX_I420)


def yuv2bgr(Y, U, V):
    """the contract, element-wise (int32, arithmetic shifts): uint8 arrays B, G, R"""
    Y, U, V = (np.asarray(a, np.int32) for a in (Y, U, V))
    u, v = U - 128, V - 128
    yy = np.maximum(Y - 16, 0) * 1220542
    R = np.clip((yy + 1673527 * v + (1 << 19)) >> 20, 0, 255)
    G = np.clip((yy - 852492 * v - 409993 * u + (1 << 19)) >> 20, 0, 255)
    B = np.clip((yy + 2116026 * u + (1 << 19)) >> 20, 0, 255)
    return B.astype(np.uint8), G.astype(np.uint8), R.astype(np.uint8)


def i420_to_bgr(Y, U, V):
    """HxWx3 BGR of I420 planes (2x2 nearest chroma)"""
    Uf = np.repeat(np.repeat(U, 2, 0), 2, 1)
    Vf = np.repeat(np.repeat(V, 2, 0), 2, 1)
    return np.ascontiguousarray(np.stack(yuv2bgr(Y, Uf, Vf), axis=-1))


def nv12_to_bgr(Y, UV):
    return i420_to_bgr(Y, UV[:, 0::2], UV[:, 1::2])


def bgr2yuv(b, g, r):
    """BGR -> YUV of the contract (rd_annot_yuv: BT.601 limited range) in numpy int32, arrays or scalars: (Y, U, V)"""
    b, g, r = (np.asarray(v).astype(np.int32) for v in (b, g, r))
    return ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128, ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128


def bgr_to_i420(bgr):
    """chroma averaged over 2x2 (even sizes): Y, U, V uint8 planes"""
    Y, U, V = bgr2yuv(bgr[..., 0], bgr[..., 1], bgr[..., 2])
    sub = lambda c: (c[0::2, 0::2] + c[1::2, 0::2] + c[0::2, 1::2] + c[1::2, 1::2] + 2) >> 2
    return tuple(np.clip(a, 0, 255).astype(np.uint8) for a in (Y, sub(U), sub(V)))


def convert(bgr, fmt):
    """(planes of `bgr` in format fmt, the BGR frame the detector must see for them)"""
    if fmt == ra.PIX_BGR:
        return (bgr,), bgr
    if fmt == ra.PIX_RGB:
        return (np.ascontiguousarray(bgr[..., ::-1]),), bgr
    if fmt in (ra.PIX_BGRA, ra.PIX_RGBA):
        c = bgr if fmt == ra.PIX_BGRA else bgr[..., ::-1]
        alpha = (np.arange(bgr.shape[1], dtype=np.uint32) * 7 % 256).astype(np.uint8)      # (ignored by the detector: anything but constant)
        return (np.ascontiguousarray(np.concatenate([c, np.broadcast_to(alpha[None, :, None], bgr.shape[:2] + (1,))], axis=-1)),), bgr
    Y, U, V = bgr_to_i420(bgr)
    if fmt == ra.PIX_I420:
        return (Y, U, V), i420_to_bgr(Y, U, V)
    UV = np.ascontiguousarray(np.stack([U, V], axis=-1).reshape(U.shape[0], -1))
    return (Y, UV), nv12_to_bgr(Y, UV)


def write_y4m(path, frames, iw, ih, tag="C420jpeg"):
    """frames: (Y, U, V) triples"""
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1%s\n" % (iw, ih, " " + tag if tag else "")).encode())
        for Y, U, V in frames:
            f.write(b"FRAME\n")
            for p in (Y, U, V):
                f.write(np.ascontiguousarray(p).tobytes())


def read_y4m(path):
    """(iw, ih, [(Y, U, V)]) of a 4:2:0 file, parsed the way examples/rdy4m.c does"""
    data = open(path, "rb").read()
    head, _, rest = data.partition(b"\n")
    tok = head.split()
    assert tok[0] == b"YUV4MPEG2"
    iw = int([t for t in tok if t.startswith(b"W")][0][1:])
    ih = int([t for t in tok if t.startswith(b"H")][0][1:])
    assert all(t.startswith(b"C420") for t in tok[1:] if t.startswith(b"C"))
    ny, nc = iw * ih, iw * ih // 4
    frames = []
    while rest:
        line, _, rest = rest.partition(b"\n")
        assert line.startswith(b"FRAME")
        buf = np.frombuffer(rest[:ny + 2 * nc], np.uint8)
        assert buf.size == ny + 2 * nc
        frames.append((buf[:ny].reshape(ih, iw), buf[ny:ny + nc].reshape(ih // 2, iw // 2), buf[ny + nc:].reshape(ih // 2, iw // 2)))
        rest = rest[ny + 2 * nc:]
    return iw, ih, frames
