"""Model-ready tensors without a GPU: the header's declarations and the library's exports, sizeof(rd_tensor_spec), rd_tensor_element against the restatement
(tests/tensor.py) in every bit for every dtype, m and box sum, the restatement's half and bfloat16 against torch's on the CPU, rd_tensor_spec_ok and
rd_tensor_bytes, the restatement against tests/rectify.py and tests/match.py where the contract says they coincide, and the host-only code under the sanitizers
as a plain process.  No tolerance."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rectdetect_amd as ra
from tests import helpers
from tests import match
from tests import rectify
from tests import tensor

FUNCTIONS = ("rd_tensor_spec_ok", "rd_tensor_bytes", "rd_tensor_element", "rd_tensor_limits", "rd_rectifier_create_tensor", "rd_rectifier_patch_bytes")
CONSTANTS = {"RD_TENSOR_U8": 0, "RD_TENSOR_F16": 1, "RD_TENSOR_BF16": 2, "RD_TENSOR_F32": 3, "RD_TENSOR_NHWC": 0, "RD_TENSOR_NCHW": 1, "RD_TENSOR_BGR": 0, "RD_TENSOR_RGB": 1,
             "RD_TENSOR_GRAY": 2}
# (scale, bias): ordinary normalisations, a negative scale, a bias of -0.0 (0 * 1 + -0.0 = +0.0, 0 * -1 + -0.0 = -0.0), a scale that overflows binary16 to infinity,
# scales that overflow binary32 to either infinity, integers 2048 .. 2303 and 256 .. 511 - whose odd ones are exact ties of binary16 and of bfloat16 -, and values
# that are subnormal in binary16
PAIRS = ((1.0 / 255.0, -0.5), (0.017124754, -2.1179039), (-0.0171, 2.0), (1.0, -0.0), (-1.0, -0.0), (1000.0, 0.0), (3.0e38, 1.0), (-3.0e38, 0.0), (1.0, 2048.0), (1.0, 256.0),
         (1.0e-7, 0.0), (2.3e-10, 6.0e-8))


def header():
    return open(os.path.join(helpers.ROOT, "include", "rectdetect_hip.h")).read()


def test_header_declares_the_functions_and_constants():
    txt = header()
    for name, value in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), txt), name
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    assert re.search(r"typedef struct \{ int32_t dtype, layout, channels, oversample; float scale\[3\], bias\[3\]; \} rd_tensor_spec;", txt)
    assert "a NaN cannot arise" in txt      # (the header says why the bfloat16 formula needs no NaN case)
    for name, value in CONSTANTS.items():
        assert getattr(ra, name[3:]) == value


def test_library_exports_the_functions():
    L = ctypes.CDLL(ra.LIB_PATH)
    missing = [n for n in FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_sizeof_the_spec_is_40(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "rectdetect_hip.h"\nint main(void) { return sizeof(rd_tensor_spec) == 40 && offsetof(rd_tensor_spec, scale) == 16 && offsetof(rd_tensor_spec, bias) == 28 ? 0 : 1; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-DCL_TARGET_OPENCL_VERSION=120", "-I", os.path.join(helpers.ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    assert ra.TENSOR_SPEC_DTYPE.itemsize == 40 and ra.TENSOR_SPEC_DTYPE.fields["scale"][1] == 16 and ra.TENSOR_SPEC_DTYPE.fields["bias"][1] == 28


def test_limits():
    assert ra.tensor_limits() == {"dtypes": tensor.DTYPES, "layouts": tensor.LAYOUTS, "channels": tensor.CHANNELS, "oversamplings": tensor.OVERSAMPLINGS}
    assert "oversample m is 1, 2 or 4" in header()


def library_elements(spec, c, sums):
    """rd_tensor_element for every sum: an array of the spec's dtype"""
    L, dt = ra.lib(), tensor.numpy_dtype(spec)
    out, size = np.zeros(len(sums), dt), np.dtype(dt).itemsize
    s = np.ascontiguousarray(spec, ra.TENSOR_SPEC_DTYPE).reshape(())
    for k, S in enumerate(sums):
        assert L.rd_tensor_element(s.ctypes.data, c, int(S), out.ctypes.data + k * size) == size
    return out


@pytest.mark.parametrize("dtype", tensor.DTYPES, ids=[tensor.DTYPE_NAMES[d] for d in tensor.DTYPES])
@pytest.mark.parametrize("m", tensor.OVERSAMPLINGS)
def test_element_equals_the_restatement_in_every_bit_for_every_box_sum(dtype, m):
    sums = np.arange(255 * m * m + 1)
    ties = infs = negzero = subnormal = 0
    for k, (scale, bias) in enumerate(PAIRS):
        gray = k % 2 == 1
        c = 0 if gray else k % 3
        sc, bi = [np.nan] * 3, [np.nan] * 3      # (only channel c's may be read)
        sc[c], bi[c] = scale, bias
        spec = ra.tensor_spec(dtype, k % 2, ra.TENSOR_GRAY if gray else ra.TENSOR_RGB, m, sc, bi)
        got, want = library_elements(spec, c, sums), tensor.elements(spec, c, sums)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (tensor.name(spec), scale, bias, np.nonzero(got.view(np.uint8) != want.view(np.uint8))[0][:4])
        v = tensor.f32_value(sums, m, spec["scale"][c], spec["bias"][c])
        assert not np.isnan(v).any()
        u = v.view(np.uint32)
        if dtype == ra.TENSOR_BF16:
            ties += int(((u & 0xFFFF) == 0x8000).sum())
            infs += int(((want & 0x7FFF) == 0x7F80).sum())
        elif dtype == ra.TENSOR_F16:
            ties += int((((u & 0x1FFF) == 0x1000) & (np.abs(v) >= 6.2e-5) & (np.abs(v) < 65504)).sum())
            infs += int(np.isinf(want).sum())
            subnormal += int(((want.view(np.uint16) & 0x7C00) == 0).sum() - (want == 0).sum())
        elif dtype == ra.TENSOR_F32:
            infs += int(np.isinf(want).sum())
        if dtype != ra.TENSOR_U8:
            negzero += int((want.view(want.dtype.str.replace("f", "u")) == (1 << (8 * want.itemsize - 1))).sum())
    if dtype == ra.TENSOR_U8:
        spec = ra.tensor_spec(dtype, 0, ra.TENSOR_BGR, m)
        assert library_elements(spec, 2, sums).tolist() == [(S + m * m // 2) // (m * m) for S in sums.tolist()]      # the rounded mean, 0 .. 255
    else:
        assert infs > 0 and negzero > 0, (infs, negzero)      # the sweep met what it was built to meet
        if dtype in (ra.TENSOR_F16, ra.TENSOR_BF16):
            assert ties >= 100, ties
        if dtype == ra.TENSOR_F16:
            assert subnormal > 0


def test_element_refuses_bad_arguments():
    spec = ra.tensor_spec(ra.TENSOR_F32, ra.TENSOR_NCHW, ra.TENSOR_GRAY, 2)
    assert len(ra.tensor_element(spec, 0, 17)) == 4
    for bad in (dict(c=1), dict(c=-1), dict(dtype=4), dict(oversample=3), dict(channels=3)):
        s = spec.copy()
        for k, v in bad.items():
            if k != "c":
                s[k] = v
        with pytest.raises(ValueError):
            ra.tensor_element(s, bad.get("c", 0), 17)


def restated_values():
    """binary32 values of the sweep, both signs, and the exact ties and extremes of both 16-bit formats"""
    parts = [tensor.f32_value(np.arange(255 * 16 + 1), 4, s, b) for s, b in PAIRS]
    parts.append(np.array([0.0, -0.0, 65504.0, 65519.99, 65520.0, 65536.0, 1e-8, 2.9802322e-8, 2.9802326e-8, 5.9604645e-8, 6.1035156e-5, 3.3895314e38, 3.4028235e38, np.inf, -np.inf], np.float32))
    return np.concatenate(parts).astype(np.float32)


def test_restated_bfloat16_equals_torch():
    import torch
    v = restated_values()
    want = torch.from_numpy(v.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(tensor.bf16_bits(v), want)


def test_restated_half_equals_torch():
    import torch
    v = restated_values()
    want = torch.from_numpy(v.copy()).to(torch.float16).numpy()
    with np.errstate(all="ignore"):
        assert v.astype(np.float16).tobytes() == want.tobytes()


def test_spec_ok_refuses_what_the_header_says():
    ok = ra.tensor_spec(ra.TENSOR_F16, ra.TENSOR_NCHW, ra.TENSOR_RGB, 2, 1 / 255.0, -0.5)
    assert ra.tensor_spec_ok(ok, 128, 128)
    for field, values in (("dtype", (-1, 4, 255)), ("layout", (-1, 2, 3)), ("channels", (-1, 3, 4)), ("oversample", (0, 3, 8, -1, 5))):
        for v in values:
            s = ok.copy()
            s[field] = v
            assert not ra.tensor_spec_ok(s, 128, 128), (field, v)
            assert ra.tensor_bytes(s, 128, 128) == 0
    for field in ("scale", "bias"):
        for v in (np.nan, np.inf, -np.inf):
            for c in range(3):
                s = ok.copy()
                s[field][c] = v
                assert not ra.tensor_spec_ok(s, 128, 128), (field, v, c)
                s["channels"] = ra.TENSOR_GRAY
                assert ra.tensor_spec_ok(s, 128, 128) == (c != 0), (field, v, c, "GRAY uses index 0 alone")
                s["dtype"] = ra.TENSOR_U8
                assert ra.tensor_spec_ok(s, 128, 128), "U8 ignores scale and bias"
    for m in tensor.OVERSAMPLINGS:
        s = ok.copy()
        s["oversample"] = m
        assert ra.tensor_spec_ok(s, 16384 // m, 16384 // m)
        assert not ra.tensor_spec_ok(s, 16384 // m + 1, 8) and not ra.tensor_spec_ok(s, 8, 16384 // m + 1)
        assert not ra.tensor_spec_ok(s, 0, 8) and not ra.tensor_spec_ok(s, 8, 0)
    assert ra.lib().rd_tensor_spec_ok(None, 8, 8) == 0 and ra.lib().rd_tensor_bytes(None, 8, 8) == 0


def test_bytes_for_every_dtype_and_channel_kind():
    size = {ra.TENSOR_U8: 1, ra.TENSOR_F16: 2, ra.TENSOR_BF16: 2, ra.TENSOR_F32: 4}
    for dt in tensor.DTYPES:
        for ch in tensor.CHANNELS:
            for layout in tensor.LAYOUTS:
                for m in tensor.OVERSAMPLINGS:
                    spec = ra.tensor_spec(dt, layout, ch, m)
                    C = 1 if ch == ra.TENSOR_GRAY else 3
                    assert ra.tensor_bytes(spec, 33, 9) == 33 * 9 * C * size[dt]
                    assert np.dtype(tensor.numpy_dtype(spec)).itemsize == size[dt] and int(np.prod(tensor.shape(spec, 1, 33, 9))) == 33 * 9 * C


def noise(iw, ih, seed):
    return np.random.default_rng(seed).integers(0, 256, (ih, iw, 3), dtype=np.uint8)


QUADS = np.array([[(10.25, 8.5), (80.75, 3.0), (90.0, 50.5), (5.5, 44.0)], [(-6.0, -4.0), (50.0, -2.5), (45.0, 40.0), (-3.0, 30.0)], [(0, 0), (60, 0), (20, 20), (0, 50)]], np.float64)


def test_restatement_with_u8_nhwc_bgr_m1_is_the_classic_patch():
    bgr = noise(97, 61, 3)
    spec = ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NHWC, ra.TENSOR_BGR, 1)
    for pw, ph in ((33, 9), (5, 3)):
        got, st = tensor.tensors(bgr, QUADS, pw, ph, spec)
        want, wst = rectify.patches(bgr, QUADS, pw, ph)
        assert st.tolist() == wst.tolist() == [1, 1, 0]
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    rgb, _ = tensor.tensors(bgr, QUADS, 33, 9, ra.tensor_spec(ra.TENSOR_U8, ra.TENSOR_NCHW, ra.TENSOR_RGB, 1))
    assert np.array_equal(rgb.transpose(0, 2, 3, 1)[..., ::-1], rectify.patches(bgr, QUADS, 33, 9)[0])


@pytest.mark.parametrize("m", tensor.OVERSAMPLINGS)
def test_restatement_with_u8_gray_is_the_matchers_signature_plus_128(m):
    G = 8
    bgr = noise(97, 61, 4)
    quads = np.concatenate([QUADS, match.whole(97, 61)[None]])
    sig, st = match.signatures(bgr, quads, G, m)
    for layout in tensor.LAYOUTS:
        got, gst = tensor.tensors(bgr, quads, G, G, ra.tensor_spec(ra.TENSOR_U8, layout, ra.TENSOR_GRAY, m))
        assert gst.tolist() == st.tolist()
        for k in range(len(quads)):
            if st[k]:
                assert np.array_equal(got[k].reshape(G, G).astype(np.int64), sig[k] + 128)
            else:
                assert not got[k].any()


def test_host_code_under_the_sanitizers_as_a_plain_process(tmp_path):
    """tests/native/tensor_host_check.c with csrc/rd_tensor_host.c, both compiled with -fsanitize=address,undefined, run as a process of its own"""
    csrc = os.path.join(helpers.ROOT, "rectdetect_amd", "csrc")
    exe = str(tmp_path / "tensor_host_check")
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-DCL_TARGET_OPENCL_VERSION=120", "-I", csrc, "-I", os.path.join(helpers.ROOT, "include"),
           os.path.join(helpers.ROOT, "tests", "native", "tensor_host_check.c"), os.path.join(csrc, "rd_tensor_host.c"), "-o", exe, "-lm"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode != 0 and "sanitize" in p.stderr and ("cannot find" in p.stderr or "unrecognized" in p.stderr):
        pytest.skip("this compiler has no address / undefined sanitizer runtime: %s" % p.stderr[-200:])
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tensor_host_check: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
