"""rectdetect_amd - MI355X-native rectangle/polyline detector (host-side Python mirror of the C API).

The product is ``librectdetect_hip.so`` (hand-written gfx950 HIP kernels behind the reference's C API:
``oclimgutil.h`` / ``oclpolyline.h`` / ``oclrect.h`` / ``oclhelper.h``).  This module only binds that C ABI with
ctypes so that tests and ``bench.py`` can drive it; it contains no detector logic and NO CPU fallback: if the
library or a GPU is missing, calls fail loudly.

Mirrors of the reference programs' call sequences:
  * :func:`poly_frame`  - poly.cpp:104-131 (explicit operator sequence + ``oclpolyline_execute``)
  * :class:`RectDetector` - rect.cpp / vidrect.cpp (``oclrect_executeOnce`` / ``enqueueTask`` / ``pollTask``)
  * :class:`Detector` - the ``rd_detector`` extension (device-resident frames, several frames in flight)
  * :class:`PolylineDetector` - its polyline kind: poly.cpp / vidpoly.cpp per frame, several frames in flight
  * :class:`Rectifier` - the ``rd_rectifier`` extension: what is inside detected quads as upright patches of fixed size, or - with a
    :func:`tensor_spec` - as model-ready tensors (float, planar, normalised, box-filtered), or - with a :func:`scan_spec` - as scanned pages (shading-corrected
    gray, bilevel bytes or packed bit rows), or - with a :func:`grade_spec` - as graded quads (per-cell sharpness, exposure and glare records, a histogram),
    or - with a :func:`code_spec` and a dictionary - as decoded quads (a grid code's payload, its id, rotation and Hamming distance), or - with a
    :func:`blob_spec` - as page components (the connected ink regions of the bilevel page as boxes, areas and coordinate sums, and the despeckled page)
  * :class:`Annotator` - the ``rd_annotator`` extension: rectangles' outlines and line segments drawn into frames on the device
  * :class:`Compositor` - the ``rd_compositor`` extension: a colour or an image written into the quads of a frame on the device
  * :class:`Matcher` - the ``rd_matcher`` extension: which template of a library is inside each quad, decided on the device
"""
import collections
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RD_LIB_PATH") or os.path.join(_HERE, "librectdetect_hip.so")      # (RD_LIB_PATH: tuning builds, tools/variants.sh)

RECT_DTYPE = np.dtype([("c2", "<f8", (4, 2)), ("c3", "<f8", (4, 3)), ("value", "<f8"), ("status", "<u4"), ("_pad", "<u4")])
LS_DTYPE = np.dtype([("x0", "<f4"), ("y0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("startIndex", "<i4"), ("endIndex", "<i4"),
                     ("leftPtr", "<i4"), ("rightPtr", "<i4"), ("startCount", "<i4"), ("endCount", "<i4"), ("maxDist", "<i4"),
                     ("polyid", "<i4"), ("npix", "<i4"), ("level", "<i4")])
# a primitive of an annotator's job (rd_annot_prim; the coverage contract is in include/rectdetect_hip.h, "annotated frames")
PRIM_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("thickness", "u1")])
assert RECT_DTYPE.itemsize == 176 and LS_DTYPE.itemsize == 56 and PRIM_DTYPE.itemsize == 20
ANNOT_CLEAR = 1
COMP_ITEM_DTYPE = np.dtype([("quad", "<f8", (4, 2)), ("patch", "<i4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("pad", "u1")])      # rd_comp_item, 72 bytes
COMP_FILL = -1
# the record of a matched quad (rd_match; the contract is in include/rectdetect_hip.h, "matched quads")
MATCH_DTYPE = np.dtype([("status", "<i4"), ("tmpl", "<i4"), ("rot", "<i4"), ("dot", "<i4"), ("tmpl2", "<i4"), ("rot2", "<i4"), ("dot2", "<i4"), ("sa", "<i4"),
                        ("saa", "<i8"), ("score", "<f8"), ("score2", "<f8")])
assert MATCH_DTYPE.itemsize == 56
MATCH_DOTS = 1
# a rectifier's tensor spec (rd_tensor_spec; the contract is in include/rectdetect_hip.h, "model-ready tensors")
TENSOR_U8, TENSOR_F16, TENSOR_BF16, TENSOR_F32 = range(4)
TENSOR_NHWC, TENSOR_NCHW = 0, 1
TENSOR_BGR, TENSOR_RGB, TENSOR_GRAY = range(3)
LENS_DTYPE = np.dtype([(n, "<f8") for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")])      # rd_lens, 72 bytes
VIEW_DTYPE = np.dtype([(n, "<f8") for n in ("fx", "fy", "cx", "cy")])                                    # rd_view, 32 bytes
TENSOR_SPEC_DTYPE = np.dtype([("dtype", "<i4"), ("layout", "<i4"), ("channels", "<i4"), ("oversample", "<i4"), ("scale", "<f4", (3,)), ("bias", "<f4", (3,))])
assert TENSOR_SPEC_DTYPE.itemsize == 40
TENSOR_NUMPY = {TENSOR_U8: np.dtype(np.uint8), TENSOR_F16: np.dtype(np.float16), TENSOR_BF16: np.dtype(np.uint16), TENSOR_F32: np.dtype(np.float32)}      # (bf16: its bits)
# a rectifier's scan spec (rd_scan_spec; the contract is in include/rectdetect_hip.h, "scanned pages")
SCAN_FLAT, SCAN_BILEVEL, SCAN_BITS = range(3)
SCAN_SPEC_DTYPE = np.dtype([(n, "<i4") for n in ("mode", "radius", "k", "d", "white", "oversample", "invert", "reserved")])
assert SCAN_SPEC_DTYPE.itemsize == 32
# a rectifier's grade spec and the record of a cell (rd_grade_spec, rd_grade_cell; the contract is in include/rectdetect_hip.h, "graded quads")
GRADE_SPEC_DTYPE = np.dtype([("cells", "<i4"), ("dark", "<i4"), ("bright", "<i4"), ("edge", "<i4"), ("oversample", "<i4"), ("hist", "<i4"), ("reserved", "<i4", (2,))])
GRADE_CELL_DTYPE = np.dtype([("n", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("ne", "<i4"), ("sg", "<i8"), ("sgg", "<i8"), ("sl", "<i8"), ("sll", "<i8")])
assert GRADE_SPEC_DTYPE.itemsize == 32 and GRADE_CELL_DTYPE.itemsize == 48
GRADE_CELL_BYTES, GRADE_HIST_BYTES, GRADE_MAX_EDGE = 48, 1024, 1020
# a rectifier's code spec and the record of a quad (rd_code_spec, rd_code; the contract is in include/rectdetect_hip.h, "decoded quads")
CODE_SPEC_DTYPE = np.dtype([("n", "<i4"), ("border", "<i4"), ("inset", "<i4"), ("polarity", "<i4"), ("oversample", "<i4"), ("contrast", "<i4"), ("max_border", "<i4"), ("max_hamming", "<i4")])
CODE_DTYPE = np.dtype([("bits", "<u8"), ("id", "<i4"), ("rot", "<i4"), ("hamming", "<i4"), ("second", "<i4"), ("border_errors", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("margin", "<i4"), ("ok", "<i4"), ("reserved", "<i4")])
assert CODE_SPEC_DTYPE.itemsize == 32 and CODE_DTYPE.itemsize == 48
CODE_BYTES, CODE_MAX_DICT, CODE_NONE = 48, 4096, 65
# a rectifier's blob spec, the head of a quad and the record of a component (rd_blob_spec, rd_blob_head, rd_blob; the contract is in include/rectdetect_hip.h, "page components")
BLOB_SPEC_DTYPE = np.dtype([("radius", "<i4"), ("k", "<i4"), ("d", "<i4"), ("oversample", "<i4"), ("invert", "<i4"), ("connectivity", "<i4"), ("min_area", "<i4"), ("max_area", "<i4"),
                            ("max_blobs", "<i4"), ("page", "<i4"), ("reserved", "<i4", (2,))])
BLOB_HEAD_DTYPE = np.dtype([(n, "<i4") for n in ("ink", "all", "found", "written", "ink_kept", "largest", "flags", "reserved")])
BLOB_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("area", "<i4"), ("first", "<i4"), ("sx", "<i8"), ("sy", "<i8")])
assert BLOB_SPEC_DTYPE.itemsize == 48 and BLOB_HEAD_DTYPE.itemsize == 32 and BLOB_DTYPE.itemsize == 40
BLOB_HEAD_BYTES, BLOB_BYTES, BLOB_OVERFLOW = 32, 40, 1
ANNOT_SEG_ALL, ANNOT_SEG_CHAINS = 0, 1

# pixel formats of enqueue_planes (rd_detector_enqueue_planes; the conversion contract is in include/rectdetect_hip.h)
PIX_BGR, PIX_RGB, PIX_BGRA, PIX_RGBA, PIX_NV12, PIX_I420 = range(6)
PIX_NAMES = {PIX_BGR: "BGR", PIX_RGB: "RGB", PIX_BGRA: "BGRA", PIX_RGBA: "RGBA", PIX_NV12: "NV12", PIX_I420: "I420"}

# counters of rd_detector_counter this module reads (enum rd_counter of include/rectdetect_hip.h says what each counts)
CTR_POLY_REDONE, CTR_DEVICE_US, CTR_DEVICE_FRAMES, CTR_REGION_REDONE, CTR_REGION_BUDGET, CTR_ABSORB_SLOW, CTR_FRAMES_PER_LAUNCH = 0, 1, 2, 4, 5, 14, 15

CL_MEM_READ_WRITE = 1 << 0
CL_MEM_COPY_HOST_PTR = 1 << 5
CL_TRUE = 1

_lib = None


def lib():
    """The loaded C-ABI library; raises if it has not been built (run ``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("rectdetect_amd: %s is missing - build it (python -c 'import __graft_entry__ as g; g.build()'). "
                               "There is no CPU fallback." % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def _declare(L):
    vp, ci, cf, cd, cz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    sig = {
        "rd_version": (ctypes.c_char_p, []),
        "rd_device_count": (ci, []),
        "rd_select_device": (None, [ci]),
        "rd_device_pci_bus_id": (ci, [ci, ctypes.c_char_p, ci]),
        "rd_device_alloc": (vp, [cz]),
        "rd_device_free": (None, [vp]),
        "rd_host_alloc": (vp, [cz]),
        "rd_host_free": (None, [vp]),
        "rd_release_cached_streams": (None, [ci]),
        "rd_upload": (None, [vp, vp, cz]),
        "rd_download": (None, [vp, vp, cz]),
        "rd_detector_create": (vp, [ci, ci, ci, ci, ci]),
        "rd_detector_destroy": (None, [vp]),
        "rd_polyline_detector_create": (vp, [ci, ci, ci, ci, ci, cf, ci]),
        "rd_detector_poll_segments": (vp, [vp, vp]),
        "rd_detector_enqueue": (ctypes.c_long, [vp, vp, ci, ci]),
        "rd_detector_enqueue_planes": (ctypes.c_long, [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci]),
        "rd_detector_enqueue_scaled": (ctypes.c_long, [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ci]),
        "rd_detector_poll": (vp, [vp, cd]),
        "rd_detector_drain": (None, [vp]),
        "rd_detector_set_aperture": (None, [vp, cd]),
        "rd_detector_counter": (ctypes.c_long, [vp, ci]),
        "rd_detector_last_segments": (ci, [vp, vp, ci]),
        "rd_detector_debug_plane": (cz, [vp, ctypes.c_char_p, vp, cz]),
        "rd_postprocess_planes": (vp, [vp, vp, vp, ci, ci, cd]),
        "rd_postprocess_planes_device": (vp, [ci, vp, vp, vp, ci, ci, cd, vp]),
        "rd_post_device_limits": (None, [vp]),
        "rd_polyline_planes_device": (ci, [ci, vp, ci, ci, ci, cf, ci, ci, ci, vp, vp, vp]),
        "rd_polyline_limits": (None, [vp]),
        "rd_region_planes_device": (ci, [ci, ci, ci, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp]),
        "rd_region_limits": (None, [ci, ci, vp]),
        "rd_votes_planes_device": (ci, [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ctypes.c_int32, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rd_votes_limits": (None, [vp]),
        "rd_probe_pixels": (None, [cf, cf, cf, cf, ci, ci, vp]),
        "rd_post_run": (vp, [vp, ci, vp, ci, ci, cd]),
        "rd_post_helpers_configure": (None, [ci]),
        "rd_post_helpers_arm": (None, []),
        "rd_post_helpers": (ci, []),
        # rectified patches (rd_rectify.hip)
        "rd_rect_quads": (None, [vp, ci, vp]),
        "rd_rect_aspect": (cd, [vp]),
        "rd_rectify_coefficients": (None, [vp, vp, ctypes.POINTER(ci)]),
        "rd_rectifier_create": (vp, [ci, ci, ci, ci, ci]),
        "rd_rectifier_destroy": (None, [vp]),
        "rd_rectifier_enqueue": (ctypes.c_long, [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ci, ci, vp, ci, vp, ci]),
        "rd_rectifier_wait": (ci, [vp, vp]),
        "rd_detector_rectify_polled": (ctypes.c_long, [vp, vp, vp, ci, vp, ci]),
        # model-ready tensors (rd_rectify.hip, rd_tensor_host.c)
        "rd_tensor_spec_ok": (ci, [vp, ci, ci]),
        "rd_tensor_bytes": (cz, [vp, ci, ci]),
        "rd_tensor_element": (ci, [vp, ci, ctypes.c_int32, vp]),
        "rd_tensor_limits": (None, [vp]),
        "rd_rectifier_create_tensor": (vp, [ci, ci, ci, ci, ci, vp]),
        "rd_rectifier_patch_bytes": (cz, [vp]),
        # scanned pages (rd_rectify.hip, rd_scan_host.c)
        "rd_scan_spec_ok": (ci, [vp, ci, ci]),
        "rd_scan_bytes": (cz, [vp, ci, ci]),
        "rd_scan_pixel": (ci, [vp, ci, ci, ci, vp, vp]),
        "rd_scan_limits": (None, [vp]),
        "rd_rectifier_create_scan": (vp, [ci, ci, ci, ci, ci, vp]),
        # graded quads (rd_rectify.hip, rd_grade_host.c)
        "rd_grade_spec_ok": (ci, [vp, ci, ci]),
        "rd_grade_bytes": (cz, [vp, ci, ci]),
        "rd_grade_cell_of": (ci, [vp, ci, ci, ci, ci]),
        "rd_grade_limits": (None, [vp]),
        "rd_grade_sharpness": (cd, [vp]),
        "rd_grade_percentile": (ci, [vp, ci, ci]),
        "rd_rectifier_create_grade": (vp, [ci, ci, ci, ci, ci, vp]),
        # decoded quads (rd_rectify.hip, rd_code_host.c)
        "rd_code_spec_ok": (ci, [vp, ci, ci]),
        "rd_code_bytes": (cz, [vp, ci, ci]),
        "rd_code_cell_of": (ci, [vp, ci, ci, ci, ci, vp]),
        "rd_code_rotate": (ctypes.c_uint64, [ctypes.c_uint64, ci, ci]),
        "rd_code_limits": (None, [vp]),
        "rd_code_distance": (ci, [vp, ci, ci]),
        "rd_code_dictionary": (ci, [ci, ci, ci, ctypes.c_uint64, ci, vp]),
        "rd_code_render": (cz, [vp, ctypes.c_uint64, ci, vp]),
        "rd_code_upright": (None, [vp, ci, vp]),
        "rd_rectifier_create_code": (vp, [ci, ci, ci, ci, ci, vp, vp, ci]),
        # page components (rd_rectify.hip, rd_blob_host.c)
        "rd_blob_spec_ok": (ci, [vp, ci, ci]),
        "rd_blob_bytes": (cz, [vp, ci, ci]),
        "rd_blob_limits": (None, [vp]),
        "rd_blob_page_host": (ci, [vp, ci, ci, vp, vp]),
        "rd_rectifier_create_blobs": (vp, [ci, ci, ci, ci, ci, vp]),
        "rd_blobs_pages_device": (ci, [ci, vp, ci, ci, ci, vp, vp, vp]),
        # annotated frames (rd_annotate.hip)
        "rd_annot_covers": (ci, [vp, ci, ci]),
        "rd_annot_touches": (ci, [vp, ci, ci, ci, ci]),
        "rd_annot_yuv": (None, [ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, vp]),
        "rd_annot_limits": (None, [vp]),
        "rd_annot_rects": (ci, [vp, ci, ci, vp, vp]),
        "rd_annot_segments": (ci, [vp, ci, ci, vp, ci]),
        "rd_annotator_create": (vp, [ci, ci, ci]),
        "rd_annotator_destroy": (None, [vp]),
        "rd_annotator_enqueue": (ctypes.c_long, [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ci, ci, vp, ci, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci]),
        "rd_annotator_wait": (ci, [vp]),
        "rd_detector_annotate_polled": (ctypes.c_long, [vp, vp, vp, ci, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci]),
        # composited quads (rd_composite.hip, rd_comp_host.c)
        "rd_composite_coefficients": (None, [vp, ci, ci, vp, vp, ctypes.POINTER(ci)]),
        "rd_composite_covers": (ci, [vp, ci, ci, ci, ci, vp]),
        "rd_composite_tiles": (ci, [vp, ci, ci, ci, vp, ci]),
        "rd_comp_limits": (None, [vp]),
        "rd_compositor_create": (vp, [ci, ci, ci, ci, ci]),
        "rd_compositor_destroy": (None, [vp]),
        "rd_compositor_enqueue": (ctypes.c_long, [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ci, ci, vp, ci, vp, ci, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci]),
        "rd_compositor_wait": (ci, [vp, vp]),
        "rd_detector_composite_polled": (ctypes.c_long, [vp, vp, vp, ci, vp, ci, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci]),
        # matched quads (rd_match.hip, rd_match_host.c)
        "rd_match_score": (None, [vp, ci, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64]),
        "rd_match_limits": (None, [vp]),
        "rd_matcher_create": (vp, [ci, ci, ci, ci, ci, ci]),
        "rd_matcher_destroy": (None, [vp]),
        "rd_matcher_add": (ci, [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ci, ci, vp]),
        "rd_matcher_templates": (ci, [vp]),
        "rd_matcher_signature": (ci, [vp, ci, ci, vp, vp]),
        "rd_matcher_enqueue": (ctypes.c_long, [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ci, ci, vp, ci, ci]),
        "rd_matcher_wait": (ci, [vp, vp, vp]),
        "rd_detector_match_polled": (ctypes.c_long, [vp, vp, vp, ci, ci]),
        # remapped frames (rd_remap.hip, rd_remap_host.c)
        "rd_remap_points": (None, [vp, vp, vp, ci, vp]),
        "rd_remap_table_lens": (ci, [vp, vp, ci, ci, ci, ci, vp]),
        "rd_remap_table_map": (ci, [vp, vp, ci, ci, ci, ci, vp]),
        "rd_view_tan_aov": (cd, [vp, ci]),
        "rd_remap_limits": (None, [vp]),
        "rd_remapper_create_lens": (vp, [ci, vp, vp, ci, ci, ci, ci, ci]),
        "rd_remapper_create_map": (vp, [ci, vp, vp, ci, ci, ci, ci, ci]),
        "rd_remapper_destroy": (None, [vp]),
        "rd_remapper_inside": (ci, [vp]),
        "rd_remapper_enqueue": (ctypes.c_long, [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ci, ctypes.c_uint32, vp, ci, ci]),
        "rd_remapper_wait": (ci, [vp]),
        "rd_synth_frame": (None, [vp, ci, ci, ci, ctypes.c_uint64, ci, ci]),
        "rd_synth_num_quads": (ci, [ci, ci]),
        # reference API (oclhelper.h / raw cl*)
        "simpleGetDevice": (vp, [ci]),
        "simpleCreateContext": (vp, [vp]),
        "allocatePinnedMemory": (vp, [cz, vp, vp]),
        "freePinnedMemory": (None, [vp, vp, vp]),
        "clCreateCommandQueue": (vp, [vp, vp, ctypes.c_ulong, vp]),
        "clReleaseCommandQueue": (ci, [vp]),
        "clReleaseContext": (ci, [vp]),
        "clCreateBuffer": (vp, [vp, ctypes.c_ulong, cz, vp, vp]),
        "clReleaseMemObject": (ci, [vp]),
        "clEnqueueReadBuffer": (ci, [vp, vp, ctypes.c_uint, cz, cz, vp, ctypes.c_uint, vp, vp]),
        "clEnqueueWriteBuffer": (ci, [vp, vp, ctypes.c_uint, cz, cz, vp, ctypes.c_uint, vp, vp]),
        "clFinish": (ci, [vp]),
        # oclimgutil.h
        "init_oclimgutil": (vp, [vp, vp]),
        "dispose_oclimgutil": (None, [vp]),
        "oclimgutil_clear": (vp, [vp, vp, ci, vp, vp]),
        "oclimgutil_copy": (vp, [vp, vp, vp, ci, vp, vp]),
        "oclimgutil_cast_i_f": (vp, [vp, vp, vp, cf, ci, vp, vp]),
        "oclimgutil_cast_c_i": (vp, [vp, vp, vp, ci, vp, vp]),
        "oclimgutil_threshold_i_i": (vp, [vp, vp, vp, ci, ci, ci, ci, vp, vp]),
        "oclimgutil_threshold_f_f": (vp, [vp, vp, vp, cf, cf, cf, ci, vp, vp]),
        "oclimgutil_convert_plab_bgr": (vp, [vp, vp, vp, ci, ci, ci, vp, vp]),
        "oclimgutil_unpack_f_f_f_plab": (vp, [vp, vp, vp, vp, vp, ci, ci, vp, vp]),
        "oclimgutil_pack_plab_f_f_f": (vp, [vp, vp, vp, vp, vp, ci, ci, vp, vp]),
        "oclimgutil_iirblur_f_f": (vp, [vp, vp, vp, vp, vp, ci, ci, ci, vp, vp]),
        "oclimgutil_edgevec_f2_f": (vp, [vp, vp, vp, ci, ci, vp, vp]),
        "oclimgutil_edge_f_plab": (vp, [vp, vp, vp, ci, ci, vp, vp]),
        "oclimgutil_thinthres_f_f_f2": (vp, [vp, vp, vp, vp, ci, ci, vp, vp]),
        "oclimgutil_label8x_int_int": (vp, [vp, vp, vp, vp, ci, ci, ci, vp, vp]),
        "oclimgutil_calcStrength": (vp, [vp, vp, vp, vp, ci, ci, vp, vp]),
        "oclimgutil_convert_bgr_lumaf": (vp, [vp, vp, vp, cf, ci, ci, ci, vp, vp]),
        "oclimgutil_convert_bgr_labeli": (vp, [vp, vp, vp, ci, ci, ci, ci, vp, vp]),
        "oclimgutil_convert_bgr_plab": (vp, [vp, vp, vp, ci, ci, ci, vp, vp]),
        "oclimgutil_edge_f_f": (vp, [vp, vp, vp, ci, ci, vp, vp]),
        "oclimgutil_edgevec_f2_plab": (vp, [vp, vp, vp, ci, ci, vp, vp]),
        "oclimgutil_thincubic_f_f_f2": (vp, [vp, vp, vp, vp, ci, ci, vp, vp]),
        "oclimgutil_filterStrength": (vp, [vp, vp, vp, ci, ci, ci, vp, vp]),
        # oclpolyline.h
        "init_oclpolyline": (vp, [vp, vp]),
        "dispose_oclpolyline": (None, [vp]),
        "oclpolyline_execute": (vp, [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, cf, ci, ci, ci, vp, vp]),
        # oclrect.h
        "init_oclrect": (vp, [vp, vp, vp, vp, vp, ci, ci]),
        "dispose_oclrect": (None, [vp]),
        "oclrect_executeOnce": (vp, [vp, vp, ci, cd]),
        "oclrect_enqueueTask": (None, [vp, vp, ci]),
        "oclrect_pollTask": (vp, [vp, cd]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args


_libc = ctypes.CDLL(None)
_libc.free.argtypes = [ctypes.c_void_p]


def _take_rects(ptr):
    """Copy a malloc'd rect_t array (element 0 = header with nItems) into a numpy structured array and free it."""
    if not ptr:
        raise RuntimeError("detector returned NULL")
    n = ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int))[0]
    buf = (ctypes.c_char * (176 * n)).from_address(ptr)
    out = np.frombuffer(buf, dtype=RECT_DTYPE).copy()[1:]
    _libc.free(ptr)
    return out


def gpu_available():
    return os.path.exists(LIB_PATH) and lib().rd_device_count() > 0


class Context:
    """device / context / queue triple created the way the reference programs do (rect.cpp:51-64)."""

    def __init__(self, did=0):
        L = lib()
        if L.rd_device_count() <= 0:
            raise RuntimeError("rectdetect_amd: no HIP device visible - there is no CPU fallback")
        self.device = L.simpleGetDevice(did)
        self.context = L.simpleCreateContext(self.device)
        self.queue = L.clCreateCommandQueue(self.context, self.device, 0, None)

    def buffer(self, array_or_bytes):
        L = lib()
        if isinstance(array_or_bytes, int):
            return L.clCreateBuffer(self.context, CL_MEM_READ_WRITE, array_or_bytes, None, None)
        a = np.ascontiguousarray(array_or_bytes)
        return L.clCreateBuffer(self.context, CL_MEM_READ_WRITE | CL_MEM_COPY_HOST_PTR, a.nbytes, a.ctypes.data, None)

    def read(self, mem, dtype, count):
        out = np.empty(count, dtype)
        rc = lib().clEnqueueReadBuffer(self.queue, mem, CL_TRUE, 0, out.nbytes, out.ctypes.data, 0, None, None)
        if rc != 0:
            raise RuntimeError("clEnqueueReadBuffer failed: %d" % rc)
        return out

    def pinned_copy(self, array):
        """a copy of `array` in page-locked host memory from the reference's own allocator (oclhelper.h: allocatePinnedMemory) as a numpy array; free with free_pinned()"""
        a = np.ascontiguousarray(array)
        p = lib().allocatePinnedMemory(a.nbytes, self.context, self.queue)
        out = np.ctypeslib.as_array((ctypes.c_uint8 * a.nbytes).from_address(p)).view(a.dtype).reshape(a.shape)
        out[...] = a
        return out

    def free_pinned(self, array):
        lib().freePinnedMemory(array.ctypes.data, self.context, self.queue)

    def release(self, *mems):
        for m in mems:
            lib().clReleaseMemObject(m)

    def close(self):
        lib().clReleaseCommandQueue(self.queue)
        lib().clReleaseContext(self.context)


def poly_frame(ctx, bgr, strength_thre=500, minerror=1.0, size_thre=20):
    """poly.cpp:68-131 on a BGR uint8 image (ih, iw, 3): returns (segments[LS_DTYPE] incl. header record, ids[ih*iw])."""
    L = lib()
    ih, iw = bgr.shape[:2]
    ws = bgr.strides[0]
    N = iw * ih
    img = np.zeros(N * 4, np.uint8)
    img[:ws * ih] = np.ascontiguousarray(bgr).reshape(-1)[:ws * ih]
    iu = L.init_oclimgutil(ctx.device, ctx.context)
    pl = L.init_oclpolyline(ctx.device, ctx.context)
    mem = [ctx.buffer(img)] + [ctx.buffer(N * 4) for _ in range(9)]
    memBig, memLS = ctx.buffer(N * 16), ctx.buffer(N * 16)
    q = ctx.queue
    L.oclimgutil_convert_plab_bgr(iu, mem[4], mem[0], iw, ih, ws, q, None)
    L.oclimgutil_unpack_f_f_f_plab(iu, mem[1], mem[2], mem[3], mem[4], iw, ih, q, None)
    L.oclimgutil_iirblur_f_f(iu, mem[0], mem[1], mem[4], mem[5], 2, iw, ih, q, None)
    L.oclimgutil_iirblur_f_f(iu, mem[1], mem[2], mem[4], mem[5], 2, iw, ih, q, None)
    L.oclimgutil_iirblur_f_f(iu, mem[2], mem[3], mem[4], mem[5], 2, iw, ih, q, None)
    L.oclimgutil_pack_plab_f_f_f(iu, mem[4], mem[0], mem[1], mem[2], iw, ih, q, None)
    L.oclimgutil_edgevec_f2_f(iu, memBig, mem[0], iw, ih, q, None)
    L.oclimgutil_edge_f_plab(iu, mem[5], mem[4], iw, ih, q, None)
    L.oclimgutil_thinthres_f_f_f2(iu, mem[2], mem[5], memBig, iw, ih, q, None)
    L.oclimgutil_threshold_f_f(iu, mem[9], mem[2], 0.0, 0.0, 1.0, N, q, None)
    L.oclimgutil_cast_i_f(iu, mem[8], mem[9], 1.0, N, q, None)
    L.oclimgutil_label8x_int_int(iu, mem[3], mem[8], mem[9], 0, iw, ih, q, None)
    L.oclimgutil_clear(iu, mem[4], N * 4, q, None)
    L.oclimgutil_calcStrength(iu, mem[4], mem[2], mem[3], iw, ih, q, None)
    L.oclimgutil_filterStrength(iu, mem[3], mem[4], strength_thre, iw, ih, q, None)
    L.oclimgutil_threshold_i_i(iu, mem[3], mem[3], 0, 0, 1, N, q, None)
    L.oclpolyline_execute(pl, memLS, N * 16, mem[0], mem[3], memBig, mem[4], mem[5], mem[6], mem[7], mem[8], mem[9],
                          minerror, size_thre, iw, ih, q, None)
    ids = ctx.read(mem[0], np.int32, N)
    hdr = ctx.read(memLS, np.int32, 14)
    n = int(hdr[0])
    segs = ctx.read(memLS, np.uint8, (n + 1) * 56).view(LS_DTYPE)
    ctx.release(memLS, memBig, *mem)
    L.dispose_oclpolyline(pl)
    L.dispose_oclimgutil(iu)
    return segs, ids


class RectDetector:
    """rect.cpp:78-105 / vidrect.cpp:128-172: the reference's oclrect API on host frames."""

    def __init__(self, ctx, iw, ih):
        L = lib()
        self.ctx, self.iw, self.ih = ctx, iw, ih
        self.iu = L.init_oclimgutil(ctx.device, ctx.context)
        self.pl = L.init_oclpolyline(ctx.device, ctx.context)
        self.h = L.init_oclrect(self.iu, self.pl, ctx.device, ctx.context, ctx.queue, iw, ih)

    def execute_once(self, bgr, tan_aov):
        a = np.ascontiguousarray(bgr)
        return _take_rects(lib().oclrect_executeOnce(self.h, a.ctypes.data, a.strides[0], float(tan_aov)))

    def enqueue(self, bgr):
        a = np.ascontiguousarray(bgr)
        self._keep = a
        lib().oclrect_enqueueTask(self.h, a.ctypes.data, a.strides[0])

    def poll(self, tan_aov):
        return _take_rects(lib().oclrect_pollTask(self.h, float(tan_aov)))

    def close(self):
        L = lib()
        L.dispose_oclrect(self.h)
        L.dispose_oclpolyline(self.pl)
        L.dispose_oclimgutil(self.iu)


def _plane_args(planes, pitches, on_device, pinned):
    """the plane pointers, pitches and frame kind of the C entry points that take frames in any pixel format, plus the pitches as a list and the host arrays to
    keep alive.  Host frames: numpy arrays (packed formats one HxWxC image; NV12 (Y, UV); I420 (Y, U, V)), pitches from their strides (copied before the call
    returns).  on_device / pinned: plane ADDRESSES, with `pitches` required."""
    if not isinstance(planes, (list, tuple)):
        planes = (planes,)
    planes = list(planes)[:3]
    if on_device or pinned:
        if pitches is None:
            raise ValueError("enqueue_planes: pitches are required for device / pinned planes")
        ptrs = [int(p) if p else None for p in planes]
        pitch = list(pitches)
    else:
        arrs = []
        for p in planes:
            a = np.asarray(p, dtype=np.uint8)
            if a.ndim < 2 or a.strides[0] < 0 or a.strides[-1] != 1 or (a.ndim == 3 and a.strides[1] != a.shape[2]):
                a = np.ascontiguousarray(a)      # (rows need not be adjacent - the pitch says where the next one starts - but a row's bytes must be)
            arrs.append(a)
        ptrs = [a.ctypes.data for a in arrs]
        pitch = [a.strides[0] for a in arrs] if pitches is None else list(pitches)
    ptrs += [None] * (3 - len(ptrs))
    pitch += [0] * (3 - len(pitch))
    return (ctypes.c_void_p * 3)(*ptrs), (ctypes.c_int * 3)(*pitch), 1 if on_device else (2 if pinned else 0), pitch, arrs if not (on_device or pinned) else None


def _enqueue_planes(h, fmt, planes, pitches, on_device, pinned):
    """rd_detector_enqueue_planes for both detector kinds (planes and pitches: _plane_args).  ValueError on an argument error."""
    ptrs, pitch_c, kind, pitch, _ = _plane_args(planes, pitches, on_device, pinned)
    r = lib().rd_detector_enqueue_planes(h, int(fmt), ptrs, pitch_c, kind)
    if r == -1:
        raise ValueError("rd_detector_enqueue_planes: invalid arguments (format %r, pitches %r)" % (fmt, pitch))
    return r


def _source_shapes(fmt, sw, sh):
    """(rows, row bytes) of the planes of an sw x sh frame in format fmt"""
    if fmt in (PIX_BGR, PIX_RGB):
        return [(sh, sw * 3)]
    if fmt in (PIX_BGRA, PIX_RGBA):
        return [(sh, sw * 4)]
    if fmt == PIX_NV12:
        return [(sh, sw), (sh // 2, sw)]
    if fmt == PIX_I420:
        return [(sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2)]
    raise ValueError("enqueue_scaled: unknown pixel format %r" % (fmt,))


def _enqueue_scaled(h, iw, ih, fmt, planes, pitches, scale, on_device, pinned):
    """rd_detector_enqueue_scaled for both detector kinds: planes and pitches as _plane_args, of a frame of scale*iw x scale*ih pixels.  Host planes are checked
    against that SOURCE size.  ValueError on an argument error (nothing enqueued)."""
    ptrs, pitch_c, kind, pitch, arrs = _plane_args(planes, pitches, on_device, pinned)
    if arrs is not None and scale in (1, 2):
        want = _source_shapes(fmt, scale * iw, scale * ih)
        got = [(a.shape[0], a.size // a.shape[0]) for a in arrs]
        if got[:len(want)] != want:
            raise ValueError("enqueue_scaled: a %dx%d %s source has planes of (rows, row bytes) %r, not %r" % (scale * iw, scale * ih, PIX_NAMES[fmt], want, got))
    r = lib().rd_detector_enqueue_scaled(h, int(fmt), ptrs, pitch_c, int(scale), kind)
    if r == -1:
        raise ValueError("rd_detector_enqueue_scaled: invalid arguments (format %r, scale %r, pitches %r)" % (fmt, scale, pitch))
    return r


def _quads_arg(quads):
    q = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 8)
    return q, len(q)


def _prims_arg(prims):
    p = np.ascontiguousarray(prims, dtype=PRIM_DTYPE).reshape(-1)
    return p, len(p)


def _out_args(out_planes, out_pitches):
    """(plane pointers, pitches) of an annotator's destination - ADDRESSES of device or pinned planes - or (None, None): in place"""
    if out_planes is None:
        return None, None
    if out_pitches is None:
        raise ValueError("annotate: out_pitches are required with out_planes")
    if not isinstance(out_planes, (list, tuple)):
        out_planes, out_pitches = (out_planes,), (out_pitches,)
    ptrs = [int(p) if p else None for p in list(out_planes)[:3]]
    pitch = [int(p) for p in list(out_pitches)[:3]]
    return (ctypes.c_void_p * 3)(*(ptrs + [None] * (3 - len(ptrs)))), (ctypes.c_int * 3)(*(pitch + [0] * (3 - len(pitch))))


def _items_arg(items):
    p = np.ascontiguousarray(items, dtype=COMP_ITEM_DTYPE).reshape(-1)
    return p, len(p)


class _PolledJobs:
    """what both detector kinds forward to the services behind their poll: one job on the frame of the most recently polled slot"""

    def rectify_polled(self, rectifier, quads, out, out_pinned=False):
        """patches of `quads` (n x 8 or n x 4 x 2 doubles, patch order) from the frame of the most recently polled slot into `out` - the ADDRESS of device memory or,
        with out_pinned, of pinned host memory - as one job of `rectifier` (take it with rectifier.wait()); a host frame is read from the detector's own copy,
        which lasts until the next enqueue here.  ValueError on an argument error (nothing enqueued)."""
        q, n = _quads_arg(quads)
        r = lib().rd_detector_rectify_polled(self.h, rectifier.h, q.ctypes.data, n, int(out) if out else None, 2 if out_pinned else 1)
        if r == -1:
            raise ValueError("rd_detector_rectify_polled: invalid arguments (nothing polled yet, %d quads, out %r)" % (n, out))
        return r

    def annotate_polled(self, annotator, prims, flags=0, out_planes=None, out_pitches=None, out_pinned=False):
        """`prims` (PRIM_DTYPE; annot_rects / annot_segments make them) drawn into the frame of the most recently polled slot as one job of `annotator` (take it with
        annotator.wait()): a device frame in place, or with out_planes / out_pitches - ADDRESSES of device planes or, with out_pinned, of pinned host planes - into
        another frame; a host frame needs out_planes.  A frame that came in at scale 2 is annotated at its source size.  ValueError on an argument error."""
        p, n = _prims_arg(prims)
        optrs, opitch = _out_args(out_planes, out_pitches)
        r = lib().rd_detector_annotate_polled(self.h, annotator.h, p.ctypes.data, n, int(flags), optrs, opitch, 2 if out_pinned else 1)
        if r == -1:
            raise ValueError("rd_detector_annotate_polled: invalid arguments (nothing polled yet, a host frame without out_planes, %d primitives, flags %r)" % (n, flags))
        return r

    def composite_polled(self, compositor, items, patches=None, out_planes=None, out_pitches=None, out_pinned=False, patches_on_device=False, patches_pinned=False):
        """`items` (COMP_ITEM_DTYPE; comp_items makes them) composited into the frame of the most recently polled slot as one job of `compositor` (take it with
        compositor.wait()): a device frame in place, or with out_planes / out_pitches into another frame; a host frame needs out_planes.  patches as
        Compositor.enqueue.  A frame that came in at scale 2 takes quads in detector coordinates and is composited at its source size.  ValueError on an argument error."""
        it, n = _items_arg(items)
        pp, npatches, pkind, _ = compositor._patches(patches, patches_on_device, patches_pinned)
        optrs, opitch = _out_args(out_planes, out_pitches)
        r = lib().rd_detector_composite_polled(self.h, compositor.h, it.ctypes.data, n, pp, npatches, pkind, optrs, opitch, 2 if out_pinned else 1)
        if r == -1:
            raise ValueError("rd_detector_composite_polled: invalid arguments (nothing polled yet, a host frame without out_planes, %d items, %d patches)" % (n, npatches))
        return r


    def match_polled(self, matcher, quads, flags=0):
        """the records of `quads` (n x 8 or n x 4 x 2 doubles, patch order) in the frame of the most recently polled slot as one job of `matcher` (take it with
        matcher.wait()); a host frame is read from the detector's own copy, which lasts until the next enqueue here.  A frame that came in at scale 2 takes quads in
        detector coordinates.  ValueError on an argument error (nothing enqueued)."""
        q, n = _quads_arg(quads)
        r = lib().rd_detector_match_polled(self.h, matcher.h, q.ctypes.data, n, int(flags))
        if r == -1:
            raise ValueError("rd_detector_match_polled: invalid arguments (nothing polled yet, %d quads, flags %r)" % (n, flags))
        matcher._jobs.append((n, matcher.templates(), int(flags)))
        return r


class Detector(_PolledJobs):
    """The rd_detector extension: frames may already live in HBM, several frames in flight."""

    def __init__(self, iw, ih, device=0, nslots=2, nworkers=0, aperture=None):
        L = lib()
        if L.rd_device_count() <= 0:
            raise RuntimeError("rectdetect_amd: no HIP device visible - there is no CPU fallback")
        self.iw, self.ih, self.N = iw, ih, iw * ih
        self.h = L.rd_detector_create(device, iw, ih, nslots, nworkers)
        if aperture is not None:      # tan(AOV / 2) of the polls to come (rd_detector_set_aperture): work ahead of the first poll can use it
            L.rd_detector_set_aperture(self.h, float(aperture))

    def enqueue(self, frame, ws=None, on_device=False, pinned=False):
        """frame: a numpy BGR image (copied before the call returns) - or, with on_device / pinned, the ADDRESS of a frame in device memory / in pinned host memory
        (rd_host_alloc ...), which is read in place and must stay unchanged until the frame's poll returned"""
        if on_device or pinned:
            return lib().rd_detector_enqueue(self.h, frame, ws, 1 if on_device else 2)
        a = np.ascontiguousarray(frame)
        self._keep = a
        return lib().rd_detector_enqueue(self.h, a.ctypes.data, a.strides[0] if ws is None else ws, 0)

    def enqueue_planes(self, fmt, planes, pitches=None, on_device=False, pinned=False):
        """a frame in pixel format `fmt` (PIX_*): numpy planes (HxWxC; NV12 (Y, UV); I420 (Y, U, V)), copied before the call returns - or, with on_device / pinned,
        the planes' addresses and their `pitches`, read in place until the frame's poll returned.  ValueError on an argument error (nothing enqueued)."""
        return _enqueue_planes(self.h, fmt, planes, pitches, on_device, pinned)

    def enqueue_scaled(self, fmt, planes, pitches=None, on_device=False, pinned=False, scale=2):
        """as enqueue_planes, for a source frame of scale*iw x scale*ih pixels (scale 2: every detector pixel the 2x2 box average of the conversion contract's BGR;
        scale 1: enqueue_planes).  rectify_polled on such a frame takes quads in detector coordinates and reads the full-size source."""
        return _enqueue_scaled(self.h, self.iw, self.ih, fmt, planes, pitches, scale, on_device, pinned)

    def poll(self, tan_aov):
        return _take_rects(lib().rd_detector_poll(self.h, float(tan_aov)))

    def drain(self):
        lib().rd_detector_drain(self.h)

    def redone_frames(self):
        """frames whose polyline stage overflowed the single-launch kernel and was repeated the long way"""
        return lib().rd_detector_counter(self.h, CTR_POLY_REDONE)

    def frames_per_launch(self):
        """frames that share one set of launches (group launches, RD_CTR_FRAMES_PER_LAUNCH)"""
        return lib().rd_detector_counter(self.h, CTR_FRAMES_PER_LAUNCH)

    def region_round_budget(self):
        """(current region-merge round budget, frames repeated with the full budget because theirs was too small)"""
        return lib().rd_detector_counter(self.h, CTR_REGION_BUDGET), lib().rd_detector_counter(self.h, CTR_REGION_REDONE)

    def absorption(self):
        """(undecided pixels the tile kernel of the small-region absorption left to the single-block tail, sweeps the tail took) for the last
        polled frame, and how many frames so far were finished by the slow path (RD_CTR_ABSORB_SLOW)"""
        w = self.plane("absorb", np.int32, 8)
        self.absorb_trace = {"steps": int(w[3]), "us_gather": w[4] / 100.0, "us_sweeps": w[5] / 100.0, "us_choose": w[6] / 100.0, "us_pointers": w[7] / 100.0}
        return int(w[1]), int(w[2]), lib().rd_detector_counter(self.h, CTR_ABSORB_SLOW)

    def device_time(self):
        """(summed device microseconds of the polled frames measured with HIP events, number of frames)"""
        return lib().rd_detector_counter(self.h, CTR_DEVICE_US), lib().rd_detector_counter(self.h, CTR_DEVICE_FRAMES)

    def last_segments(self):
        n = lib().rd_detector_last_segments(self.h, None, 0)
        if n < 0:
            return None
        out = np.zeros(n + 1, LS_DTYPE)
        lib().rd_detector_last_segments(self.h, out.ctypes.data, n + 1)
        return out

    def plane(self, name, dtype=np.int32, count=None):
        count = self.N if count is None else count
        out = np.zeros(count, dtype)
        got = lib().rd_detector_debug_plane(self.h, name.encode(), out.ctypes.data, out.nbytes)
        if got == 0:
            raise KeyError(name)
        return out

    def close(self):
        lib().rd_detector_destroy(self.h)


class PolylineDetector(_PolledJobs):
    """The polyline kind of rd_detector (rd_polyline_detector_create): the line segments of poly.cpp (strength_thre 500, minerror 1, size_thre 20) or
    vidpoly.cpp (2000, 1, 10) for a stream of frames, several in flight."""

    def __init__(self, iw, ih, device=0, nslots=8, strength_thre=500, minerror=1.0, size_thre=20):
        L = lib()
        self.iw, self.ih, self.N = iw, ih, iw * ih
        self.h = L.rd_polyline_detector_create(device, iw, ih, nslots, strength_thre, float(minerror), size_thre)
        if not self.h:
            raise ValueError("rd_polyline_detector_create: invalid arguments (%r)" % ((device, iw, ih, nslots, strength_thre, minerror, size_thre),))

    def enqueue(self, frame, ws=None, on_device=False, pinned=False):
        """as Detector.enqueue: a numpy BGR image (copied before the call returns), or the address of a frame in device / pinned host memory"""
        if on_device or pinned:
            return lib().rd_detector_enqueue(self.h, frame, ws, 1 if on_device else 2)
        a = np.ascontiguousarray(frame)
        self._keep = a
        return lib().rd_detector_enqueue(self.h, a.ctypes.data, a.strides[0] if ws is None else ws, 0)

    def enqueue_planes(self, fmt, planes, pitches=None, on_device=False, pinned=False):
        """as Detector.enqueue_planes"""
        return _enqueue_planes(self.h, fmt, planes, pitches, on_device, pinned)

    def enqueue_scaled(self, fmt, planes, pitches=None, on_device=False, pinned=False, scale=2):
        """as Detector.enqueue_scaled"""
        return _enqueue_scaled(self.h, self.iw, self.ih, fmt, planes, pitches, scale, on_device, pinned)

    def poll(self, ids=False):
        """(segments[LS_DTYPE] with the header record, per-pixel segment ids or None) of the oldest frame not yet polled"""
        out = np.zeros(self.N, np.int32) if ids else None
        ptr = lib().rd_detector_poll_segments(self.h, out.ctypes.data if ids else None)
        if not ptr:
            raise RuntimeError("rd_detector_poll_segments returned NULL")
        n = ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int))[0]
        segs = np.frombuffer((ctypes.c_char * (56 * (n + 1))).from_address(ptr), dtype=LS_DTYPE).copy()
        _libc.free(ptr)
        return segs, out

    def drain(self):
        lib().rd_detector_drain(self.h)

    def counter(self, which):
        return lib().rd_detector_counter(self.h, which)

    def plane(self, name, dtype=np.int32, count=None):
        count = self.N if count is None else count
        out = np.zeros(count, dtype)
        if lib().rd_detector_debug_plane(self.h, name.encode(), out.ctypes.data, out.nbytes) == 0:
            raise KeyError(name)
        return out

    def close(self):
        if self.h:
            lib().rd_detector_destroy(self.h)
            self.h = None


def rect_quads(rects):
    """the quads (n x 4 x 2 doubles) of a RECT_DTYPE array in patch order (rd_rect_quads: c2[0], c2[3], c2[2], c2[1] - s runs clockwise on screen from c2[0])"""
    a = np.ascontiguousarray(rects, dtype=RECT_DTYPE).reshape(-1)
    out = np.zeros((len(a), 4, 2), np.float64)
    lib().rd_rect_quads(a.ctypes.data, len(a), out.ctypes.data)
    return out


def rect_aspect(rect):
    """|c3[0]-c3[1]| / |c3[1]-c3[2]| of one rectangle (rd_rect_aspect): HEIGHT / WIDTH of its estimated pose in the orientation of rect_quads (ph = pw * aspect), for picking a patch shape"""
    a = np.ascontiguousarray(rect, dtype=RECT_DTYPE).reshape(-1)[:1]
    return float(lib().rd_rect_aspect(a.ctypes.data))


def rectify_coefficients(quad):
    """(coefficients a..h as 8 doubles, status) of one quad - what a job uploads (rd_rectify_coefficients; host only)"""
    q = np.ascontiguousarray(quad, dtype=np.float64).reshape(8)
    coef, status = np.zeros(8, np.float64), ctypes.c_int(0)
    lib().rd_rectify_coefficients(q.ctypes.data, coef.ctypes.data, ctypes.byref(status))
    return coef, status.value


class _Service:
    """what Rectifier, Annotator and Compositor share: a handle made by rd_<name>_create whose jobs are waited for oldest first"""
    _name = None

    def _create(self, *args, ctor="create"):
        L = lib()
        if L.rd_device_count() <= 0:
            raise RuntimeError("rectdetect_amd: no HIP device visible - there is no CPU fallback")
        self._wait_fn, self._destroy_fn = getattr(L, "rd_%s_wait" % self._name), getattr(L, "rd_%s_destroy" % self._name)
        self.h = getattr(L, "rd_%s_%s" % (self._name, ctor))(*args)
        if not self.h:
            raise ValueError("rd_%s_%s: invalid arguments (%r)" % (self._name, ctor, args))

    def _wait(self, nstatus=None):
        """blocks until the oldest job is done: its number of items, or with nstatus - the most a job takes - their status bytes"""
        if nstatus is None:
            n = out = self._wait_fn(self.h)
        else:
            status = np.zeros(nstatus, np.uint8)
            n = self._wait_fn(self.h, status.ctypes.data)
            out = status[:n].copy()
        if n < 0:
            raise RuntimeError("rd_%s_wait: no job in flight" % self._name)
        return out

    def _through_pinned(self, nbytes, enqueue):
        """the nbytes that one job, waited for, writes to pinned host memory (enqueue(address) makes the job), as a new array"""
        p = lib().rd_host_alloc(nbytes)
        try:
            enqueue(p)
            self.wait()
            return np.frombuffer((ctypes.c_uint8 * nbytes).from_address(p), np.uint8).copy()
        finally:
            lib().rd_host_free(p)

    def _frame_through_pinned(self, frame_bgr, *job):
        """a numpy BGR image after one job (what enqueue takes behind iw, ih), as a new array"""
        a = np.asarray(frame_bgr, dtype=np.uint8)
        ih, iw = a.shape[:2]
        return self._through_pinned(ih * iw * 3, lambda p: self.enqueue(PIX_BGR, a, None, iw, ih, *job, out_planes=(p,), out_pitches=(iw * 3,), out_pinned=True)).reshape(ih, iw, 3)

    def close(self):
        if self.h:
            self._destroy_fn(self.h)
            self.h = None


# one output kind of the Rectifier: the spec's dtype, the C prefix of rd_<prefix>_spec_ok and rd_<prefix>_bytes, the constructor rd_rectifier_<ctor>, whether a job's
# output is opaque rows of (n, patch_bytes) for the kind's *_view to take apart, and what one quad's output is called
_Kind = collections.namedtuple("_Kind", "dtype prefix ctor rows what")
_KINDS = {      # by the Rectifier's keyword
    "tensor": _Kind(TENSOR_SPEC_DTYPE, "rd_tensor", "create_tensor", False, "tensor"),
    "scan": _Kind(SCAN_SPEC_DTYPE, "rd_scan", "create_scan", False, "page"),
    "grade": _Kind(GRADE_SPEC_DTYPE, "rd_grade", "create_grade", True, "records and histogram"),
    "code": _Kind(CODE_SPEC_DTYPE, "rd_code", "create_code", True, "record (48)"),
    "blobs": _Kind(BLOB_SPEC_DTYPE, "rd_blob", "create_blobs", True, "head, records and page"),
}


def _spec_of(kind, spec):
    return np.ascontiguousarray(spec, dtype=_KINDS[kind].dtype).reshape(())


def _spec_fns(kind):
    """(<kind>_spec_ok, <kind>_bytes): the two questions every kind's spec answers without a GPU"""
    k = _KINDS[kind]

    def spec_ok(spec, pw, ph):
        return bool(getattr(lib(), k.prefix + "_spec_ok")(_spec_of(kind, spec).ctypes.data, int(pw), int(ph)))

    def nbytes(spec, pw, ph):
        return int(getattr(lib(), k.prefix + "_bytes")(_spec_of(kind, spec).ctypes.data, int(pw), int(ph)))

    noun = k.prefix[3:]
    spec_ok.__name__, nbytes.__name__ = noun + "_spec_ok", noun + "_bytes"
    spec_ok.__doc__ = "whether a %s spec is legal for pw x ph outputs (%s_spec_ok); runs without a GPU" % (noun, k.prefix)
    nbytes.__doc__ = "the bytes of one quad's %s, 0 for a spec that is not legal (%s_bytes); runs without a GPU" % (k.what, k.prefix)
    return spec_ok, nbytes


def tensor_spec(dtype, layout, channels, oversample=1, scale=(1, 1, 1), bias=(0, 0, 0)):
    """an rd_tensor_spec as a TENSOR_SPEC_DTYPE record: dtype TENSOR_U8 / F16 / BF16 / F32, layout TENSOR_NHWC / NCHW, channels TENSOR_BGR / RGB / GRAY, oversample 1, 2
    or 4, scale and bias per OUTPUT channel (a number: the same for all).  Whether it is legal is decided where it is used (tensor_spec_ok, Rectifier)."""
    s = np.zeros((), TENSOR_SPEC_DTYPE)
    s["dtype"], s["layout"], s["channels"], s["oversample"] = dtype, layout, channels, oversample
    s["scale"], s["bias"] = np.broadcast_to(np.asarray(scale, np.float32), (3,)), np.broadcast_to(np.asarray(bias, np.float32), (3,))
    return s


tensor_spec_ok, tensor_bytes = _spec_fns("tensor")


def tensor_element(spec, c, S):
    """the bytes of one element of channel c from its box sum S (rd_tensor_element: step 4 of the contract); runs without a GPU"""
    out = np.zeros(4, np.uint8)
    n = lib().rd_tensor_element(_spec_of("tensor", spec).ctypes.data, int(c), int(S), out.ctypes.data)
    if n <= 0:
        raise ValueError("rd_tensor_element: invalid arguments (spec %r, channel %r)" % (spec, c))
    return out[:n].tobytes()


def tensor_limits():
    """{"dtypes", "layouts", "channels", "oversamplings"}: the legal values of a spec's fields (rd_tensor_limits); runs without a GPU"""
    a = np.zeros(4, np.int32)
    lib().rd_tensor_limits(a.ctypes.data)
    bits = lambda v: tuple(k for k in range(31) if v >> k & 1)
    return {"dtypes": bits(int(a[0])), "layouts": bits(int(a[1])), "channels": bits(int(a[2])), "oversamplings": tuple(1 << k for k in bits(int(a[3])))}


def scan_spec(mode, radius=15, k=26, d=0, white=230, oversample=1, invert=False):
    """an rd_scan_spec as a SCAN_SPEC_DTYPE record: mode SCAN_FLAT / BILEVEL / BITS, the window's radius, ink where a pixel is darker than (1 - k/256) of its
    neighbourhood's mean by more than d, the value FLAT gives a pixel equal to that mean, oversample 1, 2 or 4, invert for light ink on a dark page.  Whether it is
    legal is decided where it is used (scan_spec_ok, Rectifier)."""
    s = np.zeros((), SCAN_SPEC_DTYPE)
    s["mode"], s["radius"], s["k"], s["d"], s["white"], s["oversample"], s["invert"] = mode, radius, k, d, white, oversample, int(invert)
    return s


scan_spec_ok, scan_bytes = _spec_fns("scan")


def scan_pixel(spec, G0, N, T):
    """(ink, flat) of one pixel from its gray value G0, its window's pixel count N and the window's sum T of the (inverted) values (rd_scan_pixel: steps 3 and 4 of
    the contract); runs without a GPU"""
    out = np.zeros(2, np.uint8)
    if not lib().rd_scan_pixel(_spec_of("scan", spec).ctypes.data, int(G0), int(N), int(T), out.ctypes.data, out.ctypes.data + 1):
        raise ValueError("rd_scan_pixel: invalid arguments (spec %r, G0 %r, N %r, T %r)" % (spec, G0, N, T))
    return int(out[0]), int(out[1])


def scan_limits():
    """{"modes", "oversamplings", "max_radius", "tile_w", "tile_h"}: the legal values of a scan spec's fields and the kernel's tile (rd_scan_limits); runs without a GPU"""
    a = np.zeros(8, np.int32)
    lib().rd_scan_limits(a.ctypes.data)
    bits = lambda v: tuple(k for k in range(31) if v >> k & 1)
    return {"modes": bits(int(a[0])), "oversamplings": tuple(1 << k for k in bits(int(a[1]))), "max_radius": int(a[2]), "tile_w": int(a[3]), "tile_h": int(a[4])}


def grade_spec(cells=4, dark=8, bright=247, edge=64, oversample=1, hist=False):
    """an rd_grade_spec as a GRADE_SPEC_DTYPE record: a cells x cells grid of records (1, 2, 4 or 8), a pixel is black at G <= dark, blown out at G >= bright, on an
    edge at |L| >= edge, oversample 1, 2 or 4, hist for the patch's 256-bin histogram behind the records.  Whether it is legal is decided where it is used
    (grade_spec_ok, Rectifier)."""
    s = np.zeros((), GRADE_SPEC_DTYPE)
    s["cells"], s["dark"], s["bright"], s["edge"], s["oversample"], s["hist"] = cells, dark, bright, edge, oversample, int(hist)
    return s


grade_spec_ok, grade_bytes = _spec_fns("grade")


def grade_cell_of(spec, pw, ph, i, j):
    """the number of the record pixel (i, j) counts in, -1 for a spec that is not legal or a pixel outside the patch (rd_grade_cell_of); runs without a GPU"""
    return int(lib().rd_grade_cell_of(_spec_of("grade", spec).ctypes.data, int(pw), int(ph), int(i), int(j)))


def grade_limits():
    """{"cells", "oversamplings", "max_edge", "tile_w", "tile_h", "cell_bytes", "hist_bytes"}: the legal values of a grade spec's fields, the kernel's tile and the
    sizes of the output's parts (rd_grade_limits); runs without a GPU"""
    a = np.zeros(8, np.int32)
    lib().rd_grade_limits(a.ctypes.data)
    bits = lambda v: tuple(1 << k for k in range(31) if v >> k & 1)
    return {"cells": bits(int(a[0])), "oversamplings": bits(int(a[1])), "max_edge": int(a[2]), "tile_w": int(a[3]), "tile_h": int(a[4]), "cell_bytes": int(a[5]), "hist_bytes": int(a[6])}


def grade_sharpness(cell):
    """the variance of the Laplacian over one GRADE_CELL_DTYPE record, 0.0 for an empty one (rd_grade_sharpness); runs without a GPU"""
    c = np.ascontiguousarray(cell, dtype=GRADE_CELL_DTYPE).reshape(())
    return float(lib().rd_grade_sharpness(c.ctypes.data))


def grade_percentile(hist, num, den=100):
    """the smallest gray value below or at which num / den of a 256-bin histogram's pixels lie, -1 for bad arguments or an empty histogram (rd_grade_percentile);
    runs without a GPU"""
    h = np.ascontiguousarray(hist, dtype=np.uint32).reshape(256)
    return int(lib().rd_grade_percentile(h.ctypes.data, int(num), int(den)))


def grade_view(arr, spec):
    """a grade job's bytes (what Rectifier.rectify returns, or any (n, patch_bytes) uint8 array) as (the records, a GRADE_CELL_DTYPE array of shape (n, cells, cells)
    indexed [quad, cy, cx], the histograms as an (n, 256) uint32 array or None without hist)"""
    c = int(spec["cells"])
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    a = a.reshape(-1, GRADE_CELL_BYTES * c * c + (GRADE_HIST_BYTES if int(spec["hist"]) else 0))
    cells = np.ascontiguousarray(a[:, :GRADE_CELL_BYTES * c * c]).view(GRADE_CELL_DTYPE).reshape(len(a), c, c)
    hist = np.ascontiguousarray(a[:, GRADE_CELL_BYTES * c * c:]).view(np.uint32).reshape(len(a), 256) if int(spec["hist"]) else None
    return cells, hist


def code_spec(n=6, border=1, inset=2, polarity=0, oversample=1, contrast=32, max_border=0, max_hamming=0):
    """an rd_code_spec as a CODE_SPEC_DTYPE record: an n x n payload (3 .. 8) inside `border` rings (1 or 2), the outer inset/8 of every cell ignored (0 .. 3),
    polarity 0 for a dark ring with light ones, 1 for the opposite, oversample 1, 2 or 4; ok asks for hi - lo >= 256 * contrast, at most max_border ring cells
    wrong and - with a dictionary - a Hamming distance of at most max_hamming.  Whether it is legal is decided where it is used (code_spec_ok, Rectifier)."""
    s = np.zeros((), CODE_SPEC_DTYPE)
    s["n"], s["border"], s["inset"], s["polarity"], s["oversample"], s["contrast"], s["max_border"], s["max_hamming"] = n, border, inset, polarity, oversample, contrast, max_border, max_hamming
    return s


def _dict_arg(dictionary):
    return np.zeros(0, np.uint64) if dictionary is None else np.ascontiguousarray(dictionary, dtype=np.uint64).reshape(-1)


code_spec_ok, code_bytes = _spec_fns("code")


def code_cell_of(spec, pw, ph, i, j):
    """(the number of the cell pixel (i, j) lies in, whether it counts); (-1, False) for a spec that is not legal or a pixel outside the patch (rd_code_cell_of);
    runs without a GPU"""
    counted = ctypes.c_int(0)
    cell = int(lib().rd_code_cell_of(_spec_of("code", spec).ctypes.data, int(pw), int(ph), int(i), int(j), ctypes.addressof(counted)))
    return cell, bool(counted.value)


def code_rotate(bits, n, k=1):
    """an n x n payload turned by k quarter turns clockwise (rd_code_rotate); runs without a GPU"""
    return int(lib().rd_code_rotate(int(bits), int(n), int(k)))


def code_limits():
    """{"min_n", "max_n", "max_border", "max_inset", "oversamplings", "max_side", "max_dict", "code_bytes"} (rd_code_limits); runs without a GPU"""
    a = np.zeros(8, np.int32)
    lib().rd_code_limits(a.ctypes.data)
    return {"min_n": int(a[0]), "max_n": int(a[1]), "max_border": int(a[2]), "max_inset": int(a[3]), "oversamplings": tuple(1 << k for k in range(31) if int(a[4]) >> k & 1),
            "max_side": int(a[5]), "max_dict": int(a[6]), "code_bytes": int(a[7])}


def code_distance(dictionary, n):
    """the smallest Hamming distance between two entries in any rotation and between an entry and itself turned - what max_hamming the dictionary bears; 65 for an
    empty one (rd_code_distance); runs without a GPU.  ValueError for an n, a size or an entry that is not legal"""
    d = _dict_arg(dictionary)
    r = int(lib().rd_code_distance(d.ctypes.data if len(d) else None, len(d), int(n)))
    if r < 0:
        raise ValueError("rd_code_distance: invalid arguments (%d entries, n %r)" % (len(d), n))
    return r


def code_dictionary(n, count, min_dist, seed=0, tries=1 << 20):
    """up to `count` codes of n x n bits that keep min_dist from each other in every rotation and from themselves turned, the deterministic greedy choice among
    `tries` splitmix64 candidates of `seed` (rd_code_dictionary): a uint64 array, shorter than count when the tries ran out; runs without a GPU"""
    out = np.zeros(max(int(count), 1), np.uint64)
    r = int(lib().rd_code_dictionary(int(n), int(count), int(min_dist), int(seed) & 0xFFFFFFFFFFFFFFFF, int(tries), out.ctypes.data))
    if r < 0:
        raise ValueError("rd_code_dictionary: invalid arguments (n %r, count %r, min_dist %r, tries %r)" % (n, count, min_dist, tries))
    return out[:r].copy()


def code_render(spec, bits, cell_px=8):
    """the gray image of a code, a (C * cell_px, C * cell_px) uint8 array of 0 and 255 (rd_code_render); runs without a GPU"""
    s = _spec_of("code", spec)
    side = (int(s["n"]) + 2 * int(s["border"])) * int(cell_px)
    out = np.zeros((max(side, 1), max(side, 1)), np.uint8)
    if not 1 <= side <= 12 * 64 or lib().rd_code_render(s.ctypes.data, int(bits), int(cell_px), out.ctypes.data) != side * side:
        raise ValueError("rd_code_render: invalid arguments (spec %r, bits %r, cell_px %r)" % (spec, bits, cell_px))
    return out


def code_upright(quad, rot):
    """the (4, 2) corners from which a patch shows a code upright that was read with rd_code::rot = rot from `quad` (rd_code_upright); runs without a GPU"""
    q = np.ascontiguousarray(quad, dtype=np.float64).reshape(8)
    out = np.zeros(8, np.float64)
    lib().rd_code_upright(q.ctypes.data, int(rot), out.ctypes.data)
    return out.reshape(4, 2)


def code_view(arr):
    """a code job's bytes (what Rectifier.rectify returns, or any (n, 48) uint8 array) as a CODE_DTYPE array of n records"""
    return np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1, CODE_BYTES).view(CODE_DTYPE).reshape(-1)


def blob_spec(radius=15, k=26, d=0, oversample=1, invert=False, connectivity=8, min_area=1, max_area=0, max_blobs=256, page=False):
    """an rd_blob_spec as a BLOB_SPEC_DTYPE record: the ink decision of a scan spec (radius, k, d, oversample, invert; radius 0: a fixed level, ink = G <= k),
    components through 4 or 8 neighbours, kept when min_area <= area (and area <= max_area unless that is 0), at most max_blobs records per quad, page for the
    cleaned page behind them.  Whether it is legal is decided where it is used (blob_spec_ok, Rectifier)."""
    s = np.zeros((), BLOB_SPEC_DTYPE)
    s["radius"], s["k"], s["d"], s["oversample"], s["invert"], s["connectivity"] = radius, k, d, oversample, int(invert), connectivity
    s["min_area"], s["max_area"], s["max_blobs"], s["page"] = min_area, max_area, max_blobs, int(page)
    return s


blob_spec_ok, blob_bytes = _spec_fns("blobs")


def blob_limits():
    """{"connectivities", "oversamplings", "max_radius", "max_blobs", "max_pixels", "tile_w", "tile_h"}: the legal values of a blob spec's fields and the tile kernel's
    tile (rd_blob_limits); runs without a GPU"""
    a = np.zeros(8, np.int32)
    lib().rd_blob_limits(a.ctypes.data)
    bits = lambda v: tuple(k for k in range(31) if v >> k & 1)
    return {"connectivities": bits(int(a[0])), "oversamplings": tuple(1 << k for k in bits(int(a[1]))), "max_radius": int(a[2]), "max_blobs": int(a[3]), "max_pixels": int(a[4]),
            "tile_w": int(a[5]), "tile_h": int(a[6])}


def _bit_pages(bits, pw, ph):
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    rb = (int(pw) + 7) // 8
    if pw < 1 or ph < 1 or b.size == 0 or b.size % (rb * int(ph)):
        raise ValueError("bit pages of %r bytes are not whole pages of %r x %r pixels" % (b.size, pw, ph))
    return b.reshape(-1, int(ph), rb)


def blob_page_host(bits, pw, ph, spec):
    """steps 2-7 of "page components" for one pw x ph page in the SCAN_BITS layout, on the host (rd_blob_page_host): its blob_bytes bytes; runs without a GPU"""
    b, s = _bit_pages(bits, pw, ph), _spec_of("blobs", spec)
    nb = blob_bytes(s, pw, ph)
    out = np.zeros(max(nb, 8) // 8, np.uint64)      # (8-byte aligned)
    if len(b) != 1 or not nb or not lib().rd_blob_page_host(b.ctypes.data, int(pw), int(ph), s.ctypes.data, out.ctypes.data):
        raise ValueError("rd_blob_page_host: invalid arguments (%d pages of %r x %r, spec %r)" % (len(b), pw, ph, spec))
    return out.view(np.uint8)[:nb].copy()


def blob_view(arr, spec, pw, ph):
    """a blobs job's bytes (what Rectifier.rectify returns, or any (n, patch_bytes) uint8 array) as (the heads, a BLOB_HEAD_DTYPE array of n; the records, a BLOB_DTYPE
    array of shape (n, max_blobs) of which the first heads["written"] of a row count; the cleaned pages as an (n, ph, (pw + 7) // 8) uint8 array, or None without page)"""
    s = _spec_of("blobs", spec)
    B, rb = int(s["max_blobs"]), (int(pw) + 7) // 8
    nb = BLOB_HEAD_BYTES + BLOB_BYTES * B + (((rb * int(ph) + 7) & ~7) if int(s["page"]) else 0)
    a = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1, nb)
    heads = np.ascontiguousarray(a[:, :BLOB_HEAD_BYTES]).view(BLOB_HEAD_DTYPE).reshape(-1)
    recs = np.ascontiguousarray(a[:, BLOB_HEAD_BYTES:BLOB_HEAD_BYTES + BLOB_BYTES * B]).view(BLOB_DTYPE).reshape(len(a), B)
    at = BLOB_HEAD_BYTES + BLOB_BYTES * B
    pages = np.ascontiguousarray(a[:, at:at + rb * int(ph)]).reshape(len(a), int(ph), rb) if int(s["page"]) else None
    return heads, recs, pages


def blobs_pages(bits, pw, ph, spec, device=0, guard=0):
    """The component stage alone (rd_blobs_pages_device) on n pages of pw x ph pixels in the SCAN_BITS layout (any array of n * ph * ((pw + 7) // 8) bytes; pad bits are
    ignored): ((n, blob_bytes) uint8, info = {"path", "launches", "memsets", "tiles_x", "tiles_y", "border"}).  guard > 0: the output lies between two runs of that
    many bytes of 0xA5, which must come back untouched.  Needs a GPU."""
    b, s = _bit_pages(bits, pw, ph), _spec_of("blobs", spec)
    n, nb = len(b), blob_bytes(s, pw, ph)
    g = (int(guard) + 7) & ~7
    buf = np.full((n * nb + 2 * g + 7) // 8, 0xA5A5A5A5A5A5A5A5, np.uint64).view(np.uint8)      # (8-byte aligned, like a job's out)
    info = np.zeros(8, np.int32)
    if not nb or lib().rd_blobs_pages_device(int(device), b.ctypes.data, int(pw), int(ph), n, s.ctypes.data, buf.ctypes.data + g, info.ctypes.data) != 0:
        raise ValueError("rd_blobs_pages_device: invalid arguments (%d pages of %r x %r, spec %r)" % (n, pw, ph, spec))
    if g and not (np.all(buf[:g] == 0xA5) and np.all(buf[g + n * nb:] == 0xA5)):
        raise RuntimeError("rd_blobs_pages_device wrote outside its %d bytes" % (n * nb))
    names = ("path", "launches", "memsets", "tiles_x", "tiles_y", "border")
    return buf[g:g + n * nb].reshape(n, nb).copy(), {k: int(v) for k, v in zip(names, info)}


class Rectifier(_Service):
    """The rd_rectifier extension: pw x ph BGR patches of up to max_quads quads per job, njobs jobs in flight (the contract: include/rectdetect_hip.h).  With
    tensor=tensor_spec(...) a job writes model-ready tensors instead ("model-ready tensors" there), with scan=scan_spec(...) scanned pages ("scanned pages"):
    `out` then holds n * patch_bytes bytes of shape(n) and dtype.  With grade=grade_spec(...) a job writes graded quads ("graded quads"): n rows of patch_bytes bytes, 8-byte aligned, which
    grade_view takes apart.  With code=code_spec(...) and dictionary=a uint64 array (or None: raw bits only) a job writes decoded quads ("decoded quads"): n rows of
    48 bytes, 8-byte aligned, which code_view turns into records.  With blobs=blob_spec(...) a job writes page components ("page components"): n rows of patch_bytes
    bytes, 8-byte aligned, which blob_view takes apart."""
    _name = "rectifier"

    def __init__(self, pw, ph, max_quads=64, njobs=2, device=0, tensor=None, scan=None, grade=None, code=None, dictionary=None, blobs=None):
        given = {"tensor": tensor, "scan": scan, "grade": grade, "code": code, "blobs": blobs}
        kinds = [k for k in _KINDS if given[k] is not None]
        if len(kinds) > 1:
            raise ValueError("Rectifier: tensor=, scan=, grade=, code= and blobs= exclude each other")
        if dictionary is not None and code is None:
            raise ValueError("Rectifier: dictionary= goes with code=")
        self.pw, self.ph, self.max_quads, self.njobs = pw, ph, max_quads, njobs
        for k in _KINDS:      # self.tensor, self.scan, self.grade, self.code, self.blobs: the kind's spec, None for every other
            setattr(self, k, None if given[k] is None else _spec_of(k, given[k]).copy())
        self.dictionary = None if code is None else _dict_arg(dictionary).copy()
        self._kind = _KINDS[kinds[0]] if kinds else None      # (None: BGR patches)
        args, ctor = (device, pw, ph, max_quads, njobs), "create"
        if kinds:
            args, ctor = args + (getattr(self, kinds[0]).ctypes.data,), self._kind.ctor
        if code is not None:
            d = self.dictionary
            args += (d.ctypes.data if len(d) else None, len(d))
        self._create(*args, ctor=ctor)

    @property
    def patch_bytes(self):
        """the bytes of one quad's output (rd_rectifier_patch_bytes)"""
        return int(lib().rd_rectifier_patch_bytes(self.h))

    @property
    def dtype(self):
        """the numpy dtype of an element; bfloat16 is reported as its bits, uint16"""
        return TENSOR_NUMPY[int(self.tensor["dtype"])] if self.tensor is not None else np.dtype(np.uint8)

    def shape(self, n):
        """the shape of a job of n quads: (n, ph, pw, C) or, under TENSOR_NCHW, (n, C, ph, pw); scanned pages: (n, ph, pw) or, under SCAN_BITS, (n, ph, (pw + 7) // 8); graded and decoded quads and page components: (n, patch_bytes)"""
        if self._kind is not None and self._kind.rows:
            return (n, self.patch_bytes)
        if self.scan is not None:
            return (n, self.ph, (self.pw + 7) // 8 if int(self.scan["mode"]) == SCAN_BITS else self.pw)
        if self.tensor is None:
            return (n, self.ph, self.pw, 3)
        C = 1 if int(self.tensor["channels"]) == TENSOR_GRAY else 3
        return (n, C, self.ph, self.pw) if int(self.tensor["layout"]) == TENSOR_NCHW else (n, self.ph, self.pw, C)

    def enqueue(self, fmt, planes, pitches, iw, ih, quads, out, on_device=False, pinned=False, out_pinned=False):
        """one job: patches of `quads` (n x 8 or n x 4 x 2 doubles, patch order) from an iw x ih frame in format fmt (PIX_*) into `out`, the ADDRESS of device memory or,
        with out_pinned, of pinned host memory.  planes / pitches as Detector.enqueue_planes: numpy planes (copied before the call returns; pitches may be None), or with
        on_device / pinned their addresses, read in place until the job's wait().  Returns the job's sequence number; ValueError on an argument error (nothing enqueued)."""
        ptrs, pitch_c, kind, pitch, _ = _plane_args(planes, pitches, on_device, pinned)
        q, n = _quads_arg(quads)
        r = lib().rd_rectifier_enqueue(self.h, int(fmt), ptrs, pitch_c, int(iw), int(ih), kind, q.ctypes.data, n, int(out) if out else None, 2 if out_pinned else 1)
        if r == -1:
            raise ValueError("rd_rectifier_enqueue: invalid arguments (format %r, pitches %r, %dx%d, %d quads, out %r)" % (fmt, pitch, iw, ih, n, out))
        return r

    def wait(self):
        """blocks until the oldest job is done: its status array (uint8 per quad: 1 valid, 0 invalid - an all-zero patch)"""
        return self._wait(self.max_quads)

    def rectify(self, frame_bgr, quads):
        """convenience: the (n, ph, pw, 3) patches - with a tensor or a scan spec: the array of shape(n) and dtype - of `quads` from a numpy BGR image, through pinned memory
        (one job, waited for)"""
        a = np.asarray(frame_bgr, dtype=np.uint8)
        q, n = _quads_arg(quads)
        pb = self.patch_bytes
        got = self._through_pinned(max(n, 1) * pb, lambda p: self.enqueue(PIX_BGR, a, None, a.shape[1], a.shape[0], q, p, out_pinned=True))
        return got[:n * pb].view(self.dtype).reshape(self.shape(n))


def annot_limits():
    """{"tile_w", "tile_h", "chunk"} of the annotator's kernel (rd_annot_limits); runs without a GPU"""
    out = np.zeros(4, np.int32)
    lib().rd_annot_limits(out.ctypes.data)
    return {"tile_w": int(out[0]), "tile_h": int(out[1]), "chunk": int(out[2])}


def annot_rects(rects, scale=1, style=None):
    """the six primitives per rectangle of a RECT_DTYPE array in showRect's order (rd_annot_rects); style: 4 x (b, g, r, thickness) by status, None: vidrect.cpp's"""
    a = np.ascontiguousarray(rects, dtype=RECT_DTYPE).reshape(-1)
    out = np.zeros(6 * len(a), PRIM_DTYPE)
    st = None if style is None else np.ascontiguousarray(style, dtype=np.uint8).reshape(16)
    n = lib().rd_annot_rects(a.ctypes.data, len(a), int(scale), None if st is None else st.ctypes.data, out.ctypes.data)
    return out[:n].copy()


def annot_segments(segs, mode=ANNOT_SEG_ALL, scale=1, max_prims=None):
    """the primitives of an LS_DTYPE list WITH its header record (PolylineDetector.poll, Detector.last_segments): ANNOT_SEG_ALL as vidpoly.cpp draws them,
    ANNOT_SEG_CHAINS as poly.cpp does (rd_annot_segments); at most max_prims of them"""
    a = np.ascontiguousarray(segs, dtype=LS_DTYPE).reshape(-1)
    n = lib().rd_annot_segments(a.ctypes.data, int(mode), int(scale), None, 0)
    if max_prims is not None:
        n = min(n, int(max_prims))
    out = np.zeros(n, PRIM_DTYPE)
    lib().rd_annot_segments(a.ctypes.data, int(mode), int(scale), out.ctypes.data, n)
    return out


class Annotator(_Service):
    """The rd_annotator extension: up to max_prims primitives per job drawn into a frame on the device, njobs jobs in flight (the contract: include/rectdetect_hip.h)."""
    _name = "annotator"

    def __init__(self, max_prims=4096, njobs=2, device=0):
        self.max_prims, self.njobs = max_prims, njobs
        self._create(device, max_prims, njobs)

    def enqueue(self, fmt, planes, pitches, iw, ih, prims, flags=0, out_planes=None, out_pitches=None, on_device=False, pinned=False, out_pinned=False):
        """one job: `prims` (PRIM_DTYPE) into an iw x ih frame in format fmt (PIX_*).  planes / pitches as Detector.enqueue_planes: numpy planes (copied before the call
        returns; pitches may be None), or with on_device / pinned their addresses.  out_planes None: in place (device frames only); otherwise the ADDRESSES of the
        destination's planes in device memory or, with out_pinned, in pinned host memory, and their out_pitches.  Returns the job's sequence number; ValueError on an
        argument error (nothing enqueued)."""
        ptrs, pitch_c, kind, pitch, _ = _plane_args(planes, pitches, on_device, pinned)
        p, n = _prims_arg(prims)
        optrs, opitch = _out_args(out_planes, out_pitches)
        r = lib().rd_annotator_enqueue(self.h, int(fmt), ptrs, pitch_c, int(iw), int(ih), kind, p.ctypes.data, n, int(flags), optrs, opitch, 2 if out_pinned else 1)
        if r == -1:
            raise ValueError("rd_annotator_enqueue: invalid arguments (format %r, pitches %r, %dx%d, %d primitives, flags %r)" % (fmt, pitch, iw, ih, n, flags))
        return r

    def wait(self):
        """blocks until the oldest job is done: its number of primitives"""
        return self._wait()

    def annotate(self, frame_bgr, prims, flags=0):
        """convenience: a numpy BGR image with `prims` drawn into it, as a new array, through pinned memory (one job, waited for)"""
        return self._frame_through_pinned(frame_bgr, prims, flags)


def comp_limits():
    """{"tile_w", "tile_h", "chunk"} of the compositor's kernel (rd_comp_limits); runs without a GPU"""
    out = np.zeros(4, np.int32)
    lib().rd_comp_limits(out.ctypes.data)
    return {"tile_w": int(out[0]), "tile_h": int(out[1]), "chunk": int(out[2])}


def comp_items(quads, patch=COMP_FILL, colour=(0, 0, 0)):
    """COMP_ITEM_DTYPE items of `quads` (n x 8 or n x 4 x 2 doubles, patch order: rect_quads makes them).  patch: one number for all or one per quad (COMP_FILL: fill
    with `colour`); colour: one (b, g, r) for all or one per quad"""
    q = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 4, 2)
    out = np.zeros(len(q), COMP_ITEM_DTYPE)
    out["quad"] = q
    out["patch"] = patch
    if len(colour) == 3 and np.ndim(colour[0]) == 0:
        out["b"], out["g"], out["r"] = colour
    else:
        c = np.asarray(colour, np.uint8).reshape(len(q), 3)
        out["b"], out["g"], out["r"] = c[:, 0], c[:, 1], c[:, 2]
    return out


def composite_coefficients(quad, iw, ih):
    """(the adjugate A..I as 9 doubles, the pixel box bx0, by0, bx1, by1 as 4 ints, status) of one quad in an iw x ih frame - what a job uploads
    (rd_composite_coefficients; host only)"""
    q = np.ascontiguousarray(quad, dtype=np.float64).reshape(8)
    inv, box, status = np.zeros(9, np.float64), np.zeros(4, np.int32), ctypes.c_int(0)
    lib().rd_composite_coefficients(q.ctypes.data, int(iw), int(ih), inv.ctypes.data, box.ctypes.data, ctypes.byref(status))
    return inv, box, status.value


def composite_covers(quad, iw, ih, x, y):
    """(covered?, s, t) of pixel (x, y) of an iw x ih frame under one quad (rd_composite_covers; host only)"""
    q = np.ascontiguousarray(quad, dtype=np.float64).reshape(8)
    st = np.zeros(2, np.float64)
    c = lib().rd_composite_covers(q.ctypes.data, int(iw), int(ih), int(x), int(y), st.ctypes.data)
    return bool(c), float(st[0]), float(st[1])


def composite_tiles(items, iw, ih):
    """the (m, 2) int32 tiles tx, ty an in-place job of `items` launches, in raster order (rd_composite_tiles; host only)"""
    it, n = _items_arg(items)
    m = lib().rd_composite_tiles(it.ctypes.data, n, int(iw), int(ih), None, 0)
    if m < 0:
        raise ValueError("rd_composite_tiles: invalid arguments (%d items, %dx%d)" % (n, iw, ih))
    out = np.zeros((m, 2), np.int32)
    lib().rd_composite_tiles(it.ctypes.data, n, int(iw), int(ih), out.ctypes.data, m)
    return out


class Compositor(_Service):
    """The rd_compositor extension: up to max_items quads per job filled with a colour or pasted with a pw x ph BGR patch, in a frame on the device, njobs jobs in
    flight (the contract: include/rectdetect_hip.h)."""
    _name = "compositor"

    def __init__(self, pw=64, ph=64, max_items=256, njobs=2, device=0):
        self.pw, self.ph, self.max_items, self.njobs = pw, ph, max_items, njobs
        self._create(device, pw, ph, max_items, njobs)

    def _patches(self, patches, patches_on_device, patches_pinned):
        """(pointer, number of patches, kind, array to keep alive) of a job's patch array: None, a numpy (n, ph, pw, 3) uint8 array (copied before the call returns), or
        with patches_on_device / patches_pinned an (ADDRESS, n) pair"""
        if patches is None:
            return None, 0, 0, None
        if patches_on_device or patches_pinned:
            addr, n = patches
            return (int(addr) if addr else None), int(n), 1 if patches_on_device else 2, None
        a = np.ascontiguousarray(patches, dtype=np.uint8)
        if a.ndim != 4 or a.shape[3] != 3:
            raise ValueError("composite: host patches are an (n, ph, pw, 3) uint8 array, not %r" % (a.shape,))
        if a.shape[1:] != (self.ph, self.pw, 3):
            raise ValueError("composite: patches of shape %r for a compositor of %dx%d patches" % (a.shape, self.pw, self.ph))
        return a.ctypes.data, len(a), 0, a

    def enqueue(self, fmt, planes, pitches, iw, ih, items, patches=None, out_planes=None, out_pitches=None, on_device=False, pinned=False, out_pinned=False,
                patches_on_device=False, patches_pinned=False):
        """one job: `items` (COMP_ITEM_DTYPE) into an iw x ih frame in format fmt (PIX_*).  planes / pitches as Detector.enqueue_planes: numpy planes (copied before the
        call returns; pitches may be None), or with on_device / pinned their addresses.  patches: None (fills only), a numpy (n, ph, pw, 3) uint8 array (copied before
        the call returns), or with patches_on_device / patches_pinned an (ADDRESS, n) pair.  out_planes None: in place (device frames only); otherwise the ADDRESSES of
        the destination's planes in device memory or, with out_pinned, in pinned host memory, and their out_pitches.  Returns the job's sequence number; ValueError on
        an argument error (nothing enqueued)."""
        ptrs, pitch_c, kind, pitch, _ = _plane_args(planes, pitches, on_device, pinned)
        it, n = _items_arg(items)
        pp, npatches, pkind, _ = self._patches(patches, patches_on_device, patches_pinned)
        optrs, opitch = _out_args(out_planes, out_pitches)
        r = lib().rd_compositor_enqueue(self.h, int(fmt), ptrs, pitch_c, int(iw), int(ih), kind, it.ctypes.data, n, pp, npatches, pkind, optrs, opitch, 2 if out_pinned else 1)
        if r == -1:
            raise ValueError("rd_compositor_enqueue: invalid arguments (format %r, pitches %r, %dx%d, %d items, %d patches)" % (fmt, pitch, iw, ih, n, npatches))
        return r

    def wait(self):
        """blocks until the oldest job is done: its status array (uint8 per item: 1 valid, 0 invalid - nothing written)"""
        return self._wait(self.max_items)

    def composite(self, frame_bgr, items, patches=None):
        """convenience: a numpy BGR image with `items` composited into it, as a new array, through pinned memory (one job, waited for)"""
        return self._frame_through_pinned(frame_bgr, items, patches)


def match_limits():
    """{"grids", "oversamplings", "max_templates", "max_quads"} of the matcher (rd_match_limits); runs without a GPU"""
    out = np.zeros(4, np.int32)
    lib().rd_match_limits(out.ctypes.data)
    bits = lambda v: tuple(1 << k for k in range(31) if v >> k & 1)
    return {"grids": bits(int(out[0])), "oversamplings": bits(int(out[1])), "max_templates": int(out[2]), "max_quads": int(out[3])}


def match_score(rec, grid, sb, sbb, sb2=0, sbb2=0):
    """a MATCH_DTYPE record completed on the host (rd_match_score): score and score2 from its integers and the sums of the best column and of the runner-up's; a
    record whose status is not 1 gets every other field zeroed.  Returns a new record; runs without a GPU"""
    r = np.array(rec, dtype=MATCH_DTYPE).reshape(1).copy()
    lib().rd_match_score(r.ctypes.data, int(grid), int(sb), int(sbb), int(sb2), int(sbb2))
    return r[0]


class Matcher(_Service):
    """The rd_matcher extension: a library of up to max_templates templates, up to max_quads quads per job scored against it on the device, njobs jobs in flight
    (the contract: include/rectdetect_hip.h, "matched quads")."""
    _name = "matcher"

    def __init__(self, grid=32, oversample=4, max_templates=64, max_quads=64, njobs=2, device=0):
        self.grid, self.oversample, self.max_templates, self.max_quads, self.njobs = grid, oversample, max_templates, max_quads, njobs
        self._jobs = []      # (n, T at enqueue, flags) of the jobs in flight, oldest first: what wait() needs to size its arrays
        self._create(device, grid, oversample, max_templates, max_quads, njobs)

    def templates(self):
        return lib().rd_matcher_templates(self.h)

    def add(self, fmt, planes, pitches, iw, ih, quad=None, on_device=False, pinned=False):
        """a template from `quad` (8 doubles, patch order; None: the whole image) of an iw x ih image in format fmt (planes / pitches as Detector.enqueue_planes): its
        number.  ValueError on an argument error or a full library, ArithmeticError for a flat template or an invalid quad (nothing added)."""
        ptrs, pitch_c, kind, pitch, _ = _plane_args(planes, pitches, on_device, pinned)
        q = None if quad is None else np.ascontiguousarray(quad, dtype=np.float64).reshape(8)
        r = lib().rd_matcher_add(self.h, int(fmt), ptrs, pitch_c, int(iw), int(ih), kind, None if q is None else q.ctypes.data)
        if r == -1:
            raise ValueError("rd_matcher_add: invalid arguments or a full library (format %r, pitches %r, %dx%d, %d templates)" % (fmt, pitch, iw, ih, self.templates()))
        if r == -2:
            raise ArithmeticError("rd_matcher_add: a flat template or an invalid quad")
        return r

    def add_image(self, image_bgr, quad=None):
        """convenience: add() of a numpy BGR image"""
        a = np.asarray(image_bgr, dtype=np.uint8)
        return self.add(PIX_BGR, a, None, a.shape[1], a.shape[0], quad)

    def signature(self, tmpl, rot=0):
        """test tap: (the grid x grid int8 signature of column 4 * tmpl + rot, sb, sbb) (rd_matcher_signature)"""
        out, sums = np.zeros((self.grid, self.grid), np.int8), np.zeros(2, np.int32)
        if lib().rd_matcher_signature(self.h, int(tmpl), int(rot), out.ctypes.data, sums.ctypes.data) != 0:
            raise IndexError("rd_matcher_signature: no column %r, %r" % (tmpl, rot))
        return out, int(sums[0]), int(sums[1])

    def enqueue(self, fmt, planes, pitches, iw, ih, quads, flags=0, on_device=False, pinned=False):
        """one job: the records of `quads` (n x 8 or n x 4 x 2 doubles, patch order) of an iw x ih frame in format fmt (PIX_*).  planes / pitches as
        Detector.enqueue_planes: numpy planes (copied before the call returns; pitches may be None), or with on_device / pinned their addresses, read in place until the
        job's wait().  flags: MATCH_DOTS keeps the dot matrix.  Returns the job's sequence number; ValueError on an argument error (nothing enqueued)."""
        ptrs, pitch_c, kind, pitch, _ = _plane_args(planes, pitches, on_device, pinned)
        q, n = _quads_arg(quads)
        r = lib().rd_matcher_enqueue(self.h, int(fmt), ptrs, pitch_c, int(iw), int(ih), kind, q.ctypes.data, n, int(flags))
        if r == -1:
            raise ValueError("rd_matcher_enqueue: invalid arguments (format %r, pitches %r, %dx%d, %d quads, flags %r)" % (fmt, pitch, iw, ih, n, flags))
        self._jobs.append((n, self.templates(), int(flags)))
        return r

    def wait(self, dots=False):
        """blocks until the oldest job is done: its MATCH_DTYPE records; with dots=True (a job enqueued with MATCH_DOTS) also its (n, 4T) int32 dot matrix"""
        if not self._jobs:
            raise RuntimeError("rd_matcher_wait: no job in flight")
        n, T, flags = self._jobs.pop(0)
        recs = np.zeros(max(n, 1), MATCH_DTYPE)
        want = dots and (flags & MATCH_DOTS)
        d = np.zeros((max(n, 1), max(4 * T, 1)), np.int32) if want else None
        got = lib().rd_matcher_wait(self.h, recs.ctypes.data, d.ctypes.data if want else None)
        if got != n:
            raise RuntimeError("rd_matcher_wait: %d records, expected %d" % (got, n))
        return (recs[:n], d[:n, :4 * T] if want else None) if dots else recs[:n]

    def match(self, frame_bgr, quads):
        """convenience: the records of `quads` in a numpy BGR image (one job, waited for)"""
        a = np.asarray(frame_bgr, dtype=np.uint8)
        self.enqueue(PIX_BGR, a, None, a.shape[1], a.shape[0], quads)
        return self.wait()


def lens(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    """an rd_lens as a LENS_DTYPE record: the SOURCE camera, with the Brown-Conrady coefficients in OpenCV's order"""
    return np.array((fx, fy, cx, cy, k1, k2, p1, p2, k3), LENS_DTYPE)


def view(fx, fy, cx, cy):
    """an rd_view as a VIEW_DTYPE record: the ideal camera of the OUTPUT"""
    return np.array((fx, fy, cx, cy), VIEW_DTYPE)


def _lens_arg(l):
    return np.ascontiguousarray(l, dtype=LENS_DTYPE).reshape(())


def _view_arg(v):
    """a view, or a lens whose fx, fy, cx, cy the view takes"""
    if getattr(v, "dtype", None) == LENS_DTYPE:
        return view(*(float(np.asarray(v)[n]) for n in ("fx", "fy", "cx", "cy")))
    return np.ascontiguousarray(v, dtype=VIEW_DTYPE).reshape(())


def _maps_arg(mapx, mapy, ow, oh):
    mx, my = np.ascontiguousarray(mapx, dtype=np.float32), np.ascontiguousarray(mapy, dtype=np.float32)
    if mx.size != ow * oh or my.size != ow * oh:
        raise ValueError("remap: maps of %d and %d values for an output of %dx%d" % (mx.size, my.size, ow, oh))
    return mx, my


def remap_points(lens, view, uv):
    """the source positions (n, 2) of output points uv (n, 2) under a lens and a view (rd_remap_points); runs without a GPU"""
    l, v = _lens_arg(lens), _view_arg(view)
    p = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    out = np.zeros_like(p)
    lib().rd_remap_points(l.ctypes.data, v.ctypes.data, p.ctypes.data, len(p), out.ctypes.data)
    return out


def remap_table_lens(lens, view, ow, oh, iw, ih):
    """(the (oh, ow, 2) int32 table xi, yi of an ow x oh output from an iw x ih source, its number of inside entries) (rd_remap_table_lens); runs without a GPU"""
    l, v = _lens_arg(lens), _view_arg(view)
    table = np.zeros((max(int(oh), 0), max(int(ow), 0), 2), np.int32)
    n = lib().rd_remap_table_lens(l.ctypes.data, v.ctypes.data, int(ow), int(oh), int(iw), int(ih), table.ctypes.data)
    if n < 0:
        raise ValueError("rd_remap_table_lens: invalid arguments (lens %r, view %r, %dx%d from %dx%d)" % (l, v, ow, oh, iw, ih))
    return table, n


def remap_table_map(mapx, mapy, ow, oh, iw, ih):
    """the same from a caller's float32 maps of ow * oh values each (rd_remap_table_map); runs without a GPU"""
    mx, my = _maps_arg(mapx, mapy, ow, oh)
    table = np.zeros((int(oh), int(ow), 2), np.int32)
    n = lib().rd_remap_table_map(mx.ctypes.data, my.ctypes.data, int(ow), int(oh), int(iw), int(ih), table.ctypes.data)
    if n < 0:
        raise ValueError("rd_remap_table_map: invalid arguments (%dx%d from %dx%d)" % (ow, oh, iw, ih))
    return table, n


def view_tan_aov(view, ow):
    """the tan_aov to poll with for ow-wide frames made with this view (rd_view_tan_aov); runs without a GPU"""
    return float(lib().rd_view_tan_aov(_view_arg(view).ctypes.data, int(ow)))


def remap_limits():
    """{"min_out", "max_out", "min_src", "max_src"}: the smallest and largest side of an output and of a source (rd_remap_limits); runs without a GPU"""
    a = np.zeros(4, np.int32)
    lib().rd_remap_limits(a.ctypes.data)
    return {"min_out": int(a[0]), "max_out": int(a[1]), "min_src": int(a[2]), "max_src": int(a[3])}


class Remapper(_Service):
    """The rd_remapper extension: ow x oh BGR frames as an ideal camera would have seen them, from iw x ih source frames in any pixel format, njobs jobs in flight
    (the contract: include/rectdetect_hip.h, "remapped frames").  Either lens (and view: None takes the lens's fx, fy, cx, cy) or maps=(mapx, mapy), float32."""
    _name = "remapper"

    def __init__(self, ow, oh, iw, ih, lens=None, view=None, maps=None, njobs=2, device=0):
        self.ow, self.oh, self.iw, self.ih, self.njobs = ow, oh, iw, ih, njobs
        if (lens is None) == (maps is None):
            raise ValueError("Remapper: either a lens or maps")
        if maps is not None:
            mx, my = _maps_arg(maps[0], maps[1], ow, oh)
            self._create(device, mx.ctypes.data, my.ctypes.data, ow, oh, iw, ih, njobs, ctor="create_map")
        else:
            l = _lens_arg(lens)
            v = _view_arg(l if view is None else view)
            self._create(device, l.ctypes.data, v.ctypes.data, ow, oh, iw, ih, njobs, ctor="create_lens")

    @property
    def inside(self):
        """the entries of the table that are inside the source (rd_remapper_inside)"""
        return int(lib().rd_remapper_inside(self.h))

    def enqueue(self, fmt, planes, pitches, on_device, out, out_pitch, fill=(0, 0, 0), pinned=False, out_pinned=False):
        """one job: the ow x oh frame of an iw x ih source in format fmt (PIX_*) into `out` - the ADDRESS of device memory (the data_ptr() of a torch tensor will do)
        or, with out_pinned, of pinned host memory - with rows out_pitch bytes apart; outside pixels get fill = (b, g, r).  planes / pitches as
        Detector.enqueue_planes: numpy planes (copied before the call returns; pitches may be None), or with on_device / pinned their addresses, read in place until the
        job's wait().  Returns the job's sequence number; ValueError on an argument error (nothing enqueued)."""
        if on_device == 2:      # (RD_FRAME_HOST_PINNED by its number)
            on_device, pinned = False, True
        ptrs, pitch_c, kind, pitch, _ = _plane_args(planes, pitches, on_device, pinned)
        b, g, r = (int(c) & 255 for c in fill)
        seq = lib().rd_remapper_enqueue(self.h, int(fmt), ptrs, pitch_c, kind, b | g << 8 | r << 16, int(out) if out else None, int(out_pitch), 2 if out_pinned else 1)
        if seq == -1:
            raise ValueError("rd_remapper_enqueue: invalid arguments (format %r, pitches %r, out %r, out_pitch %r)" % (fmt, pitch, out, out_pitch))
        return seq

    def wait(self):
        """blocks until the oldest job is done"""
        self._wait()

    def remap(self, frame_bgr, fill=(0, 0, 0)):
        """convenience: the (oh, ow, 3) output of a numpy BGR image, as a new array, through pinned memory (one job, waited for)"""
        a = np.asarray(frame_bgr, dtype=np.uint8)
        return self._through_pinned(self.oh * self.ow * 3, lambda p: self.enqueue(PIX_BGR, a, None, False, p, self.ow * 3, fill, out_pinned=True)).reshape(self.oh, self.ow, 3)


def postprocess_planes(segs, boundary, table, iw, ih, tan_aov):
    """Host post-process alone (oclrect.c:1049-1226 restated in csrc/rd_post.c) on full planes; runs without a GPU."""
    segs = np.ascontiguousarray(segs)
    boundary = np.ascontiguousarray(boundary, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.int32)
    return _take_rects(lib().rd_postprocess_planes(segs.ctypes.data, boundary.ctypes.data, table.ctypes.data, iw, ih, float(tan_aov)))


POST_LIMIT_NAMES = ("POST_HT", "POST_MAXG", "POST_MAXC", "POST_MEMBERS", "POST_CAP", "POST_WAVES", "RDP_HULL_DEPTH", "RDP_HULL_POOL")


def post_device_limits():
    """The fixed capacities of the device post-process (rd_post_device_limits) by name; runs without a GPU."""
    out = np.zeros(8, np.int32)
    lib().rd_post_device_limits(out.ctypes.data)
    return dict(zip(POST_LIMIT_NAMES, (int(v) for v in out)))


def postprocess_planes_device(segs, boundary, table, iw, ih, tan_aov, device=0):
    """Device post-process alone (rd_k_post.hip) on full planes: (rectangles, info).  rectangles is the list as a poll assembles it, or None when the device
    flagged an overflow; info[0] = candidates counted, info[1] = the overflow word.  Needs a GPU."""
    segs = np.ascontiguousarray(segs)
    boundary = np.ascontiguousarray(boundary, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.int32)
    info = np.zeros(8, np.int32)
    ptr = lib().rd_postprocess_planes_device(int(device), segs.ctypes.data, boundary.ctypes.data, table.ctypes.data, iw, ih, float(tan_aov), info.ctypes.data)
    return (_take_rects(ptr) if ptr else None), info


POLY_LIMIT_NAMES = ("PP_LIVE", "PP_MAXSEG", "PP_MAXCAND", "PP_ID_BITS")


def polyline_limits():
    """The fixed capacities of the polyline stage's single-block kernel (rd_polyline_limits) by name; runs without a GPU."""
    out = np.zeros(4, np.int32)
    lib().rd_polyline_limits(out.ctypes.data)
    return dict(zip(POLY_LIMIT_NAMES, (int(v) for v in out)))


def polyline_planes_device(mask, ring_nonzero, minerror, size_thre, lslist_bytes=None, form=0, device=0):
    """The polyline stage alone (rd_polyline_planes_device) on a 2-D mask: (list, ids, ctr).  form 0 = multi-launch, 1 = the single-block kernel, which does
    not fall back: ctr[25] != 0 says it gave up.  list holds the header and the records lslist_bytes has room for (default: 16 bytes per pixel).  Needs a GPU."""
    mask = np.ascontiguousarray(mask, dtype=np.int32)
    ih, iw = mask.shape
    nbytes = iw * ih * 16 if lslist_bytes is None else int(lslist_bytes)
    raw = np.zeros((nbytes + 3) // 4, np.int32)
    ids = np.zeros(iw * ih, np.int32)
    ctr = np.zeros(64, np.int32)
    if lib().rd_polyline_planes_device(int(device), mask.ctypes.data, iw, ih, int(ring_nonzero), float(minerror), int(size_thre), nbytes, int(form),
                                       raw.ctypes.data, ids.ctypes.data, ctr.ctypes.data) != 0:
        raise ValueError("rd_polyline_planes_device: invalid arguments")
    n = min(int(raw[0]), nbytes // 56 - 1)
    return raw[: 14 * (max(n, 0) + 1)].view(LS_DTYPE).copy(), ids, ctr


VOTES_LIMIT_NAMES = ("RB_MAX", "CA_T", "CA_PROBES", "BA_T", "BA_PROBES", "block", "grid", "MAXB", "CLAIM_NONE", "PACK_FLAGS", "PACK_FLAGS_INTS", "PACK_STATUS", "PACK_STATUS_INTS",
                     "RFLAGS_STATUS_AT", "PACK_RECORDS", "REC_INTS", "PROBE_INTS")
VOTES_RFLAGS_INTS = 256


def votes_limits():
    """The constants the vote stage's crafted cases are placed by (rd_votes_limits) by name; runs without a GPU."""
    out = np.zeros(24, np.int32)
    lib().rd_votes_limits(out.ctypes.data)
    return dict(zip(VOTES_LIMIT_NAMES, (int(v) for v in out)))


class VotesFrame:
    """What rd_votes_planes_device returns for one frame of one step: ids (2-D), segs (header + records, LS_DTYPE), list_ints (the whole list buffer), ctr (64), table
    (nentry x 5), tlist (the entries, tlist[0] of them), claim (nentry), probes and pack (every int of the buffers, guard words included)."""

    def __init__(self, shape, ids, raw, ctr, table, tlist, claim, probes, pack):
        self.ids, self.list_ints, self.ctr, self.table, self.claim, self.probes, self.pack = ids.reshape(shape), raw, ctr, table.reshape(-1, 5), claim, probes, pack
        n = min(max(int(raw[0]), 0), raw.size // 14 - 1)
        self.segs = raw[: 14 * (n + 1)].view(LS_DTYPE).copy()
        self.tlist_count = int(tlist[0])
        self.tlist = tlist[1: 1 + min(max(self.tlist_count, 0), tlist.size - 1)].copy()


def votes_planes_device(steps, clean=0, max_records=64, pack_records=64, rflags=None, guard=0x5a5a5a5a, probes_ints=None, pack_ints=None, device=0):
    """The vote stage through the frame path's calls (rd_votes_planes_device).  steps = [dict(frames=[(mask, boundary), ...], ring=0/1, minerror=, size_thre=, form=0/1)], every
    step with the same number of frames, every plane 2-D and of one size; frame z keeps its tables from step to step.  rflags: (frames, 256) ints.  probes_ints / pack_ints
    default to what max_records / pack_records need plus 256 guard words.  Returns [[VotesFrame per frame] per step].  Needs a GPU."""
    lim = votes_limits()
    nsteps, nb = len(steps), len(steps[0]["frames"])
    if any(len(s["frames"]) != nb for s in steps):
        raise ValueError("votes_planes_device: every step takes the same number of frames")
    masks = np.ascontiguousarray([[np.asarray(m, dtype=np.int32) for m, _ in s["frames"]] for s in steps], dtype=np.int32)
    bounds = np.ascontiguousarray([[np.asarray(b, dtype=np.int32) for _, b in s["frames"]] for s in steps], dtype=np.int32)
    if masks.ndim != 4 or masks.shape != bounds.shape:
        raise ValueError("votes_planes_device: planes of different sizes")
    ih, iw = masks.shape[2:]
    n, k = iw * ih, nsteps * nb
    nentry = n * 4 // 5
    ring = np.array([int(s.get("ring", 0)) for s in steps], np.int32)
    minerror = np.array([float(s.get("minerror", 1.0)) for s in steps], np.float32)
    size_thre = np.array([int(s.get("size_thre", 10)) for s in steps], np.int32)
    form = np.array([int(s.get("form", 0)) for s in steps], np.int32)
    rf = np.zeros((nb, VOTES_RFLAGS_INTS), np.int32) if rflags is None else np.ascontiguousarray(rflags, dtype=np.int32)
    if rf.shape != (nb, VOTES_RFLAGS_INTS):
        raise ValueError("votes_planes_device: rflags is (frames, %d) ints" % VOTES_RFLAGS_INTS)
    if probes_ints is None:
        probes_ints = max(int(max_records), 0) * lim["PROBE_INTS"] + 256
    if pack_ints is None:
        pack_ints = lim["PACK_RECORDS"] + max(int(pack_records), 0) * (lim["REC_INTS"] + lim["PROBE_INTS"]) + 256
    guard = int(np.array([guard & 0xFFFFFFFF], np.uint32).view(np.int32)[0])
    ids, raw, ctr = np.zeros((k, n), np.int32), np.zeros((k, n * 4), np.int32), np.zeros((k, 64), np.int32)
    table, tlist, claim = np.zeros((k, nentry * 5), np.int32), np.zeros((k, nentry + 1), np.int32), np.zeros((k, nentry), np.int32)
    probes, pack = np.zeros((k, int(probes_ints)), np.int32), np.zeros((k, int(pack_ints)), np.int32)
    if lib().rd_votes_planes_device(int(device), iw, ih, nsteps, nb, masks.ctypes.data, bounds.ctypes.data, ring.ctypes.data, minerror.ctypes.data, size_thre.ctypes.data,
                                    form.ctypes.data, int(clean), int(max_records), int(pack_records), rf.ctypes.data, guard, int(probes_ints), int(pack_ints),
                                    ids.ctypes.data, raw.ctypes.data, ctr.ctypes.data, table.ctypes.data, tlist.ctypes.data, claim.ctypes.data, probes.ctypes.data,
                                    pack.ctypes.data) != 0:
        raise ValueError("rd_votes_planes_device: invalid arguments")
    return [[VotesFrame((ih, iw), *(a[s * nb + z] for a in (ids, raw, ctr, table, tlist, claim, probes, pack))) for z in range(nb)] for s in range(nsteps)]


REGION_INFO_INTS = 144


def region_limits(iw=0, ih=0):
    """The constants of the region stage that crafted planes are built from (rd_region_limits) by name; slow_bound and reccap are those of an iw x ih frame.
    Runs without a GPU."""
    out = np.zeros(32, np.int32)
    lib().rd_region_limits(int(iw), int(ih), out.ctypes.data)
    v = [int(x) for x in out]
    return {"first_budget": v[0], "ladder": [b for b in v[1:5] if b], "max_launches": v[5], "AT_CAP": v[6], "AT_SWEEPS": v[7], "AT_NT": v[8], "AB_HK": v[9], "AB_OWNED": v[10],
            "merge_tile": (v[11], v[12]), "absorb_tile": (v[13], v[14]), "thre": v[15], "slow_bound": v[16], "reccap": v[17], "tile_rounds": v[18],
            "EPT": [e for e in v[19:26] if e], "size_bits": v[26]}


class RegionPlanes:
    """What rd_region_planes_device returns: the five planes (2-D) and the info block by name."""

    def __init__(self, shape, planes, info):
        self.region0, self.rsize, self.region, self.boundarysrc, self.boundary = (p.reshape(shape) for p in planes)
        m = 128
        self.info = info
        self.budget, self.settled = int(info[m]), bool(info[m + 1])
        self.flags = info[: self.budget].copy()
        self.status = [int(v) for v in info[m + 2: m + 6]]
        self.slow, self.slow_launches = bool(info[m + 6]), int(info[m + 7])


def region_planes_device(pix=None, mask=None, edge=None, launches=0, region0=None, rsize=None, force_slow=False, device=0):
    """The region stage alone (rd_region_planes_device) on 2-D planes: stage 0 from (pix, mask, edge) with a budget of `launches` (0: as the frame path does), or
    stage 1 from (region0, rsize).  Returns a RegionPlanes.  Needs a GPU."""
    stage = 0 if region0 is None else 1
    ins = [np.ascontiguousarray(a, dtype=np.int32) for a in ((pix, mask, edge) if stage == 0 else (region0, rsize))]
    ih, iw = ins[0].shape
    n = iw * ih
    if any(a.size != n for a in ins):
        raise ValueError("region_planes_device: planes of different sizes")
    outs = [np.zeros(n, np.int32) for _ in range(5)]
    info = np.zeros(REGION_INFO_INTS, np.int32)
    z = [None] * 3
    args = ([a.ctypes.data for a in ins] + [int(launches), None, None]) if stage == 0 else (z + [0] + [a.ctypes.data for a in ins])
    if lib().rd_region_planes_device(int(device), stage, iw, ih, *args, int(bool(force_slow)), *[o.ctypes.data for o in outs], info.ctypes.data) != 0:
        raise ValueError("rd_region_planes_device: invalid arguments")
    return RegionPlanes((ih, iw), outs, info)
