#!/usr/bin/env python3
"""What the reference itself (oracle/_ref: its kernels and host C on the serial OpenCL shim) returns for the three CPU checks that used to run it live
(tests/test_cpu_oracle.py: test_oracle_against_live_reference_new_seed, test_concurrent_merge_restatement_equals_the_references_own_kernel,
test_host_postprocess_equals_the_references_own_compiled_host_code), so that those checks run from the repository alone.

-> tests/golden/ref_checks.npz:
     new_seed_*                  320x240, seed SEED0 + 11, frame 3: input CRC, CRC of every plane the reference computed (the oracle's plane names), its rect_t list
     merge_<case>_f<t>_*         labelMergeMain with concurrent work-items (rdcl_set_order group order 5): CRC of region, rsize and boundary, and the rect_t list
     post_<case>_m<mode>_f<t>_*  the reference's own compiled executeCPUTask on the oracle's planes (mode: helpers.REGION_*): CRC of the planes it was given and,
                                 per aperture, its rect_t list
Only runs where the reference build oracle/_ref exists.  usage: python tools/make_golden_refchecks.py"""
import ctypes
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rectdetect_amd as ra  # noqa: E402,F401
from rectdetect_amd import synth  # noqa: E402
from tests import helpers  # noqa: E402

NEW_SEED_PLANES = ["plab0", "Lblur", "plab1", "vxy", "strength", "nms", "tidy", "str_sum", "smooth", "quant", "strong", "mergemask", "region", "boundary", "lsid", "table"]
MERGE_CASES = [(333, 217, 2, 2), (640, 480, 0, 2)]
POST_CASES = [(333, 217, 2, 2), (640, 480, 5, 2), (640, 480, 0, 1)]
POST_MODES = [helpers.REGION_REFERENCE_RASTER, helpers.REGION_SPEC]
POST_HALF_AOV = [36.0, 25.0]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def case(iw, ih, seed, nframes):
    return "%dx%d_s%d_n%d" % (iw, ih, seed, nframes)


def main():
    if not helpers.have_ref():
        raise SystemExit("make_golden_refchecks: oracle/_ref/librdref.so not built")
    out = {}
    # (1) a seed that has no other golden file, plane by plane
    iw, ih = 320, 240
    N = iw * ih
    img = synth.frame(synth.SEED0 + 11, iw, ih, 3)
    r = helpers.RefRect(iw, ih)
    rects, snaps = r.execute_once(img, 0.7, snapshots=NEW_SEED_PLANES)
    r.close()
    sizes = {"vxy": 2 * N, "table": (N * 4 // 5) * 5}
    out["new_seed_input_crc"] = np.uint32(crc(img))
    out["new_seed_planes"] = np.array(NEW_SEED_PLANES)
    out["new_seed_plane_crc"] = np.array([crc(snaps[p][: sizes.get(p, N)]) for p in NEW_SEED_PLANES], np.uint32)
    out["new_seed_rects"] = rects
    # (2) the reference's merge kernel with concurrent work-items
    R = helpers.ref()
    R.rdcl_set_order.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 4
    tan = float(np.tan(36.0 / 180.0 * np.pi))
    for iw, ih, seed, nframes in MERGE_CASES:
        c = case(iw, ih, seed, nframes)
        r = helpers.RefRect(iw, ih)
        try:
            R.rdcl_set_order(b"rect:labelMergeMain", 0, 0, 5, 0)
            for t in range(nframes):
                img = synth.frame(synth.SEED0 + seed, iw, ih, t)
                rects, snaps = r.execute_once(img, tan, snapshots=["region", "rsize", "boundary", "table"])
                out[f"merge_{c}_f{t}_input_crc"] = np.uint32(crc(img))
                for k in ("region", "rsize", "boundary"):
                    out[f"merge_{c}_f{t}_{k}_crc"] = np.uint32(crc(snaps[k].view(np.int32)))
                out[f"merge_{c}_f{t}_rects"] = rects
        finally:
            R.rdcl_set_order(b"", 0, 0, 0, 0)
            r.close()
    # (3) the reference's own host code on the oracle's planes
    for iw, ih, seed, nframes in POST_CASES:
        c = case(iw, ih, seed, nframes)
        r = helpers.RefRect(iw, ih)
        for mode in POST_MODES:
            orc = helpers.OracleRect(iw, ih, mode)
            for t in range(nframes):
                orc.frame(synth.frame(synth.SEED0 + seed, iw, ih, t))
                segs, boundary, table = orc.segments(), orc.plane("boundary"), orc.plane("table")
                key = f"post_{c}_m{mode}_f{t}"
                out[key + "_planes_crc"] = np.array([crc(segs), crc(boundary), crc(table)], np.uint32)
                for half_aov in POST_HALF_AOV:
                    out[key + "_a%d_rects" % int(half_aov)] = r.host_postprocess(segs, boundary, table, float(np.tan(half_aov / 180.0 * np.pi)))
            orc.close()
        r.close()
    path = os.path.join(helpers.GOLDEN, "ref_checks.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
