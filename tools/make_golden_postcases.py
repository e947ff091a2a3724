#!/usr/bin/env python3
"""tests/golden/postcases_ref.npz: the rectangle lists THE REFERENCE'S OWN compiled executeCPUTask (oracle/_ref, helpers.RefRect.host_postprocess) returns for
the crafted inputs of tests/postcases.py, for two apertures, with the CRCs of the planes it was given.  tests/test_cpu_postcases.py compares rd_postprocess_planes
with them everywhere and, where oracle/_ref is built, the reference itself with them again.  Needs oracle/_ref (build() where the reference sources are present)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import helpers, postcases  # noqa: E402


def main():
    out, refs = {}, {}
    for fn, kw in postcases.ALL_CASES:
        c = postcases.get(fn, kw)
        key = postcases.case_id(fn, kw)
        r = refs.setdefault((c.iw, c.ih), helpers.RefRect(c.iw, c.ih))
        out[key + "_planes_crc"] = np.array(postcases.planes_crc(c), np.int64)
        for name, tan in (("a36", postcases.TAN36), ("a25", postcases.TAN25)):
            out[key + "_" + name + "_rects"] = r.host_postprocess(c.segs, c.boundary, c.table, tan)
        print(key, len(out[key + "_a36_rects"]), "rectangles")
    for r in refs.values():
        r.close()
    np.savez_compressed(os.path.join(helpers.GOLDEN, "postcases_ref.npz"), **out)


if __name__ == "__main__":
    main()
