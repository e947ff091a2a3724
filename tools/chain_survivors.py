#!/usr/bin/env python3
"""What the chain graph's prefilter leaves on the bench stream: per frame the chain pixels (polyctr[0]), those in 8-connected components of more than size_thre
pixels (polyctr[26], the survivor list the graph runs on) and the live pixels behind the exact filter (polyctr[24]).
usage: chain_survivors.py [frames [WxH [stream seed]]]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rectdetect_amd as ra
from rectdetect_amd import synth

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 32
iw, ih = (int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "1920x1080").split("x"))
seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
det = ra.Detector(iw, ih, nslots=1)
tot = np.zeros(3, np.int64)
for t in range(frames):
    det.enqueue(synth.frame(synth.SEED0 + seed, iw, ih, t))
    det.poll(np.tan(np.pi / 5))
    c = det.plane("polyctr", np.int32, 64)
    row = np.array([c[0], c[26], c[24]], np.int64)
    tot += row
    print("frame %3d: chain pixels %6d  survivors %6d (%.1f %%)  live %6d" % (t, row[0], row[1], 100.0 * row[1] / max(row[0], 1), row[2]))
det.close()
print("all %d frames: chain pixels %d  survivors %d (%.1f %%)  live %d (%.1f %%)" % (frames, tot[0], tot[1], 100.0 * tot[1] / max(tot[0], 1), tot[2], 100.0 * tot[2] / max(tot[0], 1)))
