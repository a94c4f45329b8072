"""Randomised check of mm_locate_gll (tolerance / snap loop) and mm_locate_gll_bbox (bounding-box loop)
plus mm_gather_elem and the fused mm_interpolate_gll against the oracle's restatement: orders 1, 2, 4 in 2-D and 3-D, distorted meshes,
targets inside, on and outside the hull, random k / tolerance / snapping.  Bit-equal element ids,
coefficients and gathered values are required.  The long run of tests/fuzz_cases.py (draw_gll / check_gll at the "tool"
sizes; tests/test_fuzz_gpu.py runs a seeded slice at the suite's sizes).
    python tools/fuzz_gll.py [ncases [seed]]"""
import os, sys, time
import numpy as np
sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import fuzz_cases as F
from multimesh_amd.device import Context

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
ctx = Context(0)
t0 = time.time()
for c in F.cases("gll", seed, ncases, "tool"):
    try:
        print(F.check_gll(ctx, c)["line"], flush=True)
    except AssertionError as e:
        print(e, flush=True)
        sys.exit(1)
print(f"{ncases} cases ok in {time.time() - t0:.0f} s")
