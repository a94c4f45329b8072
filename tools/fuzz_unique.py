"""Randomised check of mm_unique_points against np.unique(axis=0, return_inverse=True), and of the order-free form
mm_unique_points_any_order: the same SET of unique rows, in the order of their first occurrence, and an inverse that
rebuilds the input.  The long run of tests/fuzz_cases.py (draw_unique / check_unique at the "tool" sizes;
tests/test_fuzz_gpu.py runs a seeded slice at the suite's sizes).
    python tools/fuzz_unique.py [ncases [seed]]"""
import os, sys, time
import numpy as np
sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import fuzz_cases as F
from multimesh_amd.device import Context

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ctx = Context(0)
t0 = time.time()
for c in F.cases("unique", seed, ncases, "tool"):
    try:
        print(F.check_unique(ctx, c)["line"], flush=True)
    except AssertionError as e:
        print(e, flush=True)
        sys.exit(1)
print(f"{ncases} cases ok in {time.time() - t0:.0f} s")
