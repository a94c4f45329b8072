"""Randomised check of mm_knn_build / mm_knn_query against scipy's cKDTree: 1-3 dimensions, uniform,
clustered, anisotropic and lattice-like clouds, targets inside and outside the sources' box, k from 1
to 64, more targets than sources and the reverse.  The long run of tests/fuzz_cases.py (draw_knn / check_knn at the
"tool" sizes; tests/test_fuzz_gpu.py runs a seeded slice of the same at the suite's sizes); exits non-zero on the
first mismatch.
    python tools/fuzz_knn.py [ncases [seed [only [start]]]]"""
import os, sys, time
import numpy as np
sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import fuzz_cases as F
from multimesh_amd.device import Context

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 2024
only = int(sys.argv[3]) if len(sys.argv) > 3 else -1
start = int(sys.argv[4]) if len(sys.argv) > 4 else 0     # skip the cases before this one (same random sequence)
ctx = Context(0)
t0 = time.time()
for c in F.cases("knn", seed, ncases, "tool"):
    if (only >= 0 and c["case"] != only) or c["case"] < start:
        continue
    try:
        print(F.check_knn(ctx, c)["line"], flush=True)
    except AssertionError as e:
        print(e, flush=True)
        sys.exit(1)
print(f"{ncases} cases ok in {time.time() - t0:.0f} s")
