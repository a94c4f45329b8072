"""Randomised end-to-end check of mm_interpolate_hex8 against the oracle (cKDTree + C restatement +
NumPy-order gather): random mesh sizes, shears, anisotropy, k, component counts, target clouds that
lie inside, on and outside the hull, lazy and eager candidate lists.  The long run of tests/fuzz_cases.py
(draw_pipeline / check_pipeline at the "tool" sizes; tests/test_fuzz_gpu.py runs a seeded slice at the suite's sizes);
prints one line per case and exits non-zero on the first mismatch.
    python tools/fuzz_pipeline.py [ncases [seed [only [big]]]]
FP_MODE=tol in the environment runs the context in MM_FP_TOL: node ids, failed counts and zero rows are still compared
exactly, weights and values to max(1e-12, 64 eps max|x| / shortest element edge) (the mode's stated tolerance)."""
import os, sys, time
import numpy as np
sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import fuzz_cases as F
from multimesh_amd.device import Context

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
only = int(sys.argv[3]) if len(sys.argv) > 3 else -1      # replay one case of a seed's sequence
big = len(sys.argv) > 4 and sys.argv[4] == "big"         # meshes up to 120^3 nodes, up to 2 M targets
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 12345
ctx = Context(0)
TOL = os.environ.get("FP_MODE", "exact") == "tol"
ctx.set_fp_mode("tol" if TOL else "exact")
redone = solves_guess = 0
t_start = time.time()
for c in F.cases("pipeline", seed, ncases, "big" if big else "tool"):
    if only >= 0 and c["case"] != only:
        continue
    try:
        info = F.check_pipeline(ctx, c)
    except AssertionError as e:
        print(e, flush=True)
        sys.exit(1)
    print(info["line"], flush=True)
    redone += info["redone"]
    solves_guess += c["npts"] if TOL else 0
print(f"{ncases} cases ok in {time.time() - t_start:.0f} s" + (f" (MM_FP_TOL: {redone} solves repeated exactly for {solves_guess} targets)" if TOL else ""))
