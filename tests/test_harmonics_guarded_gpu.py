"""mm_harmonic_model_apply under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/harmonic_cases.py bit for
bit (NaN positions compared, payloads not), counts exactly.

At the end of a mapping: the points, the radii (4 or 5 knots), the coefficients f64[NC, m, 2, NLM] (a multiple of 16
bytes whatever the shape: the last value read is the last of the array), values_in, and in the scratch the recurrence
tables d, a, b and the layer starts.
A net under: the coefficient row of knot i + 1 at the top knot (i <= m - 2, so the sine plane of row m - 1 at idx(lmax, lmax)
is the last double of a component); the packed (l, k) tables at l = lmax (q <= NLM - 1); d[lmax]; lstart[nlayers]; lanes
without work, which adopt the interval of the wave's first live lane and never one of their own; degrees 0, 1, 8 and 40.

The inputs are those of tests/guarded_cases.py, whose edges tests/test_guarded_cases.py counts without a GPU.  The switch is
read once per process, so the checks run in a child process, as in tests/test_resolution_guarded_gpu.py; the child prints
the name of every case before it runs it."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_CHECKS = r"""
import sys
import numpy as np
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import guarded_cases as G
import harmonic_cases as HC
from multimesh_amd import harmonics as H
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.harmonic_cases():
    print(case["name"], flush=True)
    pts, R, coef, L = case["points"], case["radius"], case["coef"], case["lmax"]
    for extend in (False, True):
        for mode in (0, 1, 2):
            vin = case["values_in"] if mode else None
            want, nout = HC.model_apply(pts, R, coef, L, mode=mode, extend=extend, values_in=vin)
            count = ctx.to_device(np.array([3], dtype=np.int64))
            got = H.harmonic_model_apply(ctx, pts, R, coef, L, mode=mode, extend=extend,
                                         values_in=None if vin is None else ctx.to_device(vin), noutside=count)
            assert HC.same_bits_nan(got.numpy().reshape(want.shape), want), (case["name"], extend, mode)
            assert int(count.numpy()[0]) == 3 + nout, (case["name"], extend, mode)
print("ok")
"""


def test_harmonics_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
