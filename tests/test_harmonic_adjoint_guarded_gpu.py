"""mm_harmonic_model_transpose under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/harmonic_adjoint_cases.py bit for
bit (NaN positions compared, payloads not), counts exactly.

At the end of a mapping: the points, the radii, the values and the weight, the output f64[NC, m, 2, NLM], and in the
scratch the recurrence tables, the layer starts and the slabs f64[nseg][nc][m - 1][4][nq] of a pass.
A net under: the same table reads as the forward call; the slab row of interval m - 2, factor 3, at the pass's last (l, k)
(the slab's last double) -- also with the slabs cut to one order per pass by a scratch limit of one order-0 slab, where the
smallest case must give the same bits as at the library's own limit; the gather's rows j = 0 (no Hi) and j = m - 1 (no Lo).

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
import harmonic_adjoint_cases as AC
import harmonic_cases as HC
from multimesh_amd import harmonic_adjoint as A
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.harmonic_adjoint_cases():
    print(case["name"], flush=True)
    pts, R, L, values = case["points"], case["radius"], case["lmax"], case["values"]
    for weight in (None, case["weight"]):
        for extend in (False, True):
            want, nout = AC.model_transpose(pts, R, L, values, weight=weight, extend=extend)
            first = None
            for limit in case["limits"]:                  # (the argument of tests/test_harmonic_adjoint_gpu.py)
                count = ctx.to_device(np.array([3], dtype=np.int64))
                out = ctx.to_device(np.full(want.shape, -7.0))
                got = A.harmonic_model_transpose(ctx, pts, R, L, values, weight=weight, extend=extend, out=out, noutside=count,
                                                 scratch_limit=limit).numpy().reshape(want.shape)
                assert HC.same_bits_nan(got, want), (case["name"], extend, limit)
                assert int(count.numpy()[0]) == 3 + nout
                assert first is None or got.tobytes() == first, (case["name"], limit)
                first = got.tobytes()
print("ok")
"""


def test_harmonic_adjoint_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
