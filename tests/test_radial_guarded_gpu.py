"""mm_radial_bins, mm_binned_weighted_sum and mm_radial_model_apply under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statements of tests/radial_cases.py bit for
bit (NaN positions compared, payloads not), counts exactly.

At the end of a mapping: the points (24 n bytes: a granule, six pages, neither), the edges (4 values: 32 bytes; 5: 40), the
table's radii and values (4 or 5 rows), mass, fields and the int32 bins (4 n bytes), the layer starts in the scratch.
A net under: edges[nbins] and the bisection's a[n] (the largest index read is nbins, with a radius equal to the last edge
clipped to bin nbins - 1); R[i + 1] and V[i + 1] of the lerp at the top knot (i is clipped to b - 1 <= m - 2 before the
read); lstart[k + 1] of the last layer (k <= nlayers - 1, the array holds nlayers + 1); the tile's coordinate load on a
partial last tile (3 * nnodes doubles, not 768).

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
import radial_cases as RC
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.radial_cases():
    print(case["name"], flush=True)
    pts, R, V = case["points"], case["radius"], case["values"]
    for mode in (0, 1, 2, 3, 4):
        vin = case["values_in"] if mode else None
        got = ctx.radial_model_apply(pts, R, V, mode=mode, values_in=vin).numpy().reshape(len(V), -1)
        assert RC.same_bits_nan(got, RC.model_apply(pts, R, V, mode, vin)), (case["name"], mode)
    if "edges" in case:
        b, nout, r = RC.bins(pts, case["edges"])
        gb, gout, gr = ctx.radial_bins(pts, case["edges"], want_radius=True)
        assert np.array_equal(gb.numpy(), b) and gb.numpy().dtype == np.int32 and gout == nout and RC.same_bits(gr.numpy(), r)
        for square in (False, True):
            sums, count = ctx.binned_weighted_sum(case["mass"], b, case["nbins"], fields=case["fields"], square=square,
                                                  want_count=True)
            assert RC.same_bits(sums, RC.binned_weighted_sum(case["mass"], case["fields"], b, case["nbins"], square))
            assert np.array_equal(count, RC.bin_counts(b, case["nbins"]))
        assert RC.same_bits(ctx.binned_weighted_sum(case["mass"], b, case["nbins"]),
                            RC.binned_weighted_sum(case["mass"], None, b, case["nbins"]))
print("ok")
"""


def test_radial_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
