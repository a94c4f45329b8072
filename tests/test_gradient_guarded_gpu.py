"""mm_gll_gradient under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/gradient_cases.py bit for
bit (NaN positions compared, payloads not), counts exactly.

At the end of a mapping: the coordinates f64[E, P, dim], u f64[C, E, P], the derivative table f64[m][m] and the four
outputs, at element counts of one tile minus one, one tile and one tile plus one, orders 1, 2, 4, in 2-D and 3-D.
A net under: the shared tile core (mm_gll_tile.h) on a partial last tile -- fetch_x and fetch_u load idx < tile_nodes
only, 0.0 elsewhere --; the prefetch of a tile past the last; lanes that hold no node (256 / P leaves some over), which
neither load nor store; the table's last row.

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
import gradient_cases as GC
import mass_cases as M
from multimesh_amd import api
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.gradient_cases():
    print(case["name"], flush=True)
    order, dim, gp, u = case["order"], case["dim"], case["points"], case["u"]
    ref = GC.gradient(gp, order, api.gll_quadrature(order)[2], u)
    if dim == 3:
        got = ctx.gll_gradient(order, gp, u, grad=True, radial=True, lateral=True, norm=True)
        want = ref
    else:
        got = ctx.gll_gradient(order, gp, u, grad=True, norm=True)
        want = (ref[0], ref[3])
    for g, w in zip(got, want):
        assert M.same_bits(g.numpy(), w), case["name"]
    assert M.same_bits(ctx.gll_gradient(order, gp, u[0], grad=False, norm=True).numpy(), ref[3][:1]), case["name"]
print("ok")
"""


def test_gradient_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
