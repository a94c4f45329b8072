"""mm_grid_operator, the operator built on it and its transpose under GUARDED allocations
(MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statement of
tests/grid_adjoint_cases.py: ids, weights and counts exactly, on the coordinates the device returned (its acos and
atan2 are compared with NumPy's within 1e-11 degrees, the bound of tests/test_grid_adjoint_gpu.py), the transpose and its
fold bit for bit with np.add.at; GridOperator.apply within 32 eps max|corner| of mm_sample_grid, the bound derived in
tests/test_grid_adjoint_gpu.py (test_gather_through_the_operator_agrees_with_sample_grid).

At the end of a mapping: the points, the three axes (6, 10 and 12 nodes: granules; 4, 7 and 13: not), ids int64[N, 8] and
w f64[N, 8] (64 bytes a row, written as four 16-byte stores), the values, the cube and the transposed result.
A net under: a[i + 1] of the last cell of every axis (i is clipped to n - 2 before the read), also clamped onto it; the
corner ids k1 / j1 / i1 of a point in the last cell of all three axes, whose id is the cube's last value, read by the
gather and written by the transpose; the cell that closes a periodic axis and the fold of its column onto column 0; axes
the caller gave descending.

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
import grid_adjoint_cases as GA
import grid_import_cases as GI
from multimesh_amd import api
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.grid_operator_cases():
    print(case["name"], flush=True)
    (depth, lat, lon), pts, periodic, v = case["axes"], case["points"], case["periodic"], case["values"]
    ref = GI.latlondepth(pts)
    if periodic:
        ref[:, 1] = GI.wrap(ref[:, 1], lon[0])
    for clamp in (False, True):
        ids, w, nout, lld = ctx.grid_operator(pts, depth, lat, lon, clamp=clamp, lon_periodic=periodic, latlondepth=True)
        ids, w, lld = ids.numpy(), w.numpy(), lld.numpy()
        assert GA.angle_difference(lld[:, :2], ref[:, :2]).max() <= 1e-11 and GI.same_bits(lld[:, 2], ref[:, 2]), case["name"]
        want_ids, want_w, want_out, inside = GA.operator(depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1], clamp, periodic)
        assert nout == want_out and np.array_equal(ids, want_ids) and GI.same_bits(w, want_w), (case["name"], clamp)
    grid = api.RegularGrid(*case["caller"], {})
    op = api.grid_import_operator(grid, pts, context=ctx)
    assert op.flipped == case["flipped"] and op.appended == case["appended"] and op.periodic == periodic
    ids, w, nout, inside = GA.operator(depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1], False, periodic)
    assert ids.max() == op.nsrc - 1                                        # the cube's last value is a corner
    want = GA.transpose(ids, w, v, op.nsrc).reshape((len(v),) + op.prepared_shape)
    assert GI.same_bits(op.transpose(v, prepared=True), want), case["name"]
    assert op.noutside == nout and np.array_equal(op.ids.numpy(), ids) and GI.same_bits(op.w.numpy(), w), case["name"]
    assert GI.same_bits(op.transpose(v), GA.fold(want, case["flipped"], case["appended"])), case["name"]
    cube = GI.grid_values(3, op.grid_shape, seed=7)
    prepared = GA.to_prepared(cube, case["flipped"], case["appended"])
    applied = op.apply(cube, fill_value=0.0)
    sampled, miss = ctx.sample_grid(pts, prepared, depth, lat, lon, lon_periodic=periodic, outside="fill", fill_value=0.0)
    corner = np.abs(prepared.reshape(3, -1)[:, ids]).max(axis=2)
    assert miss == nout and (np.abs(applied - sampled.numpy()) <= 32 * GA.EPS * corner).all(), case["name"]
    assert GI.same_bits(applied[:, inside], GA.gather(prepared.reshape(3, -1), ids, w)[:, inside]), case["name"]
    op.free()
print("ok")
"""


def test_grid_operator_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
