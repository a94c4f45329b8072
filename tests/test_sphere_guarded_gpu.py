"""mm_map_to_sphere, mm_sphere_ratio, mm_scale_points and mm_first_occurrence under GUARDED allocations
(MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the reference's own output
(tests/golden/sphere_map.npz) and its NumPy restatement (tests/test_sphere.py), bit for bit, as tests/test_sphere_gpu.py does;
the first occurrences with np.unique's.

At the end of a mapping: the points (n = 8, 101, 1024), one radius per point (element-nodal) or rad f64[E, 8] with the
connectivity int64[E, 8] and the first occurrences int64[n] (node layout), the ratio and the outputs.
A net under: rad[first[i]] of the node whose first occurrence is the connectivity's last entry -- rad[nrad - 1]; the index
is range-checked against nrad before the read, so rad[nrad] is never formed --; the connectivity's last entry in the
atomic-min pass; the last slot of first in its three passes; factor[n - 1] and the last point, in place and out of place.

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
from test_sphere import R_EARTH, map_to_sphere_numpy
from multimesh_amd.device import Context

ctx = Context(0)
print("golden", flush=True)
g = np.load("tests/golden/sphere_map.npz")
assert np.array_equal(ctx.map_to_sphere(g["en_points"], g["en_z_node_1D"]).numpy(), g["en_expected"])
got = ctx.map_to_sphere(g["node_points"], g["node_z_node_1D"], connectivity=g["node_connectivity"]).numpy()
assert np.array_equal(got, g["node_expected"])
for case in G.sphere_cases():
    print(case["name"], flush=True)
    pts, rad, conn, nodal = case["points"], case["rad"], case["connectivity"], case["rad_nodal"]
    n = len(pts)
    want = map_to_sphere_numpy(pts, rad)
    assert ctx.map_to_sphere(pts, rad).numpy().tobytes() == want.tobytes(), case["name"]
    d = ctx.to_device(pts)
    assert ctx.map_to_sphere(d, rad, out=d) is d and d.numpy().tobytes() == want.tobytes(), case["name"]
    first = ctx.first_occurrence(conn, n)
    assert np.array_equal(first.numpy(), np.unique(conn, return_index=True)[1]) and first.numpy()[-1] == conn.size - 1
    want = map_to_sphere_numpy(pts, nodal, conn)
    assert ctx.map_to_sphere(pts, nodal, connectivity=conn).numpy().tobytes() == want.tobytes(), case["name"]
    assert ctx.map_to_sphere(pts, nodal, first=first).numpy().tobytes() == want.tobytes(), case["name"]
    norm = np.sqrt((pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2])
    ratio = ctx.sphere_ratio(pts, rad).numpy()
    assert ratio.tobytes() == ((norm / R_EARTH) / rad).tobytes(), case["name"]
    nodal_first = nodal.reshape(-1)[np.unique(conn, return_index=True)[1]]
    assert ctx.sphere_ratio(pts, nodal, connectivity=conn).numpy().tobytes() == ((norm / R_EARTH) / nodal_first).tobytes()
    assert ctx.scale_points(pts, ratio).numpy().tobytes() == (ratio * pts.T).T.tobytes(), case["name"]
    d = ctx.to_device(pts)
    ctx.scale_points(d, ratio, out=d)
    assert d.numpy().tobytes() == (ratio * pts.T).T.tobytes(), case["name"]
print("ok")
"""


def test_sphere_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
