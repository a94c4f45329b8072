"""mm_sample_columns_gll through extract_regular_grid under GUARDED allocations
(MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the CPU oracle at the generated targets (centroid
kNN, acceptance loop, weighted sums), bit for bit, as tests/test_regular_grid_gpu.py does; the generated points with
latlondepth_to_xyz bit for bit; the missing count exactly.

At the end of a mapping: a small Earth chunk's coordinates and three fields, the trig tables f64[5, 2] and f64[6, 2], the
five radii (40 bytes), the chunk buffers (targets, lists, element ids, reference coordinates), sized for 64 targets,
and the output.  150 targets go in chunks of 64, 64 and 22.
A net under: the last generated column of a chunk and of the PARTIAL last chunk (n = 22 lanes of a 256-lane block write
points; the kNN, the locate and the value pass see n, not the chunk size); lat[2 a + 1] / lon[2 b + 1] of the last column and
radius[ndepth - 1]; out + t0 of the last chunk with the component stride of the whole grid.  One chunk of 150 gives the
same bits.

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
from multimesh_amd import api
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.regular_grid_cases():
    print(case["name"], flush=True)
    order, gp, f, lat, lon, depth = (case[k] for k in ("order", "points", "fields", "lat", "lon", "depth"))
    D, LA, LO = np.meshgrid(depth, lat, lon, indexing="ij")
    targets = api.latlondepth_to_xyz(np.stack([LA, LO, D], axis=-1).reshape(-1, 3))
    lat_t, lon_t, r = api.column_tables(lat, lon, depth)
    vals, miss, pts = ctx.sample_columns_gll(order, gp, f, lat_t, lon_t, r, nelem_to_search=G.SEARCH, want_points=True,
                                             chunk_points=G.REGULAR_CHUNK)
    assert pts.numpy().reshape(-1, 3).tobytes() == targets.tobytes(), case["name"]
    want, found, want_miss = G.regular_grid_oracle(case, targets)
    flat = vals.numpy().reshape(3, -1)
    assert miss == want_miss and flat[:, found].tobytes() == np.ascontiguousarray(want[:, found]).tobytes(), case["name"]
    assert np.isnan(flat[:, ~found]).all()
    mesh = api.GllMesh(gp.copy(), order, {"A": f[0], "B": f[1], "C": f[2]})
    for chunk in (G.REGULAR_CHUNK, len(targets)):
        grid = api.extract_regular_grid(mesh, ["A", "B", "C"], **G.REGULAR_GRID, nelem_to_search=G.SEARCH, chunk_points=chunk,
                                        context=ctx)
        got = np.stack([grid[k] for k in "ABC"]).reshape(3, -1)
        assert grid.nmissing == want_miss and got.tobytes() == flat.tobytes(), (case["name"], chunk)
print("ok")
"""


def test_regular_grid_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
