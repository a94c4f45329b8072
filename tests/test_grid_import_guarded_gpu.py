"""mm_sample_grid under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): the points, the axes, the
cube and the outputs end at the end of their mapping with unmapped addresses behind them, so a corner index i1 / j1 / k1
one too far, or a bisection that reads a[n], would fault at once.  A net, not a provocation: the inputs are ordinary --
cubes and axes with an even number of values, so that the last corner is the last value of its 16-byte granule -- and the
results are compared with the NumPy statement bit for bit.

The switch is read once per process, so the checks run in a child process, as in tests/test_guarded_gpu.py."""
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
import grid_import_cases as G
from multimesh_amd.device import Context

ctx = Context(0)
all_pts = G.chunk_points(4098)


def check(pts, grid, depth, lat, lon, mode, fill):
    C, N = grid.shape[0], len(pts)
    pre = np.random.default_rng(C + N).normal(size=(C, N))
    out, nmissing, lld = ctx.sample_grid(pts, grid, depth, lat, lon, outside=mode, fill_value=fill,
                                         out=pre if mode == "keep" else None, want_latlondepth=True)
    lld = lld.numpy()
    want, miss, inside = G.sample(grid, depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1], mode, fill, False, pre)
    assert nmissing == miss and G.same_bits(out.numpy(), want), (mode, C, N, grid.shape)
    return inside


# even axis lengths and an even number of cube values: nothing behind the last node, nothing behind the last corner
depth = np.concatenate([G.DEPTH, [400_000.0]])                                     # 8
lat, lon = np.linspace(-6.0, 6.0, 10), np.linspace(-5.5, 6.5, 12)
for mode in G.MODES:
    for fill in (np.nan, -12345.5):
        for C in (1, 3, 4, 5):
            grid = G.grid_values(C, (8, 10, 12))
            for N in (0, 1, 255, 256, 257, 4098):
                check(all_pts[:N].reshape(N, 3), grid, depth, lat, lon, mode, fill)
    # points that clamp onto the last node of every axis, and the axes bisected in global memory
    inside = check(all_pts, G.grid_values(2, (2, 2, 2)), depth[[1, 2]], lat[[4, 5]], lon[[5, 6]], mode, np.nan)
    assert mode == "clamp" or 0 < inside.sum() < len(inside)
    check(all_pts, G.grid_values(2, (2, 4, 9000)), depth[[0, 7]], lat[[0, 3, 6, 9]], np.linspace(-5.5, 6.5, 9000), mode, np.nan)

# points exactly on the last node of all three axes read the last value of the cube
r0 = 6_000_000.0
edge_depth = np.array([100_000.0, G.R_EARTH - r0])
for p, la, lo in (([0.0, 0.0, r0], [60.0, 90.0], [-5.0, 0.0]), ([-r0, 0.0, 0.0], [-10.0, 0.0], [135.0, 180.0]),
                  ([0.0, r0, 0.0], [-10.0, 0.0], [45.0, 90.0])):
    grid = G.grid_values(2, (2, 2, 2), seed=9)
    out, nmissing = ctx.sample_grid(np.array([p]), grid, edge_depth, np.array(la), np.array(lo))
    assert nmissing == 0 and G.same_bits(out.numpy()[:, 0], grid[:, -1, -1, -1]), p
print("ok")
"""


def test_grid_import_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
