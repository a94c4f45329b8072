"""mm_geographic_points under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array ends at the
end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A net, not a
provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/geodesy_cases.py bit for
bit (NaN positions compared, payloads not).

At the end of a mapping: f64[n, 3] points with n = 1 and 101 (3 n doubles end on no granule), 2 and 512; the radius and the
height arrays f64[n], which end at their own mappings.  A net under: the three 8-byte loads of the last point, which the
compiler may merge into wider ones (24 bytes, never 32), and the 8-byte load and store of the last radius and height; both
directions, in place and out of place.

The inputs are geodesy_cases.guarded_cases().  The switch is read once per process, so the checks run in a child process, as
in tests/test_frames_guarded_gpu.py; the child prints the name of every case before it runs it."""
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
import geodesy_cases as GC
from multimesh_amd import geodesy as G
from multimesh_amd.device import Context

ctx = Context(0)
ell = GC.constants()
for case in GC.guarded_cases():
    print(case["name"], flush=True)
    pts, rho = case["points"], case["radius"]
    n = len(pts)
    want, want_h = GC.to_geographic(ell, pts)
    want_r, _ = GC.to_geographic(ell, pts, radius=rho)
    want_back = GC.from_geographic(ell, pts)
    src = ctx.to_device(pts)
    assert GC.same_bits_nan(G.geographic_points_on_device(ctx, src, ell).numpy(), want), case["name"]
    heights = ctx.to_device(np.full(n, -7.0))
    out = G.geographic_points_on_device(ctx, src, ell, radius=ctx.to_device(rho), height_out=heights)
    assert GC.same_bits_nan(out.numpy(), want_r) and GC.same_bits_nan(heights.numpy(), want_h), case["name"]
    assert GC.same_bits_nan(G.geographic_points_on_device(ctx, src, ell, G.TO_CARTESIAN).numpy(), want_back), case["name"]
    heights = ctx.to_device(np.full(n, -7.0))
    G.geographic_points_on_device(ctx, src, ell, out=src, radius=ctx.to_device(rho), height_out=heights)
    assert GC.same_bits_nan(src.numpy(), want_r) and GC.same_bits_nan(heights.numpy(), want_h), case["name"]
    src = ctx.to_device(pts)
    G.geographic_points_on_device(ctx, src, ell, G.TO_CARTESIAN, out=src)
    assert GC.same_bits_nan(src.numpy(), want_back), case["name"]
print("ok")
"""


def test_geographic_points_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
