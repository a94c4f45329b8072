"""mm_rotate_points, mm_rotate_vectors and mm_local_components under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/frames_cases.py bit for
bit (NaN positions compared, payloads not), counts exactly.

At the end of a mapping: f64[n, 3] points with n = 1 and 101 (3 n doubles end on no granule), 2 and 512; planes
f64[3, E, P], MODEL/data rows f64[E, 5, P] whose last addressed column is the last of the array, and the positions.
A net under: the three 8-byte loads of the last point, which the compiler may merge into wider ones (24 bytes, never 32);
the last row [E - 1][cols[c]][P - 1] of rows addressed by group and component strides; in place and out of place.

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
import frames_cases as FC
from multimesh_amd import frames as F
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.frames_cases():
    print(case["name"], flush=True)
    R = case["matrix"]
    if "points" in case:
        pts = case["points"]
        for transpose in (False, True):
            want = FC.rotate_points(R, pts, transpose)
            src = ctx.to_device(pts)
            assert FC.same_bits_nan(F.rotate_points(ctx, src, R, transpose=transpose).numpy(), want), case["name"]
            F.rotate_points(ctx, src, R, transpose=transpose, out=src)
            assert FC.same_bits_nan(src.numpy(), want), case["name"]
        continue
    v, rows, cols, pos = case["planes"], case["rows"], case["cols"], case["positions"]
    _, E, P = v.shape
    plane = lambda a: (a, P, E * P, (0, 1, 2))
    for transpose in (False, True):
        want = FC.rotate_vectors(R, v, transpose)
        src, dst = ctx.to_device(v), ctx.to_device(np.full(v.shape, -7.0))
        F.rotate_vectors_on_device(ctx, R, E, P, plane(src), plane(dst), transpose=transpose)
        assert FC.same_bits_nan(dst.numpy(), want), case["name"]
        src = ctx.to_device(rows)
        F.rotate_vectors_on_device(ctx, R, E, P, (src, 5 * P, P, cols), (src, 5 * P, P, cols), transpose=transpose)
        assert FC.same_bits_nan(src.numpy()[:, cols, :].transpose(1, 0, 2), want), case["name"]
    for inverse in (False, True):
        for basis in ("rtp", "zne"):
            want = FC.local_components(pos, v, FC.TO_CARTESIAN if inverse else FC.TO_LOCAL, F.BASIS[basis])
            src, dst, p = ctx.to_device(v), ctx.to_device(np.full(v.shape, -7.0)), ctx.to_device(pos)
            F.local_components_on_device(ctx, p, E, P, plane(src), plane(dst), inverse=inverse, basis=basis)
            assert FC.same_bits_nan(dst.numpy(), want), (case["name"], inverse, basis)
            src = ctx.to_device(rows)
            F.local_components_on_device(ctx, p, E, P, (src, 5 * P, P, cols), (src, 5 * P, P, cols), inverse=inverse, basis=basis)
            assert FC.same_bits_nan(src.numpy()[:, cols, :].transpose(1, 0, 2), want), (case["name"], inverse, basis)
print("ok")
"""


def test_frames_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
