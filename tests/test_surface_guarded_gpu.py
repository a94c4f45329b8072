"""The surface entry points under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array and
every scratch carve ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array
would fault at once.  A net, not a provocation: the inputs are ordinary meshes and clouds -- element, triangle and point
counts whose arrays end on a 16-byte granule, on a whole page, or on neither -- and the results are compared with the NumPy
statements of tests/surface_cases.py bit for bit.

The switch is read once per process, so the checks run in a child process, as in tests/test_boundary_guarded_gpu.py."""
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
import boundary_cases as BC
import surface_cases as SC
from multimesh_amd import device, surface, synth
from multimesh_amd.device import Context

ctx = Context(0)
lib = surface.bind(ctx.lib)
rng = np.random.default_rng(99)

def triangles(gp, order, faces, side, mask):
    out = ctx.empty((len(faces) * 2 * order * order, 3, 3), np.float64)
    T = device._call(lib, "mm_boundary_triangles", ctx.handle, ctx.to_device(gp), len(gp), order, ctx.to_device(faces),
                     ctx.to_device(side), len(faces), mask, out, arg_error=True)
    return out.rows(0, T)

for order in (1, 2, 4):
    full = synth.gll_mesh(9, order, seed=3)                        # 512 elements: nelem * P * 24 bytes is whole pages
    for nelem in (512, 64, 1, 2, 101):                             # 64: whole pages again; 1, 2: a granule; 101: neither
        gp = np.ascontiguousarray(full[:nelem])
        corners = np.ascontiguousarray(gp[:, BC.corner_nodes(order)])
        faces, _ = BC.boundary_faces(BC.corner_ids(corners)[0])
        side = BC.classify(corners, faces, up=(0.0, 0.0, 1.0))
        for mask in (0, 0b010, 0b101, 0b111):                        # (the last one's triangles are searched below)
            ref_tri = SC.boundary_triangles(gp, order, faces, side, mask)
            tri = triangles(gp, order, faces, side, mask)
            assert SC.same_bits(tri.numpy(), ref_tri), (order, nelem, mask)
        if nelem in (64, 101) and order == 2 or nelem <= 2:
            targets = gp.reshape(-1, 3)[::3] if nelem > 2 else gp
            least, _ = SC.surface_distance(targets, ref_tri, np.inf)
            for cutoff in (0.04, 0.3, np.inf):
                ref, ref_count = SC.with_cutoff(least, cutoff)
                d, count = surface.distance_to_triangles(targets, tri, cutoff, context=ctx)
                assert count == ref_count and SC.same_bits(d.numpy().reshape(-1), ref), (order, nelem, cutoff)
for n, T in ((1, 1), (2, 3), (255, 17), (512, 512), (4097, 129), (1024, 0)):   # 24 n bytes end on a granule for even n only
    pts = rng.uniform(-0.2, 1.2, (n, 3))
    a = rng.uniform(0, 1, (T, 1, 3))
    tri = a + np.concatenate([np.zeros((T, 1, 3)), rng.uniform(-0.1, 0.1, (T, 2, 3))], axis=1)
    least, _ = SC.surface_distance(pts, tri, np.inf)
    for cutoff in (0.05, 0.4, np.inf):
        ref, ref_count = SC.with_cutoff(least, cutoff)
        d, count = surface.distance_to_triangles(pts, tri, cutoff, context=ctx)
        assert count == ref_count and SC.same_bits(d.numpy(), ref), (n, T, cutoff)
print("ok")
"""


def test_surface_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
