"""The boundary entry points under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
and every scratch carve ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array
would fault at once.  A net, not a provocation: the inputs are ordinary meshes and clouds -- element and point counts whose
arrays end on a 16-byte granule, on a whole page, or on neither -- and the results are compared with the NumPy statements
of tests/boundary_cases.py bit for bit.

The switch is read once per process, so the checks run in a child process, as in tests/test_precondition_guarded_gpu.py."""
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
from multimesh_amd import synth
from multimesh_amd.device import Context

ctx = Context(0)
rng = np.random.default_rng(99)
for order in (1, 2, 4):
    full = synth.gll_mesh(9, order, seed=3)                        # 512 elements: nelem * P * 24 bytes is whole pages
    for nelem in (512, 64, 1, 2, 101):                             # 64 * 8 ids: a page of corner ids; 101: neither
        gp = np.ascontiguousarray(full[:nelem])
        corners = np.ascontiguousarray(gp[:, BC.corner_nodes(order)])
        ids, nnodes = BC.corner_ids(corners)
        ref_faces, ref_many = BC.boundary_faces(ids)
        faces, many = ctx.boundary_faces(ids, nnodes)
        assert many == ref_many and np.array_equal(faces.numpy(), ref_faces), (order, nelem)
        ref_side = BC.classify(corners, ref_faces, up=(0.0, 0.0, 1.0))
        side = ctx.boundary_classify(corners, faces, up=(0.0, 0.0, 1.0))
        assert np.array_equal(side.numpy(), ref_side), (order, nelem)
        for mask in (0, 0b010, 0b101, 0b111):                        # (the last one's nodes are the sources below)
            ref_nodes = BC.boundary_nodes(gp, order, ref_faces, ref_side, mask)
            nodes = ctx.boundary_nodes(gp, order, faces, side, mask)
            assert BC.same_bits(nodes.numpy(), ref_nodes), (order, nelem, mask)
        if nelem in (512, 101) and order == 4 or nelem <= 2:
            targets = gp if nelem <= 101 else gp[::13]
            for cutoff in (0.04, 0.3):
                ref, ref_count = BC.cutoff_distance(targets, ref_nodes, cutoff)
                d, count = ctx.cutoff_distance(targets, nodes, cutoff)
                assert count == ref_count and BC.same_bits(d.numpy().reshape(-1), ref), (order, nelem, cutoff)
for n, K in ((1, 1), (2, 3), (255, 17), (512, 512), (4097, 1001), (1024, 0)):   # 24 n bytes end on a granule for even n only
    pts = rng.uniform(-0.2, 1.2, (n, 3))
    src = rng.uniform(0, 1, (K, 3))
    for cutoff in (0.05, 0.4):
        ref, ref_count = BC.cutoff_distance(pts, src, cutoff)
        d, count = ctx.cutoff_distance(pts, src, cutoff)
        assert count == ref_count and BC.same_bits(d.numpy(), ref), (n, K, cutoff)
    a, b = rng.normal(size=(2, n)), rng.normal(size=(2, n))
    elem = rng.integers(-1, 3, n)
    ref_out, ref_w, ref_count = BC.distance_taper(ref, 0.1, 0.3, a, b=b, elem=elem)
    out, count, w = ctx.distance_taper(d, 0.1, 0.3, a, b=b, elem=elem, want_weight=True)
    assert count == ref_count and BC.same_bits(w.numpy(), ref_w) and BC.same_bits(out.numpy(), ref_out), n
    ref_out, _, ref_count = BC.distance_taper(ref, 0.1, 0.3, a)
    a_d = ctx.to_device(a)
    _, count = ctx.distance_taper(d, 0.1, 0.3, a_d, out=a_d)
    assert count == ref_count and BC.same_bits(a_d.numpy(), ref_out), n
print("ok")
"""


def test_boundary_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
