"""mm_gll_mass, mm_weighted_sum and the assembly under GUARDED allocations (MM_GUARD_ALLOC=1,
multimesh_amd/csrc/mm_context.hip): the coordinates, the tables, the mass and the determinant end at the end of their
mapping with unmapped addresses behind them, so a read or write past an array would fault at once.  A net, not a
provocation: the inputs are ordinary meshes -- element counts whose mass array fills its last 16-byte granule exactly
(an even number of values), a whole number of pages, or neither, with a broken last tile -- and the results are compared
with NumPy bit for bit.

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
import mass_cases as M
from multimesh_amd import api, synth
from multimesh_amd.device import Context

ctx = Context(0)
rng = np.random.default_rng(99)
for order in (1, 2, 4):
    _, w, D = api.gll_quadrature(order)
    P = (order + 1) ** 3
    full = synth.gll_mesh(17, order, seed=3)                       # 4096 elements: nelem * P * 8 bytes is whole pages
    tile = M.tile_elems(order, 3)
    for nelem in (4096, 512, 2, 1, tile + 1, 3 * tile - 1, 1001):
        gp = np.ascontiguousarray(full[:nelem])
        ref_mass, ref_det = M.mass(gp, order, w, D)
        mass, n_bad, det = ctx.gll_mass(order, gp, want_det=True)
        assert M.same_bits(mass.numpy(), ref_mass) and M.same_bits(det.numpy(), ref_det) and n_bad == 0, (order, nelem)
        f = rng.normal(size=(2,) + gp.shape[:2])
        assert M.same_bits(ctx.weighted_sum(mass, f), M.weighted_sum(ref_mass, f.reshape(2, -1))), (order, nelem)
        assert M.same_bits(ctx.weighted_sum(mass), M.weighted_sum(ref_mass)), (order, nelem)
for order, dim, n in ((1, 2, 33), (2, 2, 20), (4, 2, 12)):
    _, w, D = api.gll_quadrature(order)
    gp = synth.gll_mesh(n, order, seed=3, dim=dim)
    ref_mass, _ = M.mass(gp, order, w, D)
    assert M.same_bits(ctx.gll_mass(order, gp)[0].numpy(), ref_mass), (order, dim)
gp = synth.gll_mesh(5, 2, seed=3)
vals = rng.uniform(0.5, 1.5, size=gp.shape[:2])
out = api.assemble_gll(vals, gp, context=ctx)[0].reshape(-1)
uniq, inv = np.unique(gp.reshape(-1, 3), axis=0, return_inverse=True)
ref = np.zeros(len(uniq))
np.add.at(ref, inv.reshape(-1), vals.reshape(-1))
assert M.same_bits(out, ref[inv.reshape(-1)])
print("ok")
"""


def test_mass_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
