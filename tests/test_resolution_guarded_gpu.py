"""mm_gll_resolution and mm_arg_extreme under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip):
every array ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault
at once.  A net, not a provocation: the inputs are ordinary meshes and rows -- element counts and lengths whose arrays end
on a 16-byte granule, on a whole page, or on neither -- and the results are compared with the NumPy statements of
tests/resolution_cases.py bit for bit.

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
import resolution_cases as RC
from multimesh_amd import synth
from multimesh_amd.device import Context

ctx = Context(0)
for order in (1, 2, 4):
    full = synth.gll_mesh(9, order, seed=3)                        # 512 elements: nelem * P * 24 bytes is whole pages
    fast, slow = RC.velocities(full, 2, 7), RC.velocities(full, 2, 8, lo=0.0, hi=4000.0)
    slow[:, ::5] = 0.0
    for nelem in RC.GUARDED_NELEM:                                 # 1 and 101: 8 * nelem bytes end on no granule
        gp = np.ascontiguousarray(full[:nelem])
        f, s = np.ascontiguousarray(fast[:, :nelem]), np.ascontiguousarray(slow[:, :nelem])
        for args in ((None, None), (f, None), (f, s)):
            ref, ref_info, ref_h = RC.resolution(gp, order, *args)
            out, info, h = ctx.gll_resolution(order, gp, fast=args[0], slow=args[1], want_node_spacing=True)
            assert RC.same_bits(out.numpy(), ref) and RC.same_bits(h.numpy(), ref_h), (order, nelem)
            assert info.numpy().tolist() == ref_info.tolist(), (order, nelem)
            out, info = ctx.gll_resolution(order, gp, fast=args[0], slow=args[1])
            assert RC.same_bits(out.numpy(), ref), (order, nelem)
rng = np.random.default_rng(99)
for n in RC.GUARDED_N:                                             # 8 n bytes end on a granule for even n only
    for nrows in (1, 3):
        v = rng.normal(size=(nrows, n))
        v[:, ::7] = np.nan
        for want_max in (False, True):
            ref = RC.arg_extreme(v, want_max)
            value, index, nvalid = (g.numpy() for g in ctx.arg_extreme(v, want_max=want_max))
            assert RC.same_bits(value, ref[0]) and np.array_equal(index, ref[1]) and np.array_equal(nvalid, ref[2]), (n, nrows)
print("ok")
"""


def test_resolution_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
