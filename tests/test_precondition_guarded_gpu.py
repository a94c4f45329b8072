"""mm_point_taper, mm_order_statistics and mm_clamp under GUARDED allocations (MM_GUARD_ALLOC=1,
multimesh_amd/csrc/mm_context.hip): every array and every scratch carve ends at the end of its mapping with unmapped
addresses behind it, so a read or write past an array would fault at once.  A net, not a provocation: the inputs are
ordinary meshes and fields -- element counts whose arrays end on a 16-byte granule, on a whole page, or on neither, with a
broken last tile -- and the results are compared with the NumPy statements bit for bit.

The switch is read once per process, so the checks run in a child process, as in tests/test_mass_guarded_gpu.py."""
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
import precondition_cases as PC
from multimesh_amd import synth
from multimesh_amd.device import POINT_TAPER_BATCH, Context

ctx = Context(0)
rng = np.random.default_rng(99)
for order in (1, 2, 4):
    P = (order + 1) ** 3
    full = synth.gll_mesh(9, order, seed=3)                        # 512 elements: nelem * P * 8 bytes is whole pages
    tile = 256 // P
    for nelem in (512, 2, 1, tile + 1, 3 * tile - 1, 101):
        gp = np.ascontiguousarray(full[:nelem])
        flat = gp.reshape(-1, 3)
        for K in (0, 3, POINT_TAPER_BATCH + 1):
            c = flat[rng.integers(0, len(flat), K)] + rng.normal(size=(K, 3)) * 0.01
            ri = rng.uniform(0.0, 0.05, K)
            ro = ri + rng.uniform(0.0, 0.2, K)
            vals = rng.normal(size=(2, nelem * P))
            ref_out, ref_w, ref_count = PC.taper_apply(gp, c, ri, ro, vals)
            out, count, w = ctx.point_taper(gp, c, ri, ro, values_in=vals, want_weight=True)
            assert count == ref_count and PC.same_bits(w.numpy().reshape(-1), ref_w), (order, nelem, K)
            assert PC.same_bits(out.numpy().reshape(2, -1), ref_out), (order, nelem, K)
        vals = rng.normal(size=(3, nelem * P))
        vals[1, ::9] = np.nan
        d = ctx.to_device(vals)
        for m, method in ((1, "higher"), (16, "lower")):
            q = np.linspace(0.0, 1.0, m) if m > 1 else np.array([0.999])
            for absolute in (False, True):
                ref, ref_nv = PC.order_statistics(vals, q, absolute=absolute, method=method)
                out, nv = ctx.order_statistics(d, q, absolute=absolute, method=method)
                assert PC.same_bits_nan(out.numpy(), ref) and np.array_equal(nv.numpy(), ref_nv), (order, nelem, m)
        bound, _ = ctx.order_statistics(d, [0.9], absolute=True, method="higher")
        ref_bound = PC.order_statistics(vals, [0.9], absolute=True, method="higher")[0][:, 0]
        out, changed = ctx.clamp(d, upper=bound.reshape(3), symmetric=True, out=d)
        ref, ref_changed = PC.clamp(vals, upper=ref_bound, symmetric=True)
        assert PC.same_bits_nan(d.numpy(), ref) and np.array_equal(changed.numpy(), ref_changed), (order, nelem)
for n in (1, 2, 255, 511, 512, 4097):                              # clouds: 24 n bytes end on a granule for even n only
    pts = rng.uniform(0, 1, (n, 3))
    c = rng.uniform(0, 1, (5, 3))
    ref_w, ref_count = PC.taper_weight(pts, c, 0.05, 0.3)
    _, count, w = ctx.point_taper(pts, c, np.full(5, 0.05), np.full(5, 0.3), want_weight=True)
    assert count == ref_count and PC.same_bits(w.numpy(), ref_w), n
print("ok")
"""


def test_precondition_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
