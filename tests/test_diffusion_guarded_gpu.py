"""mm_gll_diffusion_apply and the mm_pcg_* steps under GUARDED allocations
(MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/diffusion_cases.py and
the one-line statements of the vector updates (tests/test_diffusion_gpu.py) bit for bit, the active counts exactly.

At the end of a mapping: the coordinates, u f64[C, E, P] and y, the element-nodal diffusivities kappa_h and kappa_r
f64[E, P], the tables D f64[m][m] and w f64[m], at one tile minus one, one tile and one tile plus one element; the PCG
vectors f64[3, n] and the state block f64[3, 8].
A net under: the stiffness kernel's own copies of the tile's fetches on a partial last tile and its prefetch past the last
tile; kappa[node] of the last node of the last element (read by lanes with a node only); w[m - 1] behind D in the LDS
table; the state slots of the last system (slot index < 8: the block's last double is its slot 7) in the scalar kernel
and in the two vector kernels that read ACTIVE, ALPHA and BETA of system blockIdx.y.

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
import diffusion_cases as DC
import mass_cases as M
from multimesh_amd import api, helpers as S
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.diffusion_cases():
    print(case["name"], flush=True)
    order, dim, gp, u, kh, kr = (case[k] for k in ("order", "dim", "points", "u", "kappa_h", "kappa_r"))
    _, w, D = api.gll_quadrature(order)
    op = ctx.diffusion(order, gp, kappa_h=kh)
    assert M.same_bits(op.apply(u).numpy(), DC.apply(gp, order, w, D, u, kh=1.0, kh_array=kh)), case["name"]
    op.free()
    plain = ctx.diffusion(order, gp, kappa_h=0.7)
    assert M.same_bits(plain.apply(u[0]).numpy(), DC.apply(gp, order, w, D, u[:1], kh=0.7)), case["name"]
    plain.free()
    if dim == 3:
        op = ctx.diffusion(order, gp, kappa_h=kh, kappa_r=kr)
        assert M.same_bits(op.apply(u).numpy(), DC.apply(gp, order, w, D, u, kh=1.0, kh_array=kh, kr=1.0, kr_array=kr)), case["name"]
        op.free()
lib, h = S.load_lib(), ctx.handle
for case in G.pcg_cases():
    print("pcg", case["name"], flush=True)
    mass, p, kp, z, x, r = (case[k] for k in ("mass", "p", "kp", "z", "x", "r"))
    ncomp, n = p.shape
    dev = {k: ctx.to_device(case[k]) for k in ("mass", "p", "kp", "z", "x", "r")}
    out = ctx.empty((ncomp, n), np.float64)
    assert lib.mm_pcg_combine(h, dev["mass"].ptr, dev["p"].ptr, 0.125, dev["kp"].ptr, n, ncomp, out.ptr) == 0
    assert M.same_bits(out.numpy(), mass[None] * p + 0.125 * kp)
    assert lib.mm_pcg_combine(h, dev["mass"].ptr, dev["p"].ptr, 0.125, None, n, ncomp, out.ptr) == 0
    assert M.same_bits(out.numpy(), mass[None] * p)
    assert lib.mm_pcg_combine(h, None, None, -0.125, dev["kp"].ptr, n, ncomp, out.ptr) == 0
    assert M.same_bits(out.numpy(), -0.125 * kp)
    state_d = ctx.to_device(np.zeros((ncomp, S.MM_PCG_STATE)))
    nact = ctx.zeros((1,), np.int64)
    assert lib.mm_pcg_scalars(h, state_d.ptr, ncomp, S.MM_PCG_PHASE_START, 1e-3, nact.ptr) == 0 and nact.numpy()[0] == 3
    state = state_d.numpy()
    state[:, S.MM_PCG_BB] = [4.0, 4.0, 9.0]
    state[:, S.MM_PCG_RZ] = [1.0e-6, 4.1e-6, 2.0]              # system 0 converges at once, 1 and 2 go on
    state_d = ctx.to_device(state)
    assert lib.mm_pcg_scalars(h, state_d.ptr, ncomp, S.MM_PCG_PHASE_BETA, 1e-3, nact.ptr) == 0
    got = state_d.numpy()
    assert nact.numpy()[0] == 2 and list(got[:, S.MM_PCG_ACTIVE]) == [0.0, 1.0, 1.0] and list(got[1:, S.MM_PCG_RZ_OLD]) == [4.1e-6, 2.0]
    got[:, S.MM_PCG_PAP] = [1.0, 3.0, 7.0]
    got[:, S.MM_PCG_RZ] = [5.0, 1.0e-6, 0.5]
    state_d = ctx.to_device(got)
    assert lib.mm_pcg_scalars(h, state_d.ptr, ncomp, S.MM_PCG_PHASE_ALPHA, 1e-3, None) == 0
    alpha = state_d.numpy()[:, S.MM_PCG_ALPHA]
    assert list(alpha) == [0.0, 4.1e-6 / 3.0, 2.0 / 7.0]
    assert lib.mm_pcg_advance(h, state_d.ptr, dev["p"].ptr, dev["kp"].ptr, n, ncomp, dev["x"].ptr, dev["r"].ptr) == 0
    x_ref, r_ref = x + alpha[:, None] * p, r - alpha[:, None] * kp
    x_ref[0], r_ref[0] = x[0], r[0]                            # an inactive system is not touched
    assert M.same_bits(dev["x"].numpy(), x_ref) and M.same_bits(dev["r"].numpy(), r_ref)
    assert lib.mm_pcg_scalars(h, state_d.ptr, ncomp, S.MM_PCG_PHASE_BETA, 1e-3, nact.ptr) == 0
    beta = state_d.numpy()[:, S.MM_PCG_BETA]
    assert nact.numpy()[0] == 1 and list(beta) == [0.0, 0.0, 0.5 / 2.0]
    assert lib.mm_pcg_direction(h, state_d.ptr, dev["z"].ptr, n, ncomp, dev["p"].ptr) == 0
    p_ref = p.copy()
    p_ref[2] = z[2] + beta[2] * p[2]
    assert M.same_bits(dev["p"].numpy(), p_ref)
print("ok")
"""


def test_diffusion_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
