"""CPU side of the GLL stiffness operator and the diffusion smoothing (mm_gll_diffusion_apply, api.smooth_gll): the NumPy
statement in tests/diffusion_cases.py, which the kernel is compared with bit for bit on the GPU, is itself right -- it
annihilates constants, gives the Dirichlet energy of linear fields, is symmetric, and its backward-Euler steps scale an
eigenfunction by the stated symbol at the order of the elements -- and the library exports what the header declares.
Every bound is a term-count bound or a convergence order, none is a tolerance chosen from a result."""
import ctypes as C
import math

import numpy as np
import pytest

import diffusion_cases as DC
import mass_cases as M
from multimesh_amd import api, helpers, synth

SYMBOLS = ("mm_gll_diffusion_apply", "mm_pcg_combine", "mm_pcg_scalars", "mm_pcg_direction", "mm_pcg_advance")
EPS = M.EPS
SHAPES = [(1, 2), (2, 2), (4, 2), (1, 3), (2, 3), (4, 3)]
R0, R1 = 5_971_000.0, 6_371_000.0


def _tables(order):
    _, w, D = api.gll_quadrature(order)
    return w, D


def _mesh(order, dim):
    return synth.gll_mesh(5 if dim == 3 else 9, order, seed=3, dim=dim)


@pytest.mark.parametrize("order,dim", SHAPES)
def test_constants_are_in_the_kernel(order, dim):
    """(K 1)[p] = sum_q K_e[p][q]: P terms, within P * 2^-52 * sum_q |K_e[p][q]| of zero."""
    gp = _mesh(order, dim)
    w, D = _tables(order)
    E, P, _ = gp.shape
    y = DC.apply(gp, order, w, D, np.ones((1, E, P)))[0]
    Ke = DC.element_matrices(gp, order, w, D)
    bound = P * EPS * np.abs(Ke).sum(axis=2)
    print(f"order {order} dim {dim}: max |K 1| / bound = {(np.abs(y) / bound).max():.3e}")
    assert (np.abs(y) <= bound).all()


@pytest.mark.parametrize("order,dim", SHAPES)
def test_linear_field_has_the_energy_of_its_gradient(order, dim):
    """u = a . x is in the element's space whatever the geometry, and its gradient is a at every node:
    u^T K u = |a|^2 sum(mass), a sum of E * P terms u[p] (K u)[p]."""
    gp = _mesh(order, dim)
    w, D = _tables(order)
    a = np.array([1.5, -2.0, 3.0])[:dim]
    u = gp @ a
    Ku = DC.apply(gp, order, w, D, u)[0]
    mass, _ = M.mass(gp, order, w, D)
    got, exact = math.fsum((u * Ku).ravel()), float(a @ a) * math.fsum(mass.ravel())
    bound = M.term_bound(u * Ku)
    print(f"order {order} dim {dim}: u^T K u = {got!r}, |a|^2 sum(mass) = {exact!r}, bound {bound:.3e}")
    assert abs(got - exact) <= bound


def test_radial_and_lateral_energy_on_an_earth_chunk():
    """kappa = kh (1 - r r^T) + kr r r^T: u^T K u = sum_n mass_n (kh |a|^2 + (kr - kh) (r_n . a)^2), the right side formed
    from the coordinates alone.  Bound: the term count times |x| / h, as tests/test_mass.py::test_chunk_volume_at_order_4."""
    gp = synth.earth_chunk(4, nlat=4, nlon=4)["points"]
    w, D = _tables(4)
    kh, kr = 1.0, 0.25
    a = np.array([1.5, -2.0, 3.0])
    u = gp @ a
    Ku = DC.apply(gp, 4, w, D, u, kh=kh, kr=kr)[0]
    mass, _ = M.mass(gp, 4, w, D)
    rhat = gp / np.linalg.norm(gp, axis=-1, keepdims=True)
    exact = math.fsum((mass * (kh * float(a @ a) + (kr - kh) * (rhat @ a) ** 2)).ravel())
    got = math.fsum((u * Ku).ravel())
    bound = mass.size * EPS * (R1 / ((R1 - R0) / 4.0))
    print(f"chunk: relative difference {abs(got - exact) / exact:.3e}, bound {bound:.3e}")
    assert abs(got - exact) <= bound * exact
    # and the split matters: the isotropic operator gives another number
    iso = math.fsum((u * DC.apply(gp, 4, w, D, u, kh=kh)[0]).ravel())
    assert abs(iso - exact) > 1e-3 * exact
    # kr = kh is the isotropic operator up to rounding: (kr - kh) = 0 removes the radial term
    same = DC.apply(gp, 4, w, D, u, kh=kh, kr=kh)[0]
    assert abs(math.fsum((u * same).ravel()) - iso) <= bound * iso


@pytest.mark.parametrize("order,dim", SHAPES)
def test_symmetry(order, dim):
    gp = DC.welded(_mesh(order, dim))
    w, D = _tables(order)
    E, P, _ = gp.shape
    nu, inv = DC.unique_nodes(gp)
    assert nu == (order * ((5 if dim == 3 else 9) - 1) + 1) ** dim
    rng = np.random.default_rng(order * 10 + dim)
    u, v = rng.normal(size=nu)[inv].reshape(E, P), rng.normal(size=nu)[inv].reshape(E, P)
    kappa = rng.uniform(0.5, 2.0, size=(E, P))
    Ku = DC.apply(gp, order, w, D, u, kh=0.7, kh_array=kappa)[0]
    Kv = DC.apply(gp, order, w, D, v, kh=0.7, kh_array=kappa)[0]
    left, right = math.fsum((v * Ku).ravel()), math.fsum((u * Kv).ravel())
    bound = M.term_bound(v * Ku) + M.term_bound(u * Kv)
    print(f"order {order} dim {dim}: |v^T K u - u^T K v| = {abs(left - right):.3e}, bound {bound:.3e}")
    assert abs(left - right) <= bound


def _symbol_error(order, n, sigma=0.3, steps=4):
    gp = DC.welded(synth.gll_mesh(n, order, seed=3))
    assert DC.unique_nodes(gp)[0] == (order * (n - 1) + 1) ** 3
    w, D = _tables(order)
    f = np.cos(np.pi * gp[..., 0])[None]
    u, u0, Mu, _ = DC.smooth_direct(gp, order, w, D, f, steps, kh=sigma * sigma)
    return DC.m_norm(Mu, u[0] - DC.gaussian_symbol(sigma, np.pi ** 2, steps) * u0[0])


def test_smoothing_scales_an_eigenfunction_by_the_symbol():
    """cos(pi x) is an eigenfunction of the Laplacian of the unit cube under natural boundaries (eigenvalue pi^2): steps
    backward-Euler steps scale it by (1 + sigma^2 pi^2 / (2 steps))^-steps.  The nodal values of cos(pi x) are that
    eigenfunction up to the interpolation error of the elements, O(h^(order + 1)), at worst O(h^order) (the rate of its
    gradient): halving h must divide the M-norm error by more than 2^order.  Observed on the statement: 13.0 at order 2
    (4.19e-3 -> 3.22e-4), 32.3 at order 4 (9.81e-6 -> 3.03e-7)."""
    for order, lower in ((2, 4.0), (4, 16.0)):
        e3, e5 = _symbol_error(order, 3), _symbol_error(order, 5)
        print(f"order {order}: M-norm errors {e3:.3e} {e5:.3e}, ratio {e3 / e5:.2f}")
        assert e3 / e5 > lower, (order, e3, e5)


def test_library_exports_the_diffusion_symbols():
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "multimesh_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = helpers.load_lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in the header"
        assert name in helpers.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"{name} missing from {lib._filename}"
        assert getattr(lib, name).restype is C.c_int
    for slot in ("RZ", "RZ_OLD", "PAP", "BB", "ALPHA", "BETA", "ACTIVE", "PHASE_START", "PHASE_BETA", "PHASE_ALPHA"):
        value = re.search(r"#define\s+MM_PCG_%s\s+(\d+)" % slot, header)
        assert value and int(value.group(1)) == getattr(helpers, "MM_PCG_" + slot), slot


def test_argument_validation_needs_no_gpu():
    lib = helpers.load_lib()
    assert lib.mm_gll_diffusion_apply(None, 4, 3, None, 0, None, None, None, 1, 1.0, None, 0, 0.0, None, None) == -1
    assert lib.mm_pcg_combine(None, None, None, 0.0, None, 0, 1, None) == -1        # null ctx: MM_ERR_ARG
    assert lib.mm_pcg_scalars(None, None, 0, 0, 1e-10, None) == -1
    assert lib.mm_pcg_direction(None, None, None, 0, 1, None) == -1
    assert lib.mm_pcg_advance(None, None, None, None, 0, 1, None, None) == -1
    assert b"null" in lib.mm_last_error()
    assert callable(api.smooth_gll) and callable(api.gll_stiffness_apply) and callable(api.gll_roughness)


def test_sigma_is_validated_before_anything_runs():
    """Every ValueError of smooth_gll is raised before a context is touched (context=object() would fail otherwise)."""
    gp = synth.gll_mesh(3, 2, seed=3)
    mesh = api.GllMesh(gp, 2, {"f": np.ones(gp.shape[:2])})
    gp2 = synth.gll_mesh(4, 2, seed=3, dim=2)
    bad = object()
    for sigma in (-1.0, float("nan"), float("inf"), np.ones(5), np.ones((2,) + gp.shape[:2]), (1.0, -2.0), (1.0, 2.0, 3.0),
                  np.full(gp.shape[:2], -0.5)):
        with pytest.raises(ValueError):
            api.smooth_gll(mesh, ["f"], sigma, context=bad)
    with pytest.raises(ValueError):
        api.smooth_gll(api.GllMesh(gp2, 2), np.ones(gp2.shape[:2]), (1.0, 0.5), context=bad)    # a pair on a 2-D mesh
    with pytest.raises(ValueError):
        api.smooth_gll(api.GllMesh(np.zeros((2, 64, 3)), 3), np.ones((2, 64)), 1.0, context=bad)  # an order without tables
    with pytest.raises(ValueError):
        api.smooth_gll(mesh, np.ones((3, 4)), 1.0, context=bad)                                   # params of the wrong shape
    for kwargs in (dict(steps=0), dict(rtol=0.0), dict(rtol=2.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            api.smooth_gll(mesh, ["f"], 1.0, context=bad, **kwargs)
    with pytest.raises(ValueError):
        api.gll_stiffness_apply(mesh, ["f"], sigma=-1.0, context=bad)
