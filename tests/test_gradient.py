"""CPU side of the GLL gradient (mm_gll_gradient, api.gll_gradient / gll_gradient_parts): the NumPy statement in
tests/gradient_cases.py, which the kernel is compared with bit for bit on the GPU, is itself right -- it differentiates a
linear field to its constant gradient on distorted elements, its energy is the roughness u^T K u of the stiffness
statement, and on an elliptic Earth chunk it splits the gradient of |x| into a radial derivative of one and a lateral part
that vanishes with the order of the geometry -- and the library exports what the header declares."""
import ctypes as C
import math

import numpy as np
import pytest

import diffusion_cases as DC
import gradient_cases as GC
import mass_cases as M
from multimesh_amd import api, helpers, synth

SYMBOLS = ("mm_gll_gradient",)
EPS = M.EPS
SHAPES = [(1, 2), (2, 2), (4, 2), (1, 3), (2, 3), (4, 3)]
# u = |x| / 1000 on earth_chunk(order, nlat=5, nlon=6, ellipticity=3.3e-3, topography=3e-4): the relative error of the
# radial derivative against 1e-3 (asserted at ten times these), and the largest lateral / 1e-3 (3.6e-2, 9.9e-6, 2.1e-7:
# only its fall with the order is asserted, and lateral <= 1e-5 |grad u| at order 4).
RADIAL_OBSERVED = {1: 1.8e-14, 2: 1.1e-13, 4: 4.9e-13}
A, SIDE = GC.A, GC.SIDE


def _tables(order):
    _, w, D = api.gll_quadrature(order)
    return w, D


def _mesh(order, dim):
    return synth.gll_mesh(SIDE[dim], order, seed=3, dim=dim)


@pytest.mark.parametrize("order,dim", SHAPES)
def test_linear_field_has_a_constant_gradient(order, dim):
    """u = a . x + b is in the element's space whatever the geometry: grad u = a at every node, to rounding."""
    gp = _mesh(order, dim)
    _, D = _tables(order)
    a = A[:dim]
    grad, radial, lateral, norm = GC.gradient(gp, order, D, gp @ a + 0.75)
    assert grad.shape == (1, dim) + gp.shape[:2] and norm.shape == (1,) + gp.shape[:2]
    assert (radial is None and lateral is None) if dim == 2 else radial.shape == lateral.shape == norm.shape
    err = np.abs(grad[0] - a[:, None, None]).max()
    bound, multiple = GC.linear_bound(order, dim, D)
    print(f"order {order} dim {dim}: max |gr - a| = {err:.2e}, bound {bound:.2e} = {multiple:.1f} EPS max|a| cond")
    assert err <= bound
    assert np.abs(norm[0] - np.linalg.norm(a)).max() <= 2.0 * bound       # |d norm| <= |d gr|_2 <= sqrt(3) max|d gr|


@pytest.mark.parametrize("order,dim", SHAPES)
def test_energy_of_the_gradient_is_the_roughness(order, dim):
    """sum mass ((gr0^2 + gr1^2) + gr2^2) = sum u (K u) with K u of diffusion_cases.apply at kappa = 1: the two statements
    describe one operator.  Observed relative difference <= 2.3e-16 on the six shapes; asserted 1e-13."""
    gp = _mesh(order, dim)
    w, D = _tables(order)
    rng = np.random.default_rng(order * 10 + dim)
    u = rng.normal(size=gp.shape[:2])
    grad = GC.gradient(gp, order, D, u)[0][0]
    _, mass, _ = DC.geometry(gp, order, w, D)
    mass = mass.reshape(gp.shape[:2])
    sq = grad[0] * grad[0] + grad[1] * grad[1]
    if dim == 3:
        sq = sq + grad[2] * grad[2]
    energy = math.fsum((mass * sq).ravel())
    rough = math.fsum((u * DC.apply(gp, order, w, D, u)[0]).ravel())
    print(f"order {order} dim {dim}: relative difference {abs(energy - rough) / rough:.2e}")
    assert abs(energy - rough) <= 1e-13 * rough


def test_radial_and_lateral_parts_on_an_earth_chunk():
    """u = |x| / 1000 has the radial derivative 1e-3 and no lateral gradient.  |x| is not in the element's space: what is
    left is the interpolation error of the geometry, which falls with the order."""
    worst = {}
    for order in (1, 2, 4):
        gp = synth.earth_chunk(order, nlat=5, nlon=6, ellipticity=3.3e-3, topography=3e-4)["points"]
        _, D = _tables(order)
        _, radial, lateral, norm = GC.gradient(gp, order, D, np.linalg.norm(gp, axis=-1) / 1000.0)
        err = np.abs(radial - 1e-3).max() / 1e-3
        worst[order] = lateral.max() / 1e-3
        print(f"order {order}: radial error {err:.2e}, largest lateral / 1e-3 {worst[order]:.2e}")
        assert err <= 10.0 * RADIAL_OBSERVED[order], order
        if order == 4:
            assert (lateral <= 1e-5 * norm).all()
    assert worst[1] > worst[2] > worst[4]


def test_parts_need_a_3d_mesh():
    """ValueError before any device is touched (context=object() would fail otherwise), naming the function to use."""
    gp2 = synth.gll_mesh(4, 2, seed=3, dim=2)
    mesh = api.GllMesh(gp2, 2, {"f": np.ones(gp2.shape[:2])})
    with pytest.raises(ValueError, match="gll_gradient"):
        api.gll_gradient_parts(mesh, ["f"], context=object())
    with pytest.raises(ValueError):
        api.gll_gradient(mesh, np.ones((3, 4)), context=object())                                # params of the wrong shape
    with pytest.raises(ValueError):
        api.gll_gradient(api.GllMesh(np.zeros((2, 64, 3)), 3), np.ones((2, 64)), context=object())  # an order without tables


def test_library_exports_the_gradient_symbol():
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


def test_argument_validation_needs_no_gpu():
    lib = helpers.load_lib()
    assert lib.mm_gll_gradient(None, 4, 3, None, 0, None, None, 1, None, None, None, None) == -1   # null ctx: MM_ERR_ARG
    assert b"null" in lib.mm_last_error()
    assert callable(api.gll_gradient) and callable(api.gll_gradient_parts)
