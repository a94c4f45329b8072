"""CPU checks of the resolution statement (tests/resolution_cases.py) and of the module's surface: the vectorised statement
against an independent brute force, closed forms on a regular mesh, the pinned surface of multimesh_amd.resolution, and the
binding layer's two symbols.  The bit-exact form is the statement itself; the brute force is held to 1e-13 relative."""
import inspect
import itertools

import numpy as np
import pytest

import resolution_cases as RC
from multimesh_amd import api, helpers, resolution, synth
from multimesh_amd.api import GllMesh
from multimesh_amd.mesh import HexMesh

RTOL = 1e-13


def _brute(gp, order):
    """Per element, a Python loop over all node pairs that are tensor neighbours, and over the corner pairs that differ in
    one index, with np.linalg.norm: (h[E, P], edge_min[E], edge_max[E])."""
    E, P, dim = gp.shape
    m = order + 1
    index = {ijk: sum(v * m ** d for d, v in enumerate(ijk)) for ijk in itertools.product(range(m), repeat=dim)}
    h = np.full((E, P), np.inf)
    emin, emax = np.full(E, np.inf), np.full(E, -np.inf)
    for e in range(E):
        for a, pa in index.items():
            for b, pb in index.items():
                apart = [abs(x - y) for x, y in zip(a, b)]
                if sum(apart) == 1:
                    h[e, pa] = min(h[e, pa], np.linalg.norm(gp[e, pa] - gp[e, pb]))
                corners = all(x in (0, order) for x in a + b)
                if corners and pa < pb and sorted(apart) == [0] * (dim - 1) + [order]:
                    length = np.linalg.norm(gp[e, pa] - gp[e, pb])
                    emin[e], emax[e] = min(emin[e], length), max(emax[e], length)
    return h, emin, emax


@pytest.mark.parametrize("order,dim", [(1, 3), (2, 3), (4, 3), (1, 2), (2, 2), (4, 2)])
def test_the_statement_against_a_brute_force(order, dim):
    gp = synth.gll_mesh(3, order, seed=order + dim, jitter=0.25, dim=dim)
    fast, slow = RC.velocities(gp, 2, 1), RC.velocities(gp, 2, 2, lo=0.0, hi=4000.0)
    slow[:, 1] = 0.0                                                      # a fluid element: resolved by its P wavelength
    out, info, h = RC.resolution(gp, order, fast, slow)
    bh, bmin, bmax = _brute(gp, order)
    assert info.tolist() == [0, 0]
    np.testing.assert_allclose(h, bh, rtol=RTOL, atol=0)
    np.testing.assert_allclose(out[0], bh.min(axis=1), rtol=RTOL, atol=0)
    np.testing.assert_allclose(out[1], bmin, rtol=RTOL, atol=0)
    np.testing.assert_allclose(out[2], bmax, rtol=RTOL, atol=0)
    np.testing.assert_allclose(out[3], (bh / fast.max(axis=0)).min(axis=1), rtol=RTOL, atol=0)
    vslow = np.where(slow > 0, slow, np.inf).min(axis=0)
    vslow[1] = fast.min(axis=0)[1]
    np.testing.assert_allclose(out[4], bmax / vslow.min(axis=1), rtol=RTOL, atol=0)
    sizes, info3, _ = RC.resolution(gp, order)
    assert sizes.shape == (3, len(gp)) and RC.same_bits(sizes, out[:3]) and info3.tolist() == [0, 0]


@pytest.mark.parametrize("order,dim", [(1, 3), (2, 3), (4, 3), (4, 2)])
def test_closed_forms_on_a_regular_mesh(order, dim):
    n = 4
    gp = synth.gll_mesh(n, order, jitter=0.0, dim=dim)
    width = 1.0 / (n - 1)
    g = synth.gll_nodes_1d(order)
    out, _, h = RC.resolution(gp, order)
    # (the nodes come out of an 8-term floating sum of the corners: a few ulp, not bits)
    np.testing.assert_allclose(out[0], (g[1] - g[0]) / 2.0 * width, rtol=1e-12, atol=0)
    np.testing.assert_allclose(out[1], out[2], rtol=1e-12, atol=0)
    np.testing.assert_allclose(out[2], width, rtol=1e-12, atol=0)
    assert (h >= out[0][:, None]).all()


def test_validity_rules_of_the_statement():
    gp = synth.gll_mesh(3, 2, seed=9)
    fast, slow = RC.velocities(gp, 1, 3), RC.velocities(gp, 1, 4)
    gp[0, 5, 1] = np.nan
    fast[0, 1, 3] = np.inf
    fast[0, 2, 0] = 0.0
    slow[0, 3, 7] = -1.0
    gp[4, 1] = gp[4, 0]                                                    # coincident nodes: valid, step = 0
    out, info, h = RC.resolution(gp, 2, fast, slow)
    assert info.tolist() == [1, 4]
    assert np.isnan(out[:, 0]).all() and np.isnan(h[0]).all()
    assert np.isnan(out[3:, 1:4]).all() and np.isfinite(out[:3, 1:4]).all()
    assert out[0, 4] == 0.0 and out[3, 4] == 0.0 and np.isfinite(out[:, 4:]).all()


def test_arg_extreme_statement():
    row = np.array([np.nan, 3.0, -0.0, 0.0, 3.0, np.inf, np.nan])
    value, index, nvalid = RC.arg_extreme(row)
    assert index.tolist() == [2] and np.signbit(value[0]) and nvalid.tolist() == [5]
    value, index, _ = RC.arg_extreme(row, want_max=True)
    assert index.tolist() == [5] and value[0] == np.inf
    value, index, nvalid = RC.arg_extreme(np.full((2, 4), np.nan))
    assert np.isnan(value).all() and index.tolist() == [-1, -1] and nvalid.tolist() == [0, 0]


SURFACE = {
    "element_sizes": "(mesh, context=None)",
    "time_step": "(mesh, fast=None, courant=0.6, context=None)",
    "resolved_period": "(mesh, fast=None, slow=None, elements_per_wavelength=2.0, context=None)",
    "elements_per_wavelength": "(mesh, period, fast=None, slow=None, minimum=2.0, context=None)",
    "check_model": "(mesh, period, fast=None, slow=None, courant=0.6, elements_per_wavelength=2.0, context=None)",
}


def test_the_modules_surface():
    assert sorted(resolution.__all__) == sorted(SURFACE)
    for name, signature in SURFACE.items():
        fn = getattr(resolution, name)
        assert str(inspect.signature(fn)) == signature, name
        assert (fn.__doc__ or "").strip(), name
    assert "chord" in resolution.element_sizes.__doc__ and "chord" in resolution.resolved_period.__doc__
    assert "convention" in resolution.time_step.__doc__ and "convention" in resolution.resolved_period.__doc__
    assert len(api.__all__) == 71 and not set(SURFACE) & set(api.__all__)     # the api package is as it was
    assert resolution.ModelCheck.__doc__ and resolution.ModelCheck.ok.__doc__
    from multimesh_amd.device import Context
    for name in ("gll_resolution", "arg_extreme"):
        assert (getattr(Context, name).__doc__ or "").strip(), name     # (signatures: tests/test_device_calls.py)


def test_the_binding_layer_knows_the_two_symbols():
    lib = helpers.load_lib()
    for name, nargs in (("mm_gll_resolution", 12), ("mm_arg_extreme", 8)):
        assert name in helpers.EXPORTED_SYMBOLS
        assert len(helpers.SIGNATURES[name][1]) == nargs and len(getattr(lib, name).argtypes) == nargs
    order = list(helpers.EXPORTED_SYMBOLS)
    assert order.index("mm_distance_taper") + 1 == order.index("mm_gll_resolution") == order.index("mm_arg_extreme") - 1


def test_argument_mistakes_need_no_gpu():
    lib = helpers.load_lib()
    assert lib.mm_gll_resolution(None, 2, 3, None, 0, None, 0, None, 0, None, None, None) == -1
    assert b"ctx is null" in lib.mm_last_error()
    assert lib.mm_arg_extreme(None, None, 1, 0, 0, None, None, None) == -1
    gp = synth.gll_mesh(3, 2)
    with pytest.raises(ValueError, match="no fast velocity"):
        resolution.time_step(GllMesh(gp, 2, {"RHO": np.ones(gp.shape[:2])}))
    with pytest.raises(ValueError, match="has no field"):
        resolution.time_step(GllMesh(gp, 2, {"VP": np.ones(gp.shape[:2])}), fast="VPV")
    with pytest.raises(ValueError, match="courant must be positive"):
        resolution.time_step(GllMesh(gp, 2, {"VP": np.ones(gp.shape[:2])}), courant=0.0)
    with pytest.raises(ValueError, match=r"\[C, E, P\]"):
        resolution.time_step(GllMesh(gp, 2), fast=np.ones((2, 3)))
    with pytest.raises(ValueError, match="orders 1, 2 and 4"):
        resolution.element_sizes(GllMesh(np.zeros((2, 64, 3)), 3))
    pts, conn = synth.quad_mesh(3)
    with pytest.raises(ValueError, match="3-D hexahedral"):
        resolution.element_sizes(HexMesh(pts, conn))
