"""CPU side of the GLL mass matrix (mm_gll_mass, mm_weighted_sum): the quadrature tables the kernel is fed are a GLL rule
(checked against an independent construction), the NumPy statement in tests/mass_cases.py integrates what a GLL rule of
its order integrates exactly and converges at the rule's order where it does not, and the library exports what the
header declares.  Every bound is a term-count bound or a convergence order, none is a tolerance chosen from a result."""
import ctypes as C
import math

import numpy as np
import pytest

import mass_cases as M
from multimesh_amd import api, helpers, synth

SYMBOLS = ("mm_gll_mass", "mm_weighted_sum", "mm_divide_rows")
EPS = M.EPS
ORDERS = (1, 2, 4)
R0, R1 = 5_971_000.0, 6_371_000.0


def _mass(gp, order):
    _, w, D = api.gll_quadrature(order)
    return M.mass(gp, order, w, D)


@pytest.mark.parametrize("order", ORDERS)
def test_tables_are_a_gll_rule(order):
    g, w, D = api.gll_quadrature(order)
    assert np.array_equal(g, synth.gll_nodes_1d(order)) and w.shape == (order + 1,) and D.shape == (order + 1, order + 1)
    assert abs(w.sum() - 2.0) <= 4 * EPS
    assert (np.abs(D.sum(axis=1)) <= 4 * EPS).all()
    # D differentiates x^q, q <= order, at the nodes: a sum of order + 1 products with |x| <= 1 per row
    bound = (order + 1) * EPS * np.abs(D).sum(axis=1)
    for q in range(order + 1):
        exact = q * g ** (q - 1) if q else np.zeros_like(g)
        assert (np.abs(D @ g ** q - exact) <= bound).all(), q


@pytest.mark.parametrize("order", ORDERS)
def test_tables_agree_with_an_independent_construction(order):
    g, w, D = api.gll_quadrature(order)
    w_ref, D_ref = M.independent_tables(g)
    assert np.abs(w - w_ref).max() <= 4 * EPS
    # each entry is at most order + 1 terms of the size of max|D|, and the two constructions round differently
    assert np.abs(D - D_ref).max() <= 2 * (order + 1) * EPS * np.abs(D).max()


@pytest.mark.parametrize("n", [5, 9])
@pytest.mark.parametrize("order", [2, 4])
def test_cube_volume_and_linear_integral_are_exact(order, n):
    """det J of a trilinear map has degree 2 per axis, times a linear field degree 3: within 2 * order - 1 for order >= 2."""
    gp = synth.gll_mesh(n, order, seed=3)
    mass, det = _mass(gp, order)
    assert M.n_bad(det) == 0 and (mass > 0).all()
    f = synth.field_linear(gp)
    for got, exact, terms in ((M.weighted_sum(mass)[0], 1.0, mass), (M.weighted_sum(mass, f[None])[0], 0.75, mass * f)):
        print(f"order {order} n {n}: error {got - exact:.3e}, bound {M.term_bound(terms):.3e}")
        assert abs(got - exact) <= M.term_bound(terms)
        assert abs(math.fsum(terms.ravel()) - exact) <= M.term_bound(terms)


@pytest.mark.parametrize("n", [5, 9])
def test_cube_volume_at_order_1_is_not_exact(n):
    """The rule is exact to degree 2 * order - 1 = 1 only: an over-integrating kernel, or one of the wrong order, would
    give 1 here."""
    gp = synth.gll_mesh(n, 1, seed=3)
    mass, det = _mass(gp, 1)
    assert M.n_bad(det) == 0
    assert abs(math.fsum(mass.ravel()) - 1.0) > 1e-7


def _chunk_error(order, nl):
    chunk = synth.earth_chunk(order, nlat=nl, nlon=nl)
    mass, det = _mass(chunk["points"], order)
    assert M.n_bad(det) == 0
    exact = M.chunk_volume(R0, R1, 8.0, 16.0)
    return (math.fsum(mass.ravel()) - exact) / exact, mass


@pytest.mark.parametrize("nl", [4, 8])
def test_chunk_volume_at_order_4(nl):
    rel, mass = _chunk_error(4, nl)
    # the term-count bound times |x| / h: the coordinates are of size r, the differences J is made of of the size of an
    # element (the thinnest edge: a quarter of the shell), the factor of MM_FP_TOL's bound
    bound = mass.size * EPS * (R1 / ((R1 - R0) / 4.0))
    print(f"order 4 nl {nl}: relative error {rel:.3e}, bound {bound:.3e}")
    assert abs(rel) <= bound


def test_chunk_volume_converges_at_the_order_of_the_rule():
    for order, lo, hi in ((2, 12.0, 20.0), (1, 3.5, 5.0)):
        e4, e8 = _chunk_error(order, 4)[0], _chunk_error(order, 8)[0]
        print(f"order {order}: relative errors {e4:.3e} {e8:.3e}, ratio {e4 / e8:.2f}")
        assert lo <= e4 / e8 <= hi, (order, e4, e8)


@pytest.mark.parametrize("order,dim", [(1, 2), (2, 2), (4, 2), (1, 3), (2, 3), (4, 3)])
def test_a_mirrored_element_is_counted(order, dim):
    gp = synth.gll_mesh(6, order, seed=3, dim=dim)
    mass, det = _mass(gp, order)
    e = len(gp) // 2
    mass_m, det_m = _mass(M.mirrored(gp, e), order)
    P = gp.shape[1]
    assert M.n_bad(det) == 0 and M.n_bad(det_m) == P and (det_m[e] < 0).all()
    keep = np.arange(len(gp)) != e
    assert M.same_bits(mass_m[keep], mass[keep]) and (mass_m[e] > 0).all()


def test_square_area_in_2d():
    for order in (2, 4):
        gp = synth.gll_mesh(7, order, seed=3, dim=2)
        mass, det = _mass(gp, order)
        assert M.n_bad(det) == 0 and abs(math.fsum(mass.ravel()) - 1.0) <= M.term_bound(mass)


def test_weighted_sum_statement():
    rng = np.random.default_rng(5)
    for n in (0, 1, 255, 4096, 4097, 3 * 4096 * 4096 // 1000):
        mass = rng.uniform(0.5, 1.5, size=n)
        f = rng.normal(size=(2, n)) * 10.0 ** rng.uniform(-8, 8, size=(2, n))
        got = M.weighted_sum(mass, f)
        for c in range(2):
            assert abs(got[c] - math.fsum(mass * f[c])) <= M.term_bound(mass * f[c])
        assert abs(M.weighted_sum(mass)[0] - math.fsum(mass)) <= M.term_bound(mass)
    # the order is part of the statement: another one changes the bits
    mass = np.ones(20000)
    f = rng.normal(size=(1, 20000)) * 10.0 ** rng.uniform(-8, 8, size=(1, 20000))
    assert M.weighted_sum(mass, f)[0] != np.cumsum(f[0])[-1]


def test_library_exports_the_mass_symbols():
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "multimesh_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = helpers.load_lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in the header"
        assert name in helpers.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"{name} missing from {lib._filename}"
    assert lib.mm_gll_mass.restype is C.c_int64 and lib.mm_weighted_sum.restype is C.c_int


def test_argument_validation_needs_no_gpu():
    lib = helpers.load_lib()
    assert lib.mm_gll_mass(None, 4, 3, None, 0, None, None, None, None) == -1          # null ctx: MM_ERR_ARG
    assert lib.mm_weighted_sum(None, None, None, 0, 1, None) == -1
    assert lib.mm_divide_rows(None, None, None, 0, 1, None) == -1
    with pytest.raises(ValueError):
        api.gll_quadrature(3)


def test_multi_tile_cases_reach_a_third_step():
    """mass_cases.MULTI_TILE is what its comment says: tiles, the short last tile, and the blocks that take three steps."""
    expect = {4: (4098, 1, 2), 2: (4097, 5, 1)}                  # order -> tiles, elements of the last tile, blocks with 3 steps
    for order, side, nelem in M.MULTI_TILE:
        tile = M.tile_elems(order, 3)
        ntiles = -(-nelem // tile)
        assert nelem <= (side - 1) ** 3
        assert (ntiles, nelem - (ntiles - 1) * tile, ntiles - 2 * M.MAX_BLOCKS) == expect[order]
