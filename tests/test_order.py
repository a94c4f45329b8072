"""CPU side of the order change (mm_gll_tensor_apply, api.gll_order_table / gll_order_apply / resample_gll_order /
restrict_gll_kernel / gll_change_order): the NumPy statement in tests/order_cases.py, which the kernel is compared with bit
for bit on the GPU, is itself right -- its tables sum to one and are unit rows at coinciding nodes, up then down is the
identity bit for bit, the transposed table is the adjoint, coordinates and polynomials of the input's degree are
reproduced, the restriction keeps the integral -- and the library checks its arguments without a device."""
import ctypes as C

import numpy as np
import pytest

import mass_cases as M
import order_cases as OC
from multimesh_amd import api, helpers, io as mio, synth

EPS = OC.EPS
MM_ERR_ARG = -1


@pytest.mark.parametrize("order_in,order_out", OC.PAIRS)
def test_tables_sum_to_one_and_are_unit_rows_at_coinciding_nodes(order_in, order_out):
    R = api.gll_order_table(order_in, order_out)
    assert R.shape == (order_out + 1, order_in + 1)
    assert M.same_bits(R, OC.table(order_in, order_out))                         # the package's table is the statement's
    assert M.same_bits(synth.gll_nodes_1d(order_in), OC.nodes(order_in))
    assert (np.abs(R.sum(axis=1) - 1.0) <= 2 * EPS).all()
    gi, go = OC.nodes(order_in), OC.nodes(order_out)
    shared = 0
    for q, x in enumerate(go):
        for a, g in enumerate(gi):
            if g == x:
                shared += 1
                assert np.array_equal(R[q], np.eye(order_in + 1)[a]), (q, a)
    assert shared == min(order_in, order_out) + 1                                # the coarser nodes are among the finer
    # against the Lagrange basis through another route: the Vandermonde solve
    V = np.vander(gi, increasing=True)
    ref = np.vander(go, order_in + 1, increasing=True) @ np.linalg.inv(V)
    assert np.abs(R - ref).max() <= 64 * EPS


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("order_in,order_out", OC.UP)
def test_up_then_down_is_the_identity_bit_for_bit(order_in, order_out, dim):
    rng = np.random.default_rng(order_in * 10 + order_out + dim)
    u = rng.normal(size=(2, 5, (order_in + 1) ** dim)) * 10.0 ** rng.uniform(-8, 8, size=(2, 5, 1))
    up = OC.tensor_apply(OC.table(order_in, order_out), dim, u)
    down = OC.tensor_apply(OC.table(order_out, order_in), dim, up)
    assert up.shape == (2, 5, (order_out + 1) ** dim)
    assert np.array_equal(down, u)


@pytest.mark.parametrize("order_in,order_out", OC.UP)
def test_transposed_table_is_the_adjoint(order_in, order_out):
    worst = 0.0
    for dim in (2, 3):
        rng = np.random.default_rng(10 * order_in + order_out + dim)
        u = rng.normal(size=(1, 7, (order_in + 1) ** dim))
        v = rng.normal(size=(1, 7, (order_out + 1) ** dim))
        Iu = OC.tensor_apply(OC.table(order_in, order_out), dim, u)
        Itv = OC.tensor_apply(OC.transposed_table(order_out, order_in), dim, v)
        assert Itv.shape == u.shape
        lhs, rhs = float(np.sum(Iu * v)), float(np.sum(u * Itv))
        worst = max(worst, abs(lhs - rhs))
    print(f"{order_in}->{order_out}: |<Iu,v> - <u,I^T v>| = {worst:.2e}")
    assert worst <= 10.0 * OC.ADJOINT_OBSERVED[(order_in, order_out)]


@pytest.mark.parametrize("order_in,order_out", OC.UP)
def test_upsampled_coordinates_are_the_finer_mesh(order_in, order_out):
    lo, hi = synth.gll_mesh(4, order_in, seed=3), synth.gll_mesh(4, order_out, seed=3)
    up = OC.tensor_apply(OC.table(order_in, order_out), 3, lo, layout=1)
    assert up.shape == hi.shape
    err = np.abs(up - hi).max()
    print(f"{order_in}->{order_out}: max |upsampled - finer mesh| = {err:.2e}")
    assert err <= 10.0 * OC.COORDS_OBSERVED[(order_in, order_out)]
    # and down again, in the coordinates' own layout
    assert np.array_equal(OC.tensor_apply(OC.table(order_out, order_in), 3, up, layout=1), lo)


def _poly(order_in, order_out, dim):
    rng = np.random.default_rng(100 + 10 * order_in + order_out + dim)
    coef = rng.normal(size=(dim, order_in + 1))

    def f(order):
        g = OC.nodes(order)
        per_axis = [sum(coef[d][n] * g ** n for n in range(order_in + 1)) for d in range(dim)]   # axis d = i, j, k
        full = per_axis[0]
        for d in range(1, dim):
            full = per_axis[d][(slice(None),) + (None,) * d] * full[None]
        return full.reshape(1, 1, -1)
    return f, float(np.prod(np.abs(coef).sum(axis=1)))


@pytest.mark.parametrize("order_in,order_out", OC.UP)
def test_polynomials_of_the_input_degree_are_reproduced(order_in, order_out):
    worst = 0.0
    for dim in (2, 3):
        f, size = _poly(order_in, order_out, dim)
        got = OC.tensor_apply(OC.table(order_in, order_out), dim, f(order_in))
        worst = max(worst, np.abs(got - f(order_out)).max() / size)
    print(f"{order_in}->{order_out}: max |I f - f| / size = {worst:.2e}")
    assert worst <= 10.0 * OC.POLY_OBSERVED[(order_in, order_out)]


@pytest.mark.parametrize("order_f,order_c", [(4, 2), (4, 1), (2, 1)])
def test_restriction_statement_keeps_the_integral(order_f, order_c):
    gp = synth.earth_chunk(order_f, nlat=3, nlon=3, ellipticity=3.3e-3, topography=3e-4)["points"]
    _, wf, Df = api.gll_quadrature(order_f)
    _, wc, Dc = api.gll_quadrature(order_c)
    coarse = OC.tensor_apply(OC.table(order_f, order_c), 3, gp, layout=1)
    Mf, Mc = M.mass(gp, order_f, wf, Df)[0], M.mass(coarse, order_c, wc, Dc)[0]
    Kf = np.random.default_rng(7).normal(size=(1,) + gp.shape[:2])
    Kc = OC.tensor_apply(OC.transposed_table(order_f, order_c), 3, Kf, scale_in=Mf, div_out=Mc)
    fine, coarse_int = M.weighted_sum(Mf, Kf)[0], M.weighted_sum(Mc, Kc)[0]
    rel = abs(fine - coarse_int) / M.weighted_sum(Mf, np.abs(Kf))[0]
    print(f"{order_f}->{order_c}: |int K_c - int K_f| / int |K_f| = {rel:.2e}")
    assert rel <= 10.0 * OC.RESTRICT_OBSERVED[(order_f, order_c)]
    # without the two masses it is the plain transpose; with only the division the two steps commute with the statement
    plain = OC.tensor_apply(OC.transposed_table(order_f, order_c), 3, Mf[None] * Kf)
    assert M.same_bits(plain / Mc[None], Kc)


def test_layouts_of_the_statement_agree():
    rng = np.random.default_rng(2)
    planes = rng.normal(size=(3, 4, 27))
    ref = OC.tensor_apply(OC.table(2, 4), 3, planes)
    for layout in (1, 2):
        got = OC.tensor_apply(OC.table(2, 4), 3, OC.from_planes(planes, layout), layout=layout)
        assert got.shape == ((4, 125, 3) if layout == 1 else (4, 3, 125))
        assert M.same_bits(OC.to_planes(got, layout), ref)
    nan = planes.copy()
    nan[0, 1, 13] = np.nan                                                         # the centre node of element 1
    out = OC.tensor_apply(OC.table(2, 4), 3, nan)
    assert np.isnan(out[0, 1]).all() and not np.isnan(out[0, 0]).any() and not np.isnan(out[1:]).any()   # 0 * NaN is NaN


def test_tile_formula():
    assert [OC.tile_elems(a, b, d) for a, b, d in OC.SHAPES] == [28, 10, 28, 10, 10, 10, 9, 2, 9, 2, 2, 2]


# ---------------------------------------------------------------------------------------------- the library, without a GPU
def test_library_exports_the_symbol():
    lib = helpers.load_lib()
    assert "mm_gll_tensor_apply" in helpers.EXPORTED_SYMBOLS and hasattr(lib, "mm_gll_tensor_apply")
    assert lib.mm_gll_tensor_apply.restype is C.c_int


def test_argument_validation_needs_no_gpu():
    """Every argument is judged before the context or a device is looked at, so a null context shows the checks: the
    message names what is wrong, and only arguments that are otherwise right reach "ctx is null".  No pointer is read."""
    lib = helpers.load_lib()
    fn, err = lib.mm_gll_tensor_apply, lib.mm_last_error
    buf = np.zeros(4096)
    a = buf.ctypes.data
    tab = a + 8 * 3000                                         # in = 2 x 27, out = 2 x 125 doubles: all inside buf
    far = a + 8 * 1000
    assert fn(None, 3, 2, 4, tab, 0, a, far, 2, 1, None, None) == MM_ERR_ARG and b"ctx is null" in err()
    cases = {
        b"equals": fn(None, 3, 2, 2, tab, 0, a, far, 2, 1, None, None),
        b"order_in": fn(None, 3, 3, 4, tab, 0, a, far, 2, 1, None, None),
        b"order_out": fn(None, 3, 2, 5, tab, 0, a, far, 2, 1, None, None),
        b"layout": fn(None, 3, 2, 4, tab, 3, a, far, 2, 1, None, None),
        b"dim": fn(None, 4, 2, 4, tab, 0, a, far, 2, 1, None, None),
        b"nelem": fn(None, 3, 2, 4, tab, 0, a, far, -1, 1, None, None),
        b"ncomp": fn(None, 3, 2, 4, tab, 0, a, far, 2, 65536, None, None),
        b"null table": fn(None, 3, 2, 4, None, 0, a, far, 2, 1, None, None),
        b"null array": fn(None, 3, 2, 4, tab, 0, None, far, 2, 1, None, None),
        b"overlap in_d": fn(None, 3, 2, 4, tab, 0, a, a, 2, 1, None, None),
        b"overlap scale_in_d": fn(None, 3, 2, 4, tab, 0, a, far, 2, 1, far + 8 * 249, None),
        b"overlap div_out_d": fn(None, 3, 2, 4, tab, 0, a, far, 2, 1, None, far),
    }
    for what, rc in cases.items():
        assert rc == MM_ERR_ARG, what
    for what, args in {
        b"equals": (3, 2, 2, tab, 0, a, far, 2, 1, None, None),
        b"layout": (3, 2, 4, tab, -1, a, far, 2, 1, None, None),
        b"dim": (4, 2, 4, tab, 0, a, far, 2, 1, None, None),
        b"overlap in_d": (3, 2, 4, tab, 0, a, a + 8 * 53, 2, 1, None, None),          # the last double of in_d
        b"overlap scale_in_d": (3, 2, 4, tab, 0, a, far, 2, 1, far + 8 * 249, None),  # the last double of out_d
        b"overlap div_out_d": (3, 2, 4, tab, 0, a, far, 2, 1, None, far - 8 * 249),
    }.items():
        assert fn(None, *args) == MM_ERR_ARG
        assert what in err(), (what, err())
    # neighbours are not an overlap: these get as far as the context
    assert fn(None, 3, 2, 4, tab, 0, a, a + 8 * 54, 2, 1, None, None) == MM_ERR_ARG and b"ctx is null" in err()
    assert fn(None, 3, 2, 4, tab, 0, a, far, 2, 1, far - 8 * 54, far + 8 * 250) == MM_ERR_ARG and b"ctx is null" in err()
    assert not buf.any()


def test_element_deviation_statement_and_argument_validation_without_a_gpu():
    b = synth.gll_mesh(3, 2, seed=3)
    a = b.copy()
    a[2, 5, 1] += 0.25
    a[4, 26, 2] = np.nan
    dev, edge = OC.element_deviation(a, b)
    assert dev[2] == abs(a[2, 5, 1] - b[2, 5, 1]) > 0 and np.isnan(dev[4]) and not dev[[0, 1, 3, 5, 6, 7]].any()
    assert np.array_equal(edge, (b.max(axis=1) - b.min(axis=1)).max(axis=1))
    lib = helpers.load_lib()
    fn, err = lib.mm_element_deviation, lib.mm_last_error
    assert "mm_element_deviation" in helpers.EXPORTED_SYMBOLS and len(fn.argtypes) == 8 and fn.restype is C.c_int
    buf = np.zeros(1024)
    p = buf.ctypes.data                                        # a, b = 2 x 27 x 3 = 162 doubles each; 2 + 2 outputs
    a_, b_, d_, e_ = p, p + 8 * 162, p + 8 * 324, p + 8 * 326
    assert fn(None, 3, 27, a_, b_, 2, d_, e_) == MM_ERR_ARG and b"ctx is null" in err()
    for what, args in {
        b"dim": (4, 27, a_, b_, 2, d_, e_),
        b"npts": (3, 0, a_, b_, 2, d_, e_),
        b"nelem": (3, 27, a_, b_, -1, d_, e_),
        b"null array": (3, 27, a_, None, 2, d_, e_),
        b"deviation_d must not overlap an input": (3, 27, a_, b_, 2, d_ - 8, e_),        # the last double of b
        b"edge_d must not overlap an input": (3, 27, a_, b_, 2, d_, a_ + 8 * 161),
        b"edge_d must not overlap deviation_d": (3, 27, a_, b_, 2, d_, d_ + 8),
    }.items():
        assert fn(None, *args) == MM_ERR_ARG
        assert what in err(), (what, err())
    assert not buf.any()


# ---------------------------------------------------------------------------------------------- the Python layer, without a GPU
def test_same_order_is_a_copy_and_bad_arguments_raise_before_a_device():
    gp = synth.gll_mesh(3, 2, seed=3)
    u = np.random.default_rng(0).normal(size=gp.shape[:2])
    mesh = api.GllMesh(gp, 2, {"f": u})
    same = api.resample_gll_order(mesh, 2, context=object())
    assert same.shape_order == 2 and np.array_equal(same.gll_points, gp) and np.array_equal(same.element_nodal_fields["f"], u)
    assert same.gll_points is not mesh.gll_points and same.element_nodal_fields["f"] is not mesh.element_nodal_fields["f"]
    got = api.gll_order_apply(u, 2, 2, 3, context=object())
    assert np.array_equal(got, u) and got is not u
    with pytest.raises(ValueError):
        api.resample_gll_order(mesh, 3, context=object())
    with pytest.raises(ValueError):
        api.gll_order_apply(u, 4, 2, 3, context=object())                         # 27 nodes are not order 4
    with pytest.raises(ValueError):
        api.gll_order_apply(u, 2, 4, 4, context=object())
    with pytest.raises(ValueError, match="goes down"):
        api.restrict_gll_kernel(mesh, 4, context=object())
    with pytest.raises(ValueError, match="goes down"):
        api.restrict_gll_kernel(mesh, 2, context=object())


def _model_file(points, names, data):
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=points)
    ds = f.create_dataset("MODEL/data", data=data)
    mio.set_dimension_labels(ds, names)
    return f


def test_change_order_plan_and_what_it_refuses_without_a_device():
    plan = api._change_order_plan
    assert plan((7, 27, 3), (7, 125, 3), (7, 2, 27), ["VP", "RHO"], "all", False) == (2, 4, 3, ["VP", "RHO"], [0, 1])
    assert plan((7, 25, 2), (7, 4, 2), (7, 2, 25), ["VP", "RHO"], ["RHO"], True) == (4, 1, 2, ["RHO"], [1])
    assert plan((7, 8, 3), (7, 8, 3), (7, 1, 8), ["VP"], "VP", False) == (1, 1, 3, ["VP"], [0])
    for args in [((7, 27, 3), (8, 125, 3), (7, 2, 27), ["VP", "RHO"], "all", False),      # another element count
                 ((7, 27, 3), (7, 64, 3), (7, 2, 27), ["VP", "RHO"], "all", False),       # order 3
                 ((7, 27, 3), (7, 25, 2), (7, 2, 27), ["VP", "RHO"], "all", False),       # 3-D onto 2-D
                 ((7, 27, 3), (7, 125, 3), (7, 2, 27), ["VP", "RHO"], "all", True),       # a restriction going up
                 ((7, 27, 3), (7, 27, 3), (7, 2, 27), ["VP", "RHO"], "all", True),        # ... or nowhere
                 ((7, 27, 3), (7, 125, 3), (7, 2, 27), ["VP", "RHO"], ["VS"], False),     # a parameter the source lacks
                 ((7, 27, 3), (7, 125, 3), (7, 3, 27), ["VP", "RHO"], "all", False)]:     # data that is not [E, C, P]
        with pytest.raises(ValueError):
            plan(*args)
    # through the driver: refused before a context is asked for, and the receiving file is left as it was
    lo, hi = synth.gll_mesh(3, 2, seed=3), synth.gll_mesh(3, 4, seed=3)
    src = _model_file(hi, ["VP"], np.ones((8, 1, 125)))
    dst = _model_file(lo, ["VP"], np.full((8, 1, 27), 5.0))
    with pytest.raises(ValueError, match="goes down"):
        api.gll_change_order(dst, src, kernel=True, context=object())
    with pytest.raises(ValueError, match="same elements"):
        api.gll_change_order(_model_file(hi[:7], ["VP"], np.ones((7, 1, 125))), dst, context=object())
    assert np.array_equal(dst["MODEL/data"][:], np.full((8, 1, 27), 5.0))
    assert np.array_equal(src["MODEL/data"][:], np.ones((8, 1, 125)))
