"""The order change on the GPU.  mm_gll_tensor_apply is compared BIT for bit with its NumPy statement (tests/order_cases.py):
the 12 (order_in, order_out, dim) kernels in the three layouts with one and three components, element counts around the
tile of a 256-thread block, the scale and the division (pointer tests in the kernel), Earth-scale coordinates where they
lie, the transpose through R.T, and the Python layers over it.  Inputs have full mantissas (transpose_cases.wide).
mm_element_deviation, the check of the file driver, is compared with its statement in the same way."""
import numpy as np
import pytest

import mass_cases as M
import order_cases as OC
import transpose_cases as T
from multimesh_amd import api, helpers, io as mio, synth
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context

pytestmark = pytest.mark.gpu

MM_ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def _raw(ctx, R, order_in, order_out, dim, values, layout, scale=None, div=None):
    """Straight at the ABI -> the result as a NumPy array in ``layout``."""
    C, E, _ = OC.to_planes(values, layout).shape
    pout = (order_out + 1) ** dim
    out = ctx.empty(((C, E, pout), (E, pout, C), (E, C, pout))[layout], np.float64)
    v_d, R_d = ctx.to_device(np.ascontiguousarray(values)), ctx.to_device(np.ascontiguousarray(R))
    s_d = ctx.to_device(scale) if scale is not None else None
    d_d = ctx.to_device(div) if div is not None else None
    rc = ctx.lib.mm_gll_tensor_apply(ctx.handle, dim, order_in, order_out, R_d.ptr, layout, v_d.ptr, out.ptr, E, C,
                                     s_d.ptr if s_d else None, d_d.ptr if d_d else None)
    assert rc == 0, helpers.load_lib().mm_last_error()
    return out.numpy()


def _check(ctx, order_in, order_out, dim, nelem, ncomp, layout, seed, scale=False, div=False, R=None):
    rng = np.random.default_rng(seed)
    pin, pout = (order_in + 1) ** dim, (order_out + 1) ** dim
    values = OC.from_planes(T.wide(rng, (ncomp, nelem, pin)), layout)
    s = rng.uniform(0.5, 2.0, size=(nelem, pin)) * 10.0 ** rng.uniform(-3, 3, size=(nelem, 1)) if scale else None
    d = rng.uniform(0.5, 2.0, size=(nelem, pout)) * 10.0 ** rng.uniform(-3, 3, size=(nelem, 1)) if div else None
    R = OC.table(order_in, order_out) if R is None else R
    ref = OC.tensor_apply(R, dim, values, layout, s, d)
    got = _raw(ctx, R, order_in, order_out, dim, values, layout, s, d)
    what = (order_in, order_out, dim, nelem, ncomp, layout, scale, div)
    assert got.shape == ref.shape, what
    assert M.same_bits(got, ref), (what, int((got != ref).sum()), ref.size)


def _nelem(dim):
    """The elements of synth.gll_mesh(6, ...) in 3-D and gll_mesh(16, ..., dim=2): 125 / 225."""
    return len(synth.gll_mesh(6 if dim == 3 else 16, 1, seed=3, dim=dim))


# ---------------------------------------------------------------------------------------------- mm_gll_tensor_apply
@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("order_in,order_out,dim", OC.SHAPES)
def test_bit_for_bit_in_every_layout(ctx, order_in, order_out, dim, layout, ncomp):
    _check(ctx, order_in, order_out, dim, _nelem(dim), ncomp, layout, 1000 * order_in + 100 * order_out + 10 * dim + layout)


@pytest.mark.parametrize("order_in,order_out,dim", OC.SHAPES)
def test_element_counts_around_a_tile(ctx, order_in, order_out, dim):
    tile = OC.tile_elems(order_in, order_out, dim)
    counts = (0, 1, tile - 1, tile, tile + 1, 3 * tile + max(tile // 2, 1))
    assert max(counts) <= _nelem(dim)
    for nelem in counts:
        _check(ctx, order_in, order_out, dim, nelem, 2, 0, nelem + 7)
    # layout 2 takes TILE items of the tile's run per step: an item count that is no multiple of the tile
    _check(ctx, order_in, order_out, dim, 3 * tile + 1, 3, 2, 5)
    _check(ctx, order_in, order_out, dim, tile + 1, 5, 2, 6)


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("order_in,order_out,dim", [(4, 2, 3), (2, 4, 3), (1, 2, 3), (4, 1, 2), (2, 4, 2)])
def test_scale_and_division_alone_and_together(ctx, order_in, order_out, dim, layout):
    tile = OC.tile_elems(order_in, order_out, dim)
    for scale, div in ((True, False), (False, True), (True, True)):
        _check(ctx, order_in, order_out, dim, 2 * tile + 1, 3, layout, 31 + layout, scale=scale, div=div)


@pytest.mark.parametrize("order_in,order_out", [(1, 4), (2, 4), (4, 2)])
def test_earth_coordinates_where_they_lie(ctx, order_in, order_out):
    gp = synth.earth_chunk(order_in, nlat=5, nlon=6, ellipticity=3.3e-3, topography=3e-4)["points"]
    assert np.abs(gp).max() > 6.0e6
    R = OC.table(order_in, order_out)
    got = _raw(ctx, R, order_in, order_out, 3, gp, 1)
    assert M.same_bits(got, OC.tensor_apply(R, 3, gp, layout=1))
    assert M.same_bits(ctx.gll_tensor_apply(order_in, order_out, 3, gp, layout=1).numpy(), got)


@pytest.mark.parametrize("order_in,order_out", [(4, 2), (4, 1)])
def test_transpose_through_the_transposed_table(ctx, order_in, order_out):
    Rt = OC.transposed_table(order_in, order_out)
    for dim in (2, 3):
        _check(ctx, order_in, order_out, dim, 13, 2, 0, 77 + dim, R=Rt)
    rng = np.random.default_rng(5)
    v = T.wide(rng, (2, 13, 125))
    ref = OC.tensor_apply(Rt, 3, v)
    assert M.same_bits(ctx.gll_tensor_apply(order_in, order_out, 3, v, transpose=True).numpy(), ref)
    assert M.same_bits(api.gll_order_apply(v, order_in, order_out, 3, transpose=True, context=ctx), ref)
    assert M.same_bits(api.gll_order_apply(v[0], order_in, order_out, 3, transpose=True, context=ctx), ref[0])
    # <I u, v> = <u, I^T v> on the device, to the bound of the statement
    u = rng.normal(size=(1, 7, (order_out + 1) ** 3))
    w = rng.normal(size=(1, 7, 125))
    Iu = api.gll_order_apply(u, order_out, order_in, 3, context=ctx)
    Itw = api.gll_order_apply(w, order_in, order_out, 3, transpose=True, context=ctx)
    diff = abs(float(np.sum(Iu * w)) - float(np.sum(u * Itw)))
    print(f"{order_out}->{order_in}: |<Iu,w> - <u,I^T w>| = {diff:.2e}")
    assert diff <= 10.0 * OC.ADJOINT_OBSERVED[(order_out, order_in)]


# ---------------------------------------------------------------------------------------------- the Python layers
@pytest.mark.parametrize("order,new_order", OC.UP)
def test_resample_up_then_down_returns_the_mesh(ctx, order, new_order):
    gp = synth.gll_mesh(4, order, seed=3)
    rng = np.random.default_rng(order)
    fields = {"a": T.wide(rng, gp.shape[:2]), "b": rng.normal(size=gp.shape[:2])}
    mesh = GllMesh(gp, order, fields)
    before = (gp.copy(), {k: v.copy() for k, v in fields.items()})
    up = api.resample_gll_order(mesh, new_order, context=ctx)
    assert up.shape_order == new_order and up.gll_points.shape == (len(gp), (new_order + 1) ** 3, 3)
    assert M.same_bits(up.gll_points, OC.tensor_apply(OC.table(order, new_order), 3, gp, layout=1))
    assert M.same_bits(up.element_nodal_fields["a"], OC.tensor_apply(OC.table(order, new_order), 3, fields["a"][None])[0])
    assert np.abs(up.gll_points - synth.gll_mesh(4, new_order, seed=3)).max() <= 10.0 * OC.COORDS_OBSERVED[(order, new_order)]
    down = api.resample_gll_order(up, order, context=ctx)
    assert down.shape_order == order and np.array_equal(down.gll_points, gp)
    assert sorted(down.element_nodal_fields) == ["a", "b"]
    assert all(np.array_equal(down.element_nodal_fields[k], fields[k]) for k in fields)
    only_b = api.resample_gll_order(mesh, new_order, params=["b"], context=ctx)
    assert list(only_b.element_nodal_fields) == ["b"]
    assert M.same_bits(only_b.element_nodal_fields["b"], up.element_nodal_fields["b"])
    # the input is untouched
    assert np.array_equal(mesh.gll_points, before[0]) and mesh.shape_order == order
    assert all(np.array_equal(mesh.element_nodal_fields[k], before[1][k]) for k in fields)


@pytest.mark.parametrize("order_f,order_c", [(4, 2), (4, 1), (2, 1)])
def test_restriction_keeps_the_integral(ctx, order_f, order_c):
    """The mesh, the seed and the bound of tests/test_order.py::test_restriction_statement_keeps_the_integral."""
    gp = synth.earth_chunk(order_f, nlat=3, nlon=3, ellipticity=3.3e-3, topography=3e-4)["points"]
    Kf = np.random.default_rng(7).normal(size=gp.shape[:2])
    fine = GllMesh(gp, order_f, {"K": Kf, "absK": np.abs(Kf)})
    coarse = api.restrict_gll_kernel(fine, order_c, params=["K"], context=ctx)
    assert coarse.shape_order == order_c and list(coarse.element_nodal_fields) == ["K"]
    # bit for bit the statement
    _, wf, Df = api.gll_quadrature(order_f)
    _, wc, Dc = api.gll_quadrature(order_c)
    cpts = OC.tensor_apply(OC.table(order_f, order_c), 3, gp, layout=1)
    ref = OC.tensor_apply(OC.transposed_table(order_f, order_c), 3, Kf[None], scale_in=M.mass(gp, order_f, wf, Df)[0],
                          div_out=M.mass(cpts, order_c, wc, Dc)[0])
    assert M.same_bits(coarse.gll_points, cpts) and M.same_bits(coarse.element_nodal_fields["K"], ref[0])
    ints = api.integrate(fine, ["K", "absK"], context=ctx)
    rel = abs(api.integrate(coarse, ["K"], context=ctx)[0] - ints[0]) / ints[1]
    print(f"{order_f}->{order_c}: |int K_c - int K_f| / int |K_f| = {rel:.2e}")
    assert rel <= 10.0 * OC.RESTRICT_OBSERVED[(order_f, order_c)]


def _model_file(points, names, data):
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=points)
    ds = f.create_dataset("MODEL/data", data=data)
    mio.set_dimension_labels(ds, names)
    return f


def test_change_order_between_two_files(ctx):
    kw = dict(nlat=3, nlon=4, ellipticity=3.3e-3, topography=3e-4)
    p2, p4 = synth.earth_chunk(2, **kw)["points"], synth.earth_chunk(4, **kw)["points"]
    E = len(p2)
    rng = np.random.default_rng(9)
    names = ["VP", "VS", "RHO"]
    d2, d4 = T.wide(rng, (E, 3, 27)), T.wide(rng, (E, 3, 125))
    sentinel = np.full((E, 3, 125), -7.0)
    # up: all parameters, values equal the statement's in the files' own layout
    src, dst = _model_file(p2, names, d2), _model_file(p4, names, sentinel)
    api.gll_change_order(src, dst, context=ctx)
    assert M.same_bits(dst["MODEL/data"][:], OC.tensor_apply(OC.table(2, 4), 3, d2, layout=2))
    assert mio.dimension_labels(dst["MODEL/data"], 1) == names
    assert M.same_bits(src["MODEL/data"][:], d2) and M.same_bits(dst["MODEL/coordinates"][:], p4)
    # down: a subset, in the order asked for
    back = _model_file(p2, names, np.zeros((E, 3, 27)))
    api.gll_change_order(dst, back, parameters=["RHO", "VP"], context=ctx)
    assert mio.dimension_labels(back["MODEL/data"], 1) == ["RHO", "VP"]
    assert np.array_equal(back["MODEL/data"][:], d2[:, [2, 0], :])                   # up then down: the input
    # kernel=True going down is the mass-weighted restriction
    _, w4, D4 = api.gll_quadrature(4)
    _, w2, D2 = api.gll_quadrature(2)
    c2 = OC.tensor_apply(OC.table(4, 2), 3, p4, layout=1)
    ref = OC.tensor_apply(OC.transposed_table(4, 2), 3, d4, 2, M.mass(p4, 4, w4, D4)[0], M.mass(c2, 2, w2, D2)[0])
    kdst = _model_file(p2, names, np.zeros((E, 3, 27)))
    api.gll_change_order(_model_file(p4, names, d4), kdst, kernel=True, context=ctx)
    assert M.same_bits(kdst["MODEL/data"][:], ref)
    # kernel=True going up raises
    with pytest.raises(ValueError, match="goes down"):
        api.gll_change_order(src, _model_file(p4, names, sentinel), kernel=True, context=ctx)
    # two elements swapped in the receiving file: ValueError naming the first of them, nothing written
    swapped = p4.copy()
    swapped[[3, 8]] = swapped[[8, 3]]
    bad = _model_file(swapped, ["OLD"], sentinel[:, :1])
    with pytest.raises(ValueError, match="element 3 "):
        api.gll_change_order(src, bad, context=ctx)
    assert M.same_bits(bad["MODEL/data"][:], sentinel[:, :1]) and mio.dimension_labels(bad["MODEL/data"], 1) == ["OLD"]


# wave-per-element kernel, 4 waves to a block, at most 2048 blocks: one element, a part of a block, more than one block, and
# more elements than the capped grid has waves (8192), at every node count the orders give
@pytest.mark.parametrize("dim,npts,nelem", [(2, 4, 1), (2, 9, 3), (2, 25, 8195), (3, 8, 4), (3, 27, 5), (3, 125, 131),
                                            (3, 22, 7)])
def test_element_deviation_is_its_statement(ctx, dim, npts, nelem):
    rng = np.random.default_rng(100 * npts + dim)
    b = T.wide(rng, (nelem, npts, dim)) + 6.4e6
    a = b + T.wide(rng, (nelem, npts, dim)) * 1e-3
    if nelem > 2:
        a[1, npts - 1, dim - 1] = np.nan                     # a NaN in the last lane's share ...
        b[2, 0, 0] = np.nan                                  # ... and one in the node the bounding box starts from
    ref_dev, ref_edge = OC.element_deviation(a, b)
    dev, edge = (x.numpy() for x in ctx.element_deviation(a, b))
    assert np.isnan(ref_dev).sum() == (2 if nelem > 2 else 0) and not np.isnan(ref_edge).any()
    assert np.array_equal(np.isnan(dev), np.isnan(ref_dev))
    ok = ~np.isnan(ref_dev)
    assert M.same_bits(dev[ok], ref_dev[ok]) and M.same_bits(edge, ref_edge)


def test_element_deviation_error_paths_write_nothing(ctx):
    fn, h = helpers.load_lib().mm_element_deviation, ctx.handle
    sentinel = np.full((8,), -7.0)
    out, a, b = ctx.to_device(sentinel), ctx.to_device(np.ones((4, 27, 3))), ctx.to_device(np.ones((4, 27, 3)))
    cases = {
        "dim 4": fn(h, 4, 27, a.ptr, b.ptr, 4, out.ptr, out.ptr + 32),
        "npts 0": fn(h, 3, 0, a.ptr, b.ptr, 4, out.ptr, out.ptr + 32),
        "nelem": fn(h, 3, 27, a.ptr, b.ptr, -1, out.ptr, out.ptr + 32),
        "null a": fn(h, 3, 27, None, b.ptr, 4, out.ptr, out.ptr + 32),
        "null edge": fn(h, 3, 27, a.ptr, b.ptr, 4, out.ptr, None),
        "deviation in a": fn(h, 3, 27, a.ptr, b.ptr, 4, a.ptr + 8 * 100, out.ptr),
        "edge in b": fn(h, 3, 27, a.ptr, b.ptr, 4, out.ptr, b.ptr),
        "edge in deviation": fn(h, 3, 27, a.ptr, b.ptr, 4, out.ptr, out.ptr + 24),
    }
    for what, rc in cases.items():
        assert rc == MM_ERR_ARG, what
    assert fn(h, 3, 27, None, None, 0, None, None) == 0                             # nothing to do is not an error
    assert M.same_bits(out.numpy(), sentinel)
    with pytest.raises(ValueError):
        ctx.element_deviation(np.ones((4, 27, 3)), np.ones((4, 8, 3)))


def test_error_paths_write_nothing(ctx):
    fn, h = helpers.load_lib().mm_gll_tensor_apply, ctx.handle
    sentinel = np.full((1, 4, 125), -7.0)
    out, v = ctx.to_device(sentinel), ctx.to_device(np.ones((1, 4, 27)))
    R = ctx.to_device(OC.table(2, 4))
    cases = {
        "equal orders": fn(h, 3, 2, 2, R.ptr, 0, v.ptr, out.ptr, 4, 1, None, None),
        "order 3": fn(h, 3, 3, 4, R.ptr, 0, v.ptr, out.ptr, 4, 1, None, None),
        "layout": fn(h, 3, 2, 4, R.ptr, 3, v.ptr, out.ptr, 4, 1, None, None),
        "dim 4": fn(h, 4, 2, 4, R.ptr, 0, v.ptr, out.ptr, 4, 1, None, None),
        "null table": fn(h, 3, 2, 4, None, 0, v.ptr, out.ptr, 4, 1, None, None),
        "null in": fn(h, 3, 2, 4, R.ptr, 0, None, out.ptr, 4, 1, None, None),
        "null out": fn(h, 3, 2, 4, R.ptr, 0, v.ptr, None, 4, 1, None, None),
        "out is in": fn(h, 3, 2, 4, R.ptr, 0, out.ptr, out.ptr, 4, 1, None, None),
        "out inside in": fn(h, 3, 4, 2, R.ptr, 0, out.ptr, out.ptr + 8 * 100, 4, 1, None, None),
        "out is div": fn(h, 3, 2, 4, R.ptr, 0, v.ptr, out.ptr, 4, 1, None, out.ptr),
        "nelem": fn(h, 3, 2, 4, R.ptr, 0, v.ptr, out.ptr, -1, 1, None, None),
    }
    for what, rc in cases.items():
        assert rc == MM_ERR_ARG, what
    assert fn(h, 3, 2, 4, R.ptr, 0, v.ptr, out.ptr, 0, 1, None, None) == 0           # nothing to do is not an error
    assert fn(h, 3, 2, 4, R.ptr, 0, None, None, 4, 0, None, None) == 0
    assert M.same_bits(out.numpy(), sentinel)
    with pytest.raises(ValueError):
        ctx.gll_tensor_apply(2, 2, 3, np.ones((1, 4, 27)))
    with pytest.raises(ValueError):
        ctx.gll_tensor_apply(2, 4, 3, np.ones((1, 4, 125)))
    with pytest.raises(ValueError):
        ctx.gll_tensor_apply(2, 4, 3, np.ones((1, 4, 27)), scale_in=np.ones((4, 125)))
