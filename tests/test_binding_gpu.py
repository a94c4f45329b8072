"""What the Python layer over the C entry points does around its calls, on the smallest shapes at which ``[E, P]`` and
``[C, E, P]`` differ: the rule every ``out`` argument is held to, the promotion of a single component, views that outlive
the arrays they were cut from, handles freed twice and used after, and the library's own text on a caller's mistake.

Shapes: an order-1 3-D mesh of 2 elements (P = 8), an order-2 2-D mesh of 2 elements (P = 9), 5 target points, 2
components, a 2 x 2 x 2 grid."""
import gc
import re
import types

import numpy as np
import pytest

from multimesh_amd import api, synth
from multimesh_amd.device import Context

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def d():
    d = types.SimpleNamespace()
    rng = np.random.default_rng(5)
    chunk = synth.earth_chunk(order=1, nlat=1, nlon=2, lat=(-1.0, 1.0), lon=(-2.0, 2.0), radii=(6_171_000.0, synth.R_EARTH),
                              nrad=(1,))     # (2 degrees a side: the flat faces stay within 1 km of the sphere)
    d.g3, d.z3 = chunk["points"], chunk["z_node_1D"]                      # [2, 8, 3], [2, 8]
    d.g2 = synth.gll_mesh(3, 2, jitter=0.0, dim=2)[:2]                    # [2, 9, 2]: x in [0, 0.5], y in [0, 1]
    d.f3, d.f2 = rng.standard_normal((2, 2, 8)), rng.standard_normal((2, 2, 9))
    lat, lon, r = rng.uniform(-0.8, 0.8, 5), rng.uniform(-1.8, 1.8, 5), rng.uniform(6.2e6, 6.35e6, 5)
    colat, phi = np.deg2rad(90.0 - lat), np.deg2rad(lon)
    d.p3 = np.ascontiguousarray(np.stack([r * np.sin(colat) * np.cos(phi), r * np.sin(colat) * np.sin(phi),
                                          r * np.cos(colat)], axis=1))    # 5 points inside the chunk
    d.p2 = np.ascontiguousarray(np.stack([rng.uniform(0.05, 0.45, 5), rng.uniform(0.05, 0.95, 5)], axis=1))
    d.nodes, conn = synth.hex_mesh(3, jitter=0.0)                         # hex8: 27 nodes, the 2 elements over z
    d.conn = np.ascontiguousarray(conn[:2])
    d.ph = np.ascontiguousarray(np.stack([rng.uniform(0.05, 0.45, 5), rng.uniform(0.05, 0.45, 5),
                                          rng.uniform(0.05, 0.95, 5)], axis=1))
    d.fn = rng.standard_normal((2, 27))
    d.ids = rng.integers(0, 27, (5, 8))
    d.w = rng.uniform(0.0, 1.0, (5, 8))
    d.lat_t, d.lon_t, d.rad = api.column_tables([-0.5, 0.5], [-1.0, 1.0], [50e3, 150e3])
    d.grid = rng.standard_normal((2, 2, 2, 2))                            # [C, D, LA, LO]
    d.axes = (np.array([0.0, 300e3]), np.array([-7.0, 7.0]), np.array([-7.0, 7.0]))
    d.table_r, d.table_v = np.array([6.0e6, 6.4e6]), np.array([[1.0, 2.0], [3.0, 5.0]])
    return d


# --------------------------------------------------------------------------------------------------------- out buffers
def _check_out(ctx, call, shape, message, size_only=False):
    """``call(out)`` returns the method's array.  The right shape is returned itself, another size is refused with
    ``message``, and the same size in another shape is accepted where only the size is held to and refused elsewhere."""
    size = int(np.prod(shape))
    good = ctx.empty(shape, np.float64)
    assert call(good) is good
    with pytest.raises(ValueError, match=re.escape(message)):
        call(ctx.empty(tuple(shape) + (2,), np.float64))
    flat = ctx.empty((size,), np.float64)
    if size_only:
        assert call(flat) is flat
    else:
        with pytest.raises(ValueError, match=re.escape(message)):
            call(flat)
    return good


def test_out_of_the_transposed_operator(ctx, d):
    op = ctx.transpose_nodes(d.ids, d.w, 27)
    values = np.arange(10.0).reshape(5, 2)
    got = _check_out(ctx, lambda out: op.apply(values, out=out), (2, 27), "out must be (2, 27)")
    assert np.array_equal(got.numpy(), op.apply(values).numpy())
    op.free()


def test_out_of_the_stiffness_operator(ctx, d):
    dif = ctx.diffusion(1, d.g3)
    u = ctx.to_device(d.f3)
    message = "out must be another array of the shape of u"
    got = _check_out(ctx, lambda out: dif.apply(u, out=out), (2, 2, 8), message)
    assert np.array_equal(got.numpy(), dif.apply(u).numpy())
    with pytest.raises(ValueError, match=message):
        dif.apply(u, out=u)
    dif.free()


def test_out_of_divide_rows(ctx, d):
    den = np.abs(d.f3[0]) + 1.0
    got = _check_out(ctx, lambda out: ctx.divide_rows(d.f3, den, out=out), (2, 2, 8), "out must have the shape of num")
    assert np.array_equal(got.numpy(), d.f3 / den)


def test_out_of_radial_model_apply_is_held_to_its_size(ctx, d):
    got = _check_out(ctx, lambda out: ctx.radial_model_apply(d.g3, d.table_r, d.table_v, out=out), (2, 2, 8),
                     "out must hold one value per component and node", size_only=True)
    assert np.array_equal(got.numpy(), ctx.radial_model_apply(d.g3, d.table_r, d.table_v).numpy())


def test_out_of_gll_tensor_apply(ctx, d):
    got = _check_out(ctx, lambda out: ctx.gll_tensor_apply(1, 2, 3, d.f3, out=out), (2, 2, 27), "out must be (2, 2, 27)")
    assert np.array_equal(got.numpy(), ctx.gll_tensor_apply(1, 2, 3, d.f3).numpy())


def test_out_of_interpolate_gll(ctx, d):
    got = _check_out(ctx, lambda out: ctx.interpolate_gll(1, d.g3, d.p3, d.f3, 2, out=out)[0], (5, 2), "out must be [N, C]")
    values, missing = ctx.interpolate_gll(1, d.g3, d.p3, d.f3, 2)
    assert missing == 0 and np.array_equal(got.numpy(), values.numpy())


def test_out_of_sample_columns_gll(ctx, d):
    def call(out):
        return ctx.sample_columns_gll(1, d.g3, d.f3, d.lat_t, d.lon_t, d.rad, nelem_to_search=2, out=out)[0]

    got = _check_out(ctx, call, (2, 2, 4), "out must be [C, D, H]")
    values, missing = ctx.sample_columns_gll(1, d.g3, d.f3, d.lat_t, d.lon_t, d.rad, nelem_to_search=2)
    assert missing == 0 and np.array_equal(got.numpy(), values.numpy())


def test_out_of_sample_grid_keeps_its_own_rule(ctx, d):
    """[C, N], or [C, ...] over the leading shape of the points: the first axis and the size are held to."""
    def call(out, **kw):
        return ctx.sample_grid(d.p3, d.grid, *d.axes, out=out, **kw)[0]

    message = re.escape("out must be [C, N] (or [C, ...] over the leading shape of points)")
    good, lead = ctx.empty((2, 5), np.float64), ctx.empty((2, 5, 1), np.float64)
    assert call(good) is good and call(lead) is lead
    for shape in ((2, 5, 2), (10,), (5, 2), (1, 10)):
        with pytest.raises(ValueError, match=message):
            call(ctx.empty(shape, np.float64))
    with pytest.raises(ValueError, match="pass out"):
        call(None, outside="keep")
    values, outside = ctx.sample_grid(d.p3, d.grid, *d.axes)
    assert outside == 0 and np.array_equal(good.numpy(), values.numpy())
    assert np.array_equal(lead.numpy().reshape(2, 5), values.numpy())


def test_out_of_the_sphere_maps_is_held_to_its_size(ctx, d):
    message = "out must have the shape of points"
    got = _check_out(ctx, lambda out: ctx.map_to_sphere(d.g3, d.z3, out=out), (2, 8, 3), message, size_only=True)
    assert np.array_equal(got.numpy(), ctx.map_to_sphere(d.g3, d.z3).numpy())
    factor = d.f3[0]
    got = _check_out(ctx, lambda out: ctx.scale_points(d.g3, factor, out=out), (2, 8, 3), message, size_only=True)
    assert np.array_equal(got.numpy(), factor[..., None] * d.g3)


def test_out_of_the_hex8_paths_is_returned_itself(ctx, d):
    source = ctx.source(d.nodes, d.conn)
    ref, nfailed = ctx.interpolate_hex8(d.nodes, d.conn, d.ph, d.fn, 2)
    assert nfailed == 0
    for call in (lambda out: ctx.interpolate_hex8(d.nodes, d.conn, d.ph, d.fn, 2, out=out),
                 lambda out: source.interpolate(d.ph, d.fn, 2, out=out)):
        out = ctx.empty((5, 2), np.float64)
        got, nf = call(out)
        assert got is out and nf == 0 and np.array_equal(out.numpy(), ref.numpy())
    source.free()


# ----------------------------------------------------------------------------------------------------------- promotion
def _same(single, promoted):
    """The call with one component given bare against the call with it as [1, ...]: the same shape and bits."""
    a, b = single.numpy(), promoted.numpy()
    assert a.shape == b.shape and a.size and np.array_equal(a, b, equal_nan=True)


def test_a_single_component_is_the_first_row_hex8(ctx, d):
    f = d.fn[1]                                                                      # [M] against [1, M]
    _same(ctx.interpolate_hex8(d.nodes, d.conn, d.ph, f, 2)[0], ctx.interpolate_hex8(d.nodes, d.conn, d.ph, f[None], 2)[0])
    source = ctx.source(d.nodes, d.conn)
    _same(source.interpolate(d.ph, f, 2)[0], source.interpolate(d.ph, f[None], 2)[0])
    source.free()
    for point_major in (True, False):
        _same(ctx.gather(f, d.ids, d.w, point_major), ctx.gather(f[None], d.ids, d.w, point_major))
    op = ctx.transpose_nodes(d.ids, d.w, 27)
    v = np.arange(5.0) - 2.0                                                         # [N] against [N, 1] and [1, N]
    _same(op.apply(v), op.apply(v[:, None]))
    _same(op.apply(v, point_major=False), op.apply(v[None], point_major=False))
    _same(op.apply(v), op.apply(v, point_major=False))
    op.free()


@pytest.mark.parametrize("dim", [3, 2])
def test_a_single_component_is_the_first_row_gll(ctx, d, dim):
    order, gp, f, pts = (1, d.g3, d.f3[1], d.p3) if dim == 3 else (2, d.g2, d.f2[1], d.p2)   # [E, P] against [1, E, P]
    nn = np.tile(np.arange(2), (5, 1))
    elem, coeffs, missing = ctx.locate_gll(order, nn, gp, pts)
    assert missing == 0
    for point_major in (True, False):
        _same(ctx.gather_elem(f, elem, coeffs, point_major), ctx.gather_elem(f[None], elem, coeffs, point_major))
    _same(ctx.interpolate_gll(order, gp, pts, f, 2)[0], ctx.interpolate_gll(order, gp, pts, f[None], 2)[0])
    _same(ctx.gll_gradient(order, gp, f), ctx.gll_gradient(order, gp, f[None]))
    other = 2 if order == 1 else 4
    _same(ctx.gll_tensor_apply(order, other, dim, f), ctx.gll_tensor_apply(order, other, dim, f[None]))
    dif = ctx.diffusion(order, gp)
    _same(dif.apply(f), dif.apply(f[None]))
    _same(dif.smooth(f, steps=1), dif.smooth(f[None], steps=1))
    assert np.array_equal(dif.roughness(f), dif.roughness(f[None]))
    dif.free()


def test_a_single_component_is_the_first_row_earth(ctx, d):
    f = d.f3[1]
    _same(ctx.sample_columns_gll(1, d.g3, f, d.lat_t, d.lon_t, d.rad, nelem_to_search=2)[0],
          ctx.sample_columns_gll(1, d.g3, f[None], d.lat_t, d.lon_t, d.rad, nelem_to_search=2)[0])
    g = d.grid[1]                                                                    # [D, LA, LO] against [1, D, LA, LO]
    _same(ctx.sample_grid(d.p3, g, *d.axes)[0], ctx.sample_grid(d.p3, g[None], *d.axes)[0])
    v = d.table_v[1]                                                                 # [m] against [1, m]
    _same(ctx.radial_model_apply(d.g3, d.table_r, v), ctx.radial_model_apply(d.g3, d.table_r, v[None]))
    mass, n_bad = ctx.gll_mass(1, d.g3)
    assert n_bad == 0
    bins, _ = ctx.radial_bins(d.g3, np.array([6.0e6, 6.3e6, 6.4e6]))
    assert np.array_equal(ctx.weighted_sum(mass, f), ctx.weighted_sum(mass, f[None]))
    assert np.array_equal(ctx.binned_weighted_sum(mass, bins, 2, f), ctx.binned_weighted_sum(mass, bins, 2, f[None]))
    for call in (ctx.weighted_sum, lambda m, x: ctx.binned_weighted_sum(m, bins, 2, x)):
        with pytest.raises(ValueError, match=re.escape("fields must be [C, ...] over the shape of mass, or the shape of mass")):
            call(mass, d.f3.reshape(2, 16))


# ------------------------------------------------------------------------------------------------------- view lifetime
def test_unique_points_outlive_the_buffers_they_are_cut_from(ctx, d):
    flat = np.ascontiguousarray(d.g3.reshape(-1, 3))
    ref, ref_inv = np.unique(flat, axis=0, return_inverse=True)
    assert len(ref) == 12 < len(flat)
    pts = ctx.to_device(flat)
    unique_out, inverse_out = ctx.empty((16, 3), np.float64), ctx.empty((16,), np.int64)
    held = ctx.unique_points(pts, unique_out, inverse_out)
    own = ctx.unique_points(pts)
    assert held[0].ptr == unique_out.ptr and held[1].ptr == inverse_out.ptr
    del unique_out, inverse_out, pts
    gc.collect()
    fill = [ctx.to_device(np.full((16, 3), -1.0)) for _ in range(4)]                 # (what a released buffer would become)
    for uniq, inv in (held, own):
        assert uniq.shape == (12, 3) and inv.shape == (16,)
        assert np.array_equal(uniq.numpy(), ref) and np.array_equal(inv.numpy(), ref_inv.reshape(-1))
    del fill


def test_reshape_views_outlive_their_parent(ctx):
    values = np.arange(24.0).reshape(2, 3, 4)
    parent = ctx.to_device(values)
    view = parent.reshape(4, 6)
    nested = view.reshape(24).reshape(1, 24)
    with pytest.raises(ValueError):
        parent.reshape(5, 5)
    del parent
    gc.collect()
    fill = [ctx.to_device(np.full(24, -1.0)) for _ in range(4)]
    assert np.array_equal(view.numpy(), values.reshape(4, 6))
    del view
    gc.collect()
    assert np.array_equal(nested.numpy(), values.reshape(1, 24))
    del fill


# -------------------------------------------------------------------------------------------------------------- handles
def test_handles_may_be_freed_twice(ctx, d):
    index = ctx.knn_build(d.p3)
    assert index.query(d.p3, 1).numpy().reshape(-1).tolist() == [0, 1, 2, 3, 4]
    source = ctx.source(d.nodes, d.conn)
    op = ctx.transpose_elem(np.arange(5) % 2, d.w, 2)
    for handle in (index, source, op):
        assert handle.handle
        handle.free()
        assert handle.handle is None
        handle.free()
        assert handle.handle is None
    assert op._keepalive is None
    with pytest.raises(ValueError, match="the operator has been freed"):
        op.apply(np.zeros(5))

    dif = ctx.diffusion(1, d.g3)
    dif.smooth(d.f3, steps=1)                                                        # (builds the assembly it then frees)
    inner = dif._asm["op"]
    dif.free()
    assert dif._asm is None and dif.gp is None and inner.handle is None
    dif.free()
    for call in (dif.apply, dif.smooth):
        with pytest.raises(ValueError, match="the operator has been freed"):
            call(d.f3)

    array = ctx.to_device(np.arange(4.0))
    assert array.ptr
    array.free()
    assert array.ptr == 0
    array.free()
    assert array.ptr == 0

    other = Context(0)
    assert other.handle
    other.close()
    assert other.handle is None
    other.close()
    assert other.handle is None


def test_handles_are_released_at_the_end_of_a_with_block(ctx):
    # a 2 x 2 x 2-element hex8 mesh: the transposed operator over its connectivity, the stiffness operator of its elements
    nodes, conn = synth.hex_mesh(3, jitter=0.0)
    weights = np.full(conn.shape, 0.125)
    gll = np.ascontiguousarray(nodes[conn[:, [0, 1, 3, 2, 4, 5, 7, 6]]])             # exodus -> tensor order, order 1
    with ctx.transpose_nodes(conn, weights, len(nodes)) as op:
        assert op.handle and op.apply(np.ones(len(conn))).numpy().sum() == len(conn)
    assert op.handle is None and op._keepalive is None
    op.free()                                                                        # (a second release is harmless)
    assert op.handle is None
    with pytest.raises(ValueError, match="inside the block"):
        with ctx.transpose_nodes(conn, weights, len(nodes)) as op:
            raise ValueError("inside the block")
    assert op.handle is None

    with ctx.diffusion(1, gll) as dif:
        assert np.abs(dif.smooth(np.ones(gll.shape[:2]), steps=0).numpy() - 1.0).max() < 1e-14     # (the node average of 1)
        inner = dif._asm["op"]
        assert inner.handle
    assert dif._asm is None and dif.gp is None and inner.handle is None
    dif.free()
    assert dif.gp is None
    with pytest.raises(ValueError, match="inside the block"):
        with ctx.diffusion(1, gll) as dif:
            dif.smooth(np.ones(gll.shape[:2]), steps=0)
            inner = dif._asm["op"]
            raise ValueError("inside the block")
    assert dif._asm is None and dif.gp is None and inner.handle is None


# -------------------------------------------------------------------------------------------------------- caller errors
def test_a_callers_mistake_raises_value_error_with_the_librarys_text(ctx, d):
    with pytest.raises(ValueError, match="mm_radial_bins: the edges are not finite and strictly ascending"):
        ctx.radial_bins(d.g3, np.array([6.4e6, 6.3e6, 6.0e6]))                       # descending edges
    with pytest.raises(ValueError, match="a layer of the table has a single row"):
        ctx.radial_model_apply(d.g3, np.array([1.0, 2.0, 2.0]), np.zeros((1, 3)))    # a table that is not layers
    with pytest.raises(ValueError, match=re.escape("mm_first_occurrence: 1 connectivity entries outside [0, 3)")):
        ctx.first_occurrence(np.array([[0, 1, 5]]), 3)
