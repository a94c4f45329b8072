"""mm_grid_operator, the GridOperator over it and regular_grid_adjoint on the GPU, against the NumPy statement of
tests/grid_adjoint_cases.py.

As for mm_sample_grid, the device's acos and atan2 are the one part compared by a bound (1e-11 degrees against NumPy's);
ids, weights and counts are compared exactly, by evaluating the statement on the coordinates the device returned, and the
transposes bit for bit with np.add.at.  The bounds that are not bit equality are derived where they are used; none is
measured."""
import types

import numpy as np
import pytest

import grid_adjoint_cases as GA
import grid_import_cases as G
from multimesh_amd import api, synth
from multimesh_amd.device import Context
from test_caller_stream_gpu import SPIN_FACTOR, SPIN_FLOOR_MS, Case, _bits, _run_on_side, _run_reference, _same_as, _spin_ms
from test_caller_views_gpu import _run_on_views

pytestmark = pytest.mark.gpu

ANGLE_TOL = 1e-11          # degrees, as tests/test_grid_import_gpu.py
EPS = GA.EPS


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()      # before this module's context opens the device: torch then finds it whichever test runs first
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    with Context(0) as c:
        yield c


def _lld(ctx, pts, depth, lat, lon, periodic=False):
    """The coordinates mm_sample_grid computes for the points (ncomp == 0)"""
    empty = np.zeros((0, len(depth), len(lat), len(lon)))
    return ctx.sample_grid(pts, empty, depth, lat, lon, lon_periodic=periodic, want_latlondepth=True)[2].numpy()


def _check_operator(ctx, pts, depth, lat, lon, clamp, periodic=False):
    """ids, w and the count == the statement on the device's own coordinates -> (ids, w, noutside, inside, lld)"""
    n = len(pts)
    ids, w, nout, lld = ctx.grid_operator(pts, depth, lat, lon, clamp=clamp, lon_periodic=periodic, latlondepth=True)
    ids, w, lld = ids.numpy(), w.numpy(), lld.numpy()
    assert ids.shape == (n, 8) and w.shape == (n, 8) and lld.shape == (n, 3) and ids.dtype == np.int64
    assert G.same_bits(lld, _lld(ctx, pts, depth, lat, lon, periodic))          # the coordinates of mm_sample_grid
    ref = G.latlondepth(pts)
    if periodic:
        ref[:, 1] = G.wrap(ref[:, 1], lon[0])
    ok = ~np.isnan(ref).any(axis=1)
    assert np.array_equal(np.isnan(lld).any(axis=1), ~ok) and G.same_bits(lld[:, 2], ref[:, 2])
    if ok.any():
        assert GA.angle_difference(lld[ok, :2], ref[ok, :2]).max() <= ANGLE_TOL
    want_ids, want_w, want_out, inside = GA.operator(depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1], clamp, periodic)
    assert nout == want_out == int((~inside).sum()), (nout, want_out)
    assert np.array_equal(ids, want_ids), int((ids != want_ids).any(axis=1).sum())
    assert G.same_bits(w, want_w)
    if clamp:
        assert nout == 0
    else:
        assert not ids[~inside].any() and not w[~inside].any() and not np.signbit(w[~inside]).any()
    return ids, w, nout, inside, lld


def _global_axes(start, closed):
    """(depth, lat, lon) of a 2.5-degree global grid whose longitudes start at ``start``, with or without the column start + 360"""
    lon = start + 2.5 * np.arange(145 if closed else 144)
    return np.array([-100_000.0, 500_000.0, 1_500_000.0, 3_000_000.0]), np.linspace(-90.0, 90.0, 73), lon


# ---------------------------------------------------------------------------------------------- 1. the operator, bit for bit
@pytest.mark.parametrize("clamp", [False, True])
def test_operator_bit_for_bit_on_the_shared_axes(ctx, clamp):
    pts = GA.mixed_points()
    ids, w, nout, inside, lld = _check_operator(ctx, pts, G.DEPTH, G.LAT, G.LON, clamp)
    assert 1900 <= len(pts) <= 2100 and np.isnan(lld[-1]).any()
    if clamp:
        assert np.isnan(w[-1]).any()                          # a NaN coordinate: NaN weights on the ids the search gives
        assert 0 <= ids.min() and ids.max() < 7 * 9 * 11
    else:
        assert 0.1 * len(pts) < nout < 0.45 * len(pts) and not inside[-1]
        assert np.abs(w[inside].sum(axis=1) - 1.0).max() <= 4 * EPS
    for n in (0, 1, 255, 256, 257):
        _check_operator(ctx, pts[:n].reshape(n, 3), G.DEPTH, G.LAT, G.LON, clamp)
    ids0, w0, n0 = ctx.grid_operator(np.zeros((0, 3)), G.DEPTH, G.LAT, G.LON, clamp=clamp)
    assert n0 == 0 and ids0.shape == (0, 8) and w0.shape == (0, 8)


@pytest.mark.parametrize("clamp", [False, True])
def test_operator_past_one_pass_of_the_grid_stride_loop(ctx, clamp):
    n = 600_001                                               # 2048 workgroups x 256 lanes = 524 288 points per pass
    pts = GA.random_points(n, G.DEPTH, G.LAT, G.LON, 0.075, seed=77)
    _, _, nout, _, _ = _check_operator(ctx, pts, G.DEPTH, G.LAT, G.LON, clamp)
    assert clamp or 0.2 * n < nout < 0.5 * n


@pytest.mark.parametrize("clamp", [False, True])
def test_operator_on_long_and_degenerate_axes(ctx, clamp):
    pts = GA.mixed_points()
    # 3 + 5 + 2100 nodes do not fit the LDS copy: the axes are bisected in global memory
    depth, lat, lon = G.DEPTH[[0, 3, 6]], G.LAT[[0, 2, 4, 6, 8]], np.linspace(-5.5, 6.5, 2100)
    ids, _, _, inside, _ = _check_operator(ctx, GA.mixed_points(depth, lat, lon, nface=150), depth, lat, lon, clamp)
    assert ids.max() > 2 * 5 * 2100 and inside.sum() > 500
    # an axis of length 1: i = i1 = 0 and t = 0, two corners share an id
    ids, w, _, inside, _ = _check_operator(ctx, pts, G.DEPTH[3:4], G.LAT, G.LON, clamp)
    finite = inside & ~np.isnan(w).any(axis=1)                # (clamp: the NaN row holds NaN weights, 0 * NaN)
    assert np.array_equal(ids[:, :4], ids[:, 4:]) and not w[finite][:, 4:].any() and ids.max() < 9 * 11
    ids, w, _, inside, _ = _check_operator(ctx, pts, G.DEPTH, G.LAT, G.LON[5:6], clamp)
    finite = inside & ~np.isnan(w).any(axis=1)
    assert np.array_equal(ids[:, 0::2], ids[:, 1::2]) and not w[finite][:, 1::2].any() and ids.max() < 7 * 9
    _check_operator(ctx, pts[:300], G.DEPTH[:1], G.LAT[:1], G.LON[:1], clamp)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("start", [0.0, -180.0])
def test_operator_on_periodic_axes(ctx, start, clamp):
    sphere = G.sphere_points(1500, seed=9, rmin=3.2e6)
    for closed in (False, True):                              # the closing column appended by the host, or in the data
        depth, lat, lon = _global_axes(start, closed)
        grid = api.RegularGrid(depth, lat, lon, {"v": G.periodic_field(lat, lon, depth)})
        d, la, lo, data, _, periodic = api.prepare_regular_grid(grid)
        assert periodic and len(lo) == 145 and lo[-1] == start + 360.0
        seam = GA.xyz(np.linspace(-80.0, 80.0, 9), start, 200_000.0)              # on the seam itself
        pts = np.concatenate([sphere, seam, GA.xyz(*np.meshgrid(la[::9], lo[::12]), 100_000.0)])
        ids, w, nout, inside, lld = _check_operator(ctx, pts, d, la, lo, clamp, periodic=True)
        assert lld[:, 1].min() >= lo[0] and lld[:, 1].max() < lo[0] + 360.0
        assert clamp or 0 < nout < 0.1 * len(pts)             # (only radii below the deepest node)
        assert (ids[inside] % 145 == 144).any() and (ids[inside] % 145 == 0).any()


# ---------------------------------------------------------------------------------------------- 2. gather through it
@pytest.mark.parametrize("clamp", [False, True])
def test_gather_through_the_operator_agrees_with_sample_grid(ctx, clamp):
    """Both evaluate the same trilinear form of the same eight corners: the nested lerps with at most ten roundings, the
    8-term sum with at most seven (weights, product, NumPy's sum), each relative to terms of at most max|corner|: the two
    differ by at most 32 eps max|corner|, margin included."""
    pts = GA.mixed_points()[:-1]                              # (finite data: without the NaN row)
    grid = G.grid_values(3)
    ids, w, nout = ctx.grid_operator(pts, G.DEPTH, G.LAT, G.LON, clamp=clamp)
    got = ctx.gather(grid.reshape(3, -1), ids, w, point_major=False).numpy()
    want, miss = ctx.sample_grid(pts, grid, G.DEPTH, G.LAT, G.LON, outside="clamp" if clamp else "fill", fill_value=0.0)
    want = want.numpy()
    assert miss == nout
    corner = np.abs(grid.reshape(3, -1)[:, ids.numpy()]).max(axis=2)              # [C, N]
    worst = (np.abs(got - want) / (EPS * corner)).max()
    print(f"max |gather - sample_grid| = {worst:.2f} eps max|corner|")
    assert G.same_bits(got, GA.gather(grid.reshape(3, -1), ids.numpy(), w.numpy()))
    assert (np.abs(got - want) <= 32 * EPS * corner).all()
    # GridOperator.apply: the same values, fill_value in the rows outside
    op = api.grid_import_operator(api.RegularGrid(G.DEPTH, G.LAT, G.LON, {}), pts, outside="clamp" if clamp else "fill", context=ctx)
    applied = op.apply(grid, fill_value=-3.0)
    outside = ~w.numpy().any(axis=1)
    assert op.noutside == nout and applied.shape == (3, len(pts))
    assert G.same_bits(applied[:, ~outside], got[:, ~outside]) and (applied[:, outside] == -3.0).all()
    named = api.RegularGrid(G.DEPTH, G.LAT, G.LON, {"a": grid[0], "b": grid[1]})
    assert G.same_bits(op.apply(named, parameters=["b"], fill_value=-3.0)[0], applied[1])
    op.free()


# ---------------------------------------------------------------------------------------------- 3. the transpose
def _wide(rng, shape):
    return rng.normal(size=shape) * 10.0 ** rng.uniform(-6.0, 6.0, size=shape)


@pytest.mark.parametrize("ncomp", [1, 3])
def test_transpose_is_add_at_bit_for_bit(ctx, ncomp):
    rng = np.random.default_rng(40 + ncomp)
    # the shared axes as they are, and a global grid that is flipped in latitude and gets its closing column appended
    depth, lat, lon = _global_axes(0.0, False)
    cases = [(api.RegularGrid(G.DEPTH, G.LAT, G.LON, {}), GA.mixed_points()[:-1], (False, False, False), False),
             (api.RegularGrid(depth[::-1], lat[::-1], lon, {}), G.sphere_points(2000, seed=12), (True, True, False), True)]
    for grid, pts, flipped, appended in cases:
        d, la, lo, _, _, periodic = api.prepare_regular_grid(grid, [])
        op = api.grid_import_operator(grid, pts, context=ctx)
        assert op.flipped == flipped and op.appended == appended and op.periodic == periodic == appended
        assert op.prepared_shape == (len(d), len(la), len(lo)) and op.grid_shape == tuple(len(grid.coords[k]) for k in api.DIMS)
        lld = _lld(ctx, pts, d, la, lo, periodic)
        ids, w, nout, _ = GA.operator(d, la, lo, lld[:, 2], lld[:, 0], lld[:, 1], False, periodic)
        v = _wide(rng, (ncomp, len(pts)))
        want = GA.transpose(ids, w, v, op.nsrc).reshape((ncomp,) + op.prepared_shape)
        first = op.transpose(v, prepared=True)
        assert op.noutside == nout and np.array_equal(op.ids.numpy(), ids) and G.same_bits(op.w.numpy(), w)
        assert G.same_bits(first, want)
        assert G.same_bits(op.transpose(ctx.to_device(v), prepared=True), first)      # again, from the device: the same bits
        back = op.transpose(v)
        assert back.shape == (ncomp,) + op.grid_shape and G.same_bits(back, GA.fold(want, flipped, appended))
        assert G.same_bits(op.coverage(), GA.fold(GA.transpose(ids, w, np.ones(len(pts)), op.nsrc).reshape(op.prepared_shape),
                                                  flipped, appended))
        if ncomp == 1:
            assert G.same_bits(op.transpose(v[0].reshape(op.lead)), back)
        op.free()


def test_inner_products_agree(ctx):
    """<G m, g> and <m, G^T g> are two orders of the same 8 N products w m g: each side rounds the product twice and adds
    at most 8 N + 2 terms, so either differs from the exact sum by at most (8 N + 2) eps sum|w m g| to first order."""
    pts = GA.mixed_points()[:-1]
    n = len(pts)
    rng = np.random.default_rng(50)
    with api.grid_import_operator(api.RegularGrid(G.DEPTH, G.LAT, G.LON, {}), pts, context=ctx) as op:
        m, g = rng.normal(size=(1, 7, 9, 11)), rng.normal(size=n)
        gm = op.apply(m, fill_value=0.0)[0]
        gtg = op.transpose(g)[0]
        ids, w = op.ids.numpy(), op.w.numpy()
    lhs, rhs = np.dot(gm, g), np.dot(m.reshape(-1), gtg.reshape(-1))
    scale = np.abs(w * m.reshape(-1)[ids] * g[:, None]).sum()
    print(f"|<Gm, g> - <m, G^T g>| = {abs(lhs - rhs):.3e}, bound {2 * (8 * n + 2) * EPS * scale:.3e}")
    assert abs(lhs - rhs) <= 2 * (8 * n + 2) * EPS * scale


def test_chunked_transpose_equals_the_chunk_statement(ctx):
    pts = np.ascontiguousarray(GA.mixed_points()[3::10])      # ~200 points: chunk_points = 1 is one chunk per point
    n = len(pts)
    v = _wide(np.random.default_rng(60), (2, n))
    nsrc = 7 * 9 * 11
    with api.grid_import_operator(api.RegularGrid(G.DEPTH, G.LAT, G.LON, {}), pts, context=ctx) as op:
        whole = op.transpose(v)
        ids, w, nout = op.ids.numpy(), op.w.numpy(), op.noutside
        for chunk in (1, 7, n - 1, n):
            got = op.transpose(v, chunk_points=chunk)
            assert G.same_bits(got, GA.chunked_transpose(ids, w, v, nsrc, chunk).reshape(2, 7, 9, 11)), chunk
            assert op.noutside == nout
        assert G.same_bits(op.transpose(v, chunk_points=n), whole)
        assert G.same_bits(op.transpose(ctx.to_device(v), chunk_points=7), op.transpose(v, chunk_points=7))
        with pytest.raises(ValueError, match="chunk_points"):
            op.transpose(v, chunk_points=0)
    # a chunked pass does not need the resident operator
    with api.grid_import_operator(api.RegularGrid(G.DEPTH, G.LAT, G.LON, {}), pts, context=ctx) as lazy:
        assert G.same_bits(lazy.transpose(v, chunk_points=n), whole) and lazy.ids is None and lazy.noutside == nout


# ---------------------------------------------------------------------------------------------- 4. regular_grid_adjoint
CONTAINING = (np.array([-1_000.0, 20_000.0, 90_000.0, 200_000.0, 401_000.0]), np.linspace(-9.0, 9.0, 13), np.linspace(-9.0, 9.0, 10))


def _check_adjoint(ctx, mesh, pts, mass, fields, axes):
    """regular_grid_adjoint == the statement composed from the mass; conservation; the normalised constant"""
    depth, lat, lon = axes
    grid = api.RegularGrid(depth, lat, lon, {})
    n = mass.size
    names = list(fields)
    K = np.stack([fields[p].reshape(-1) for p in names])
    lld = _lld(ctx, pts.reshape(-1, 3), depth, lat, lon)
    ids, w, nout, _ = GA.operator(depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1])
    shape = (len(depth), len(lat), len(lon))
    nsrc = int(np.prod(shape))
    m = mass.reshape(-1)
    out = api.regular_grid_adjoint(grid, mesh, names, context=ctx)
    assert out.nmissing == nout and list(out.data_vars) == names + ["volume"]
    for c, p in enumerate(names):
        assert G.same_bits(out[p], GA.transpose(ids, w, m * K[c], nsrc).reshape(shape)), p
    assert G.same_bits(out["volume"], GA.transpose(ids, w, m, nsrc).reshape(shape))
    plain = api.regular_grid_adjoint(grid, mesh, names, mass=False, context=ctx)
    assert G.same_bits(plain[names[0]], GA.transpose(ids, w, K[0], nsrc).reshape(shape))
    assert G.same_bits(plain["volume"], GA.transpose(ids, w, np.ones(n), nsrc).reshape(shape))
    if nout == 0:
        # sum_grid G^T(M K) = sum_n (sum_c w_nc) (M K)_n, and a row sums to 1 within 4 eps: with the products' roundings and
        # sums of at most 8 N (the transposes), nsrc (the grid) and N (the mesh) terms, both sides are within
        # (8 N + nsrc + 8) eps sum|M K| of the exact integral to first order
        for c, p in enumerate(names):
            total, want = out[p].sum(), np.sum(m * K[c])
            bound = 2 * (8 * n + nsrc + 8) * EPS * np.abs(m * K[c]).sum()
            print(f"{p}: |sum_grid - sum M K| = {abs(total - want):.3e}, bound {bound:.3e}")
            assert abs(total - want) <= bound
        assert abs(out["volume"].sum() - m.sum()) <= 2 * (8 * n + nsrc + 8) * EPS * m.sum()
    norm = api.regular_grid_adjoint(grid, mesh, ["const"], normalise=True, context=ctx)
    covered = norm["volume"] > 0.0
    assert G.same_bits(norm["volume"], out["volume"]) and covered.any()
    # sum_i w_i (M_i c) / sum_i w_i M_i with every term >= 0: the two sums run in the same order over terms that differ by
    # the factor c and one rounding each, the division adds one more; held to the 16 eps the feature states for it
    assert np.abs(norm["const"][covered] - 2.5).max() <= 16 * EPS * 2.5
    assert not norm["const"][~covered].any()
    return nout


@pytest.mark.parametrize("order", [2, 4])
def test_regular_grid_adjoint_on_a_gll_mesh(ctx, order):
    chunk = synth.earth_chunk(order, nlat=4, nlon=4)
    pts = chunk["points"]
    rng = np.random.default_rng(order)
    fields = {"K1": rng.normal(size=pts.shape[:2]), "K2": _wide(rng, pts.shape[:2]), "const": np.full(pts.shape[:2], 2.5)}
    mesh = api.GllMesh(pts, order, fields)
    mass = api.gll_mass_matrix(mesh, context=ctx)
    assert _check_adjoint(ctx, mesh, pts, mass, {p: fields[p] for p in ("K1", "K2")}, CONTAINING) == 0
    assert _check_adjoint(ctx, mesh, pts, mass, {"K1": fields["K1"]}, (G.DEPTH, G.LAT, G.LON)) > 0      # a grid the mesh sticks out of


def test_regular_grid_adjoint_on_a_hex_mesh(ctx):
    hp, hc = synth.hex_mesh(6, seed=2, lo=(5.9e6, -4.0e5, -4.0e5), hi=(6.4e6, 4.0e5, 4.0e5))
    mesh = api.HexMesh(hp, hc)
    rng = np.random.default_rng(6)
    fields = {"K1": rng.normal(size=len(hp)), "const": np.full(len(hp), 2.5)}
    for p, v in fields.items():
        mesh.attach_field(p, v)
    mass = api.hex8_mass_matrix(mesh, context=ctx)
    axes = (np.linspace(-80_000.0, 500_000.0, 6), np.linspace(-4.5, 4.5, 7), np.linspace(-4.5, 4.5, 8))
    assert _check_adjoint(ctx, mesh, hp, mass, {"K1": fields["K1"]}, axes) == 0


def test_regular_grid_adjoint_of_a_salvus_model_and_on_the_sphere_map(ctx):
    """A readable Salvus model gives what the GllMesh of its arrays gives; make_spherical evaluates the coordinates on the
    mapped copy and weights with the mass of the mesh's own geometry."""
    from multimesh_amd import io as mio

    chunk = synth.earth_chunk(2, nlat=4, nlon=4, ellipticity=3.35e-3, topography=3e-4)
    pts = chunk["points"]
    E, P = pts.shape[:2]
    K = np.random.default_rng(9).normal(size=(E, P))
    mesh = api.GllMesh(pts, 2, {"K1": K, "z_node_1D": chunk["z_node_1D"]})
    model = np.stack([np.zeros((E, P)), K, chunk["z_node_1D"]], axis=1)              # [E, 3, P]
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=pts)
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=model), ["RHO", "K1", "z_node_1D"])
    depth, lat, lon = CONTAINING
    grid = api.RegularGrid(depth, lat, lon, {})
    shape = (len(depth), len(lat), len(lon))
    m = api.gll_mass_matrix(mesh, context=ctx).reshape(-1)
    results = []
    for spherical in (False, True):
        at = api._sphere_mapped(mesh, ctx).numpy() if spherical else pts
        lld = _lld(ctx, at.reshape(-1, 3), depth, lat, lon)
        ids, w, nout, _ = GA.operator(depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1])
        want = GA.transpose(ids, w, m * K.reshape(-1), int(np.prod(shape))).reshape(shape)
        from_mesh = api.regular_grid_adjoint(grid, mesh, ["K1"], make_spherical=spherical, context=ctx)
        from_file = api.regular_grid_adjoint(grid, f, ["K1"], make_spherical=spherical, context=ctx)
        for out in (from_mesh, from_file):
            assert out.nmissing == nout and G.same_bits(out["K1"], want)
            assert G.same_bits(out["volume"], GA.transpose(ids, w, m, int(np.prod(shape))).reshape(shape))
        results.append(want)
    assert not G.same_bits(results[0], results[1])              # the sphere map changes where the nodes lie in the grid
    assert np.array_equal(mesh.gll_points, pts) and np.array_equal(f["MODEL/coordinates"][()], pts)
    with pytest.raises(ValueError, match="not in the model"):
        api.regular_grid_adjoint(grid, f, ["VS"], context=ctx)


# ---------------------------------------------------------------------------------------------- 5. whose memory it is
def test_operator_borrows_a_callers_device_array(ctx):
    """Freeing or collecting the operator leaves the caller's points, and views made of them, as they were"""
    pts = GA.mixed_points()[:-1]
    grid = api.RegularGrid(G.DEPTH, G.LAT, G.LON, {})
    mine = ctx.to_device(pts)
    view = mine.rows(100, 400)
    ptr = mine.ptr
    v = np.random.default_rng(70).normal(size=(1, len(pts)))
    op = api.grid_import_operator(grid, mine, context=ctx)
    first = op.transpose(v)
    op.free()
    assert mine.ptr == ptr != 0 and mine._owner and view.ptr == ptr + 100 * 24
    with pytest.raises(ValueError, match="freed"):
        op.transpose(v)
    with api.grid_import_operator(grid, mine, context=ctx) as again:       # leaving the block frees the operator
        assert G.same_bits(again.transpose(v), first)
    del again, op
    assert mine.ptr == ptr and G.same_bits(mine.numpy(), pts) and G.same_bits(view.numpy(), pts[100:400])
    ids, w, nout = ctx.grid_operator(view, G.DEPTH, G.LAT, G.LON)           # the caller goes on using its arrays
    whole = ctx.grid_operator(mine, G.DEPTH, G.LAT, G.LON)
    assert np.array_equal(ids.numpy(), whole[0].numpy()[100:400]) and G.same_bits(w.numpy(), whole[1].numpy()[100:400])
    mine.free()


def test_operator_without_points(ctx):
    grid = api.RegularGrid(G.DEPTH, G.LAT, G.LON, {})
    with api.grid_import_operator(grid, np.zeros((0, 3)), context=ctx) as op:
        back = op.transpose(np.zeros((2, 0)))
        assert back.shape == (2, 7, 9, 11) and not back.any() and not np.signbit(back).any() and op.noutside == 0
        assert G.same_bits(op.transpose(np.zeros((2, 0)), chunk_points=5), back)
        assert not op.coverage().any() and op.apply(G.grid_values(2)).shape == (2, 0)


def test_operator_wraps_as_the_import_of_the_same_grid_wraps(ctx):
    """-180 ... 180 with equal end columns wraps, with different ones it does not: in both cases the gather through the
    operator agrees with import_regular_grid's values for that grid, also at longitude 180"""
    lat, depth, lon = np.linspace(-90.0, 90.0, 37), np.array([-100_000.0, 3_000_000.0]), np.linspace(-180.0, 180.0, 73)
    same = G.periodic_field(lat, lon, depth)
    pts = np.concatenate([G.sphere_points(500, seed=14), GA.xyz(np.linspace(-80.0, 80.0, 9), 180.0, 200_000.0)])
    for field in (same, same + lon[None, None, :]):
        grid = api.RegularGrid(depth, lat, lon, {"v": field})
        want, miss = api.sample_regular_grid(grid, pts, context=ctx)
        with api.grid_import_operator(grid, pts, context=ctx) as op:
            got = op.apply(grid)
            assert op.periodic == api.prepare_regular_grid(grid)[5] == (field is same) and op.noutside == miss == 0
        assert (np.abs(got - want) <= 32 * EPS * np.abs(field).max()).all()


# ---------------------------------------------------------------------------------------------- 6. caller views and stream
def _caller_case():
    pts = GA.mixed_points()

    def call(ctx, a, o):
        return ctx.grid_operator(a.pts, a.depth, a.lat, a.lon, latlondepth=True, ids_out=o.ids, weights_out=o.w)

    def expect(ref):                                          # the statement on the device's own coordinates
        lld = ref[3]
        ids, w, nout, _ = GA.operator(G.DEPTH, G.LAT, G.LON, lld[:, 2], lld[:, 0], lld[:, 1])
        assert 0.1 * len(pts) < nout < 0.45 * len(pts)
        return [ids, w, nout, None]

    return Case(dict(pts=pts, depth=G.DEPTH, lat=G.LAT, lon=G.LON), call, expect,
                outs=dict(ids=((len(pts), 8), np.int64), w=((len(pts), 8), np.float64)))


def test_operator_on_views_off_16_byte_alignment(torch, ctx):
    """points, ids and w 8 bytes past a 16-byte boundary (the rows then go out as single entries), with guarded borders"""
    case = _caller_case()
    ref, _ = _run_reference(ctx, case)
    want = case.expect(ref)
    _same_as(ref, want, _bits, "NumPy inputs against the statement")
    for misaligned in (False, True):
        what = ("grid_operator", "misaligned views" if misaligned else "aligned views")
        got = _run_on_views(torch, ctx, case, misaligned, what)
        _same_as(got, ref, _bits, what + ("against NumPy inputs",))
        _same_as(got, want, _bits, what + ("against the statement",))


def test_operator_on_a_caller_stream(torch, ctx):
    """Late producer, early consumer on a side stream, as tests/test_caller_stream_gpu.py"""
    case = _caller_case()
    _run_reference(ctx, case)
    ref, seconds = _run_reference(ctx, case)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    _spin_ms(torch, side, 1_000_000)
    per_cycle = _spin_ms(torch, side, 20_000_000) / 20_000_000
    cycles = int(np.ceil(max(SPIN_FACTOR * seconds * 1e3, SPIN_FLOOR_MS) / per_cycle))
    with Context(0, stream=side.cuda_stream) as ctx_side:
        got = _run_on_side(torch, side, ctx_side, case, cycles)
    _same_as(got, ref, _bits, "caller's stream against the null stream")
    _same_as(got, case.expect(ref), _bits, "caller's stream against the statement")
