"""mm_sample_grid and the drivers over it on the GPU, against the NumPy statement of tests/grid_import_cases.py.

The device's acos and atan2 are the only part that cannot be bit for bit: the coordinates are compared with NumPy's within
1e-11 degrees (test_coordinates: ~350 ulp of an angle of up to 180 degrees, whose ulp is 2.8e-14; a single-precision or
fast-math path errs by >= 1e-6), the depth bit for bit.  Everything after them is compared bit for bit, by evaluating the
statement on the coordinates the device returned."""
import numpy as np
import pytest

import grid_import_cases as G
from multimesh_amd import api, io as mio, synth
from multimesh_amd.device import Context

pytestmark = pytest.mark.gpu

ANGLE_TOL = 1e-11          # degrees


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def _device_lld(ctx, points, depth, lat, lon, periodic=False):
    """The coordinates alone: ncomp == 0"""
    empty = np.zeros((0, len(depth), len(lat), len(lon)))
    vals, _, lld = ctx.sample_grid(points, empty, depth, lat, lon, lon_periodic=periodic, want_latlondepth=True)
    assert vals.shape == (0, len(np.asarray(points).reshape(-1, 3)))
    return lld.numpy()


# ---------------------------------------------------------------------------------------------- 1. coordinates
def _coordinate_sets():
    for order in (1, 2, 4):
        for deform in ({}, {"ellipticity": 3.35e-3, "topography": 3e-4}):
            yield f"chunk order {order} {'deformed' if deform else 'plain'}", synth.earth_chunk(order, nlat=4, nlon=4, **deform)["points"]
    yield "sphere", G.sphere_points(4099)


def test_coordinates(ctx):
    worst = [0.0, 0.0]
    for name, pts in _coordinate_sets():
        ref = G.latlondepth(pts)
        got = _device_lld(ctx, pts, G.DEPTH, G.LAT, G.LON)
        dlat, dlon = np.abs(got[:, 0] - ref[:, 0]).max(), np.abs(got[:, 1] - ref[:, 1]).max()
        print(f"{name}: max |lat - numpy| = {dlat:.2e} deg, max |lon - numpy| = {dlon:.2e} deg")
        worst = [max(worst[0], dlat), max(worst[1], dlon)]
        assert G.same_bits(got[:, 2], ref[:, 2]), name
        assert dlat <= ANGLE_TOL and dlon <= ANGLE_TOL, (name, dlat, dlon)
    print(f"all sets: max |lat - numpy| = {worst[0]:.2e}, max |lon - numpy| = {worst[1]:.2e} degrees")


def test_coordinates_on_the_axes_are_exact(ctx):
    for radius in (6_000_000.0, 6_371_000.0, 1.0):
        pts = G.AXIS_POINTS * radius
        got = _device_lld(ctx, pts, G.DEPTH, G.LAT, G.LON)
        assert np.array_equal(got[:, :2], G.AXIS_LATLON), (radius, got)
        assert G.same_bits(got, G.latlondepth(pts)), radius


# ---------------------------------------------------------------------------------------------- 2. values, bit for bit
def _check_values(ctx, pts, grid, depth, lat, lon, mode, fill, periodic=False):
    """out == the statement on the device's own coordinates; -> (nmissing, inside)"""
    C, N = grid.shape[0], len(pts)
    prefilled = np.random.default_rng(C * 1000 + N).normal(size=(C, N))
    out, nmissing, lld = ctx.sample_grid(pts, grid, depth, lat, lon, outside=mode, fill_value=fill, lon_periodic=periodic,
                                         out=prefilled if mode == "keep" else None, want_latlondepth=True)
    out, lld = out.numpy(), lld.numpy()
    assert out.shape == (C, N) and lld.shape == (N, 3)
    want, nmiss_ref, inside = G.sample(grid, depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1], mode, fill, periodic, prefilled)
    assert nmissing == nmiss_ref == int((~inside).sum()), (mode, C, N, nmissing, nmiss_ref)
    assert G.same_bits(out, want), (mode, C, N)
    if mode == "keep":
        assert G.same_bits(out[:, ~inside], prefilled[:, ~inside])
        assert N == 0 or inside.sum() == 0 or not np.array_equal(out[:, inside], prefilled[:, inside])
    if mode == "clamp":
        assert nmissing == 0 and inside.all()
    return nmissing, inside


@pytest.mark.parametrize("fill", [np.nan, -12345.5])
@pytest.mark.parametrize("mode", G.MODES)
def test_values_bit_for_bit(ctx, mode, fill):
    all_pts = G.chunk_points(4099)
    for C in (1, 3, 4, 5):
        grid = G.grid_values(C)
        for N in (0, 1, 255, 256, 257, 4099):
            nmissing, inside = _check_values(ctx, all_pts[:N].reshape(N, 3), grid, G.DEPTH, G.LAT, G.LON, mode, fill)
            if mode == "fill" and N >= 255:      # (a fraction of 0 or 1 points is 0 or 1)
                assert 0.2 * N < nmissing < 0.8 * N, (N, nmissing)


def test_values_degenerate_axes_nan_corner_and_long_axes(ctx):
    pts = G.chunk_points(4099)
    for mode in G.MODES:
        # an axis of length 1 is constant along itself
        _check_values(ctx, pts, G.grid_values(3, (1, 9, 11)), G.DEPTH[3:4], G.LAT, G.LON, mode, np.nan)
        _check_values(ctx, pts, G.grid_values(3, (7, 9, 1)), G.DEPTH, G.LAT, G.LON[5:6], mode, np.nan)
        _check_values(ctx, pts[:300], G.grid_values(2, (1, 1, 1)), G.DEPTH[:1], G.LAT[:1], G.LON[:1], mode, np.nan)
        # a NaN node makes its cells NaN, also where its weight is 0
        grid = G.grid_values(4)
        grid[1, 3, 4, 5] = np.nan
        grid[2, 0, 0, 0] = np.nan
        _check_values(ctx, pts, grid, G.DEPTH, G.LAT, G.LON, mode, -1.0)
        # axes too long for LDS are bisected in global memory
        lon = np.linspace(-5.5, 6.5, 9001)
        _check_values(ctx, pts, G.grid_values(3, (3, 3, 9001)), G.DEPTH[[0, 3, 6]], G.LAT[[0, 4, 8]], lon, mode, np.nan)
    grid = G.grid_values(1)
    grid[0, 3, 4, 5] = np.nan
    out, _, lld = ctx.sample_grid(pts, grid, G.DEPTH, G.LAT, G.LON, want_latlondepth=True)
    _, _, inside = G.sample(grid, G.DEPTH, G.LAT, G.LON, *lld.numpy()[:, [2, 0, 1]].T)
    assert 0 < np.isnan(out.numpy()[0, inside]).sum() < inside.sum()


def test_argument_errors(ctx):
    pts, grid = G.chunk_points(10), G.grid_values(1)
    with pytest.raises(ValueError, match="keep"):
        ctx.sample_grid(pts, grid, G.DEPTH, G.LAT, G.LON, outside="keep")
    with pytest.raises(ValueError, match="ascending"):
        ctx.sample_grid(pts, grid, G.DEPTH, G.LAT[::-1], G.LON)
    with pytest.raises(ValueError, match="grid_values"):
        ctx.sample_grid(pts, grid[:, :, :, :-1], G.DEPTH, G.LAT, G.LON)
    with pytest.raises(ValueError, match="periodic"):
        ctx.sample_grid(pts, grid, G.DEPTH, G.LAT, G.LON, lon_periodic=True)
    d, la, lo, g, p = (ctx.to_device(a) for a in (G.DEPTH, G.LAT, G.LON, grid, pts))
    out = ctx.to_device(np.full((1, 10), 7.0))
    rc = ctx.lib.mm_sample_grid(ctx.handle, p.ptr, 10, d.ptr, 7, la.ptr, 9, lo.ptr, 11, g.ptr, 1, 0, 3, 0.0, out.ptr, None)
    assert rc == -1
    rc = ctx.lib.mm_sample_grid(ctx.handle, p.ptr, 10, d.ptr, 7, None, 9, lo.ptr, 11, g.ptr, 1, 0, 0, 0.0, out.ptr, None)
    assert rc == -1
    rc = ctx.lib.mm_sample_grid(ctx.handle, p.ptr, 10, d.ptr, 7, la.ptr, 0, lo.ptr, 11, g.ptr, 1, 0, 0, 0.0, out.ptr, None)
    assert rc == -1
    assert np.array_equal(out.numpy(), np.full((1, 10), 7.0))


# ---------------------------------------------------------------------------------------------- 3. periodic longitude
def test_periodic_longitude(ctx):
    pts = G.sphere_points(4099)
    lat, depth = np.linspace(-90.0, 90.0, 73), np.array([-100_000.0, 500_000.0, 1_500_000.0, 3_000_000.0])
    results = []
    for lon in (np.arange(0.0, 360.0, 2.5), np.linspace(-180.0, 180.0, 145)):
        field = G.periodic_field(lat, lon, depth)
        grid = api.RegularGrid(depth, lat, lon, {"v": field})
        values, nmissing = api.sample_regular_grid(grid, pts, context=ctx)
        assert nmissing == 0 and values.shape == (1, 4099)
        d, la, lo, data, _, periodic = api.prepare_regular_grid(grid)
        assert periodic
        lld = _device_lld(ctx, pts, d, la, lo, periodic=True)
        assert lld[:, 1].min() >= lo[0] and lld[:, 1].max() < lo[0] + 360.0
        want, miss, _ = G.sample(data, d, la, lo, lld[:, 2], lld[:, 0], lld[:, 1], "fill", np.nan, True)
        assert miss == 0 and G.same_bits(values, want)
        results.append((values, field))
    (va, fa), (vb, fb) = results
    assert np.array_equal(fa, np.roll(fb[..., :-1], -72, axis=2))  # the same function at the nodes (column 72 is lon 0)
    slope = np.abs(np.diff(fb, axis=2)).max() / 2.5               # per degree
    diff = np.abs(va - vb).max()
    print(f"max |0...357.5 - (-180...180)| = {diff:.2e}")
    assert diff <= 1e-11 * slope + 1e-13 * np.abs(fb).max()
    # without the wrap the western hemisphere lies outside 0 ... 357.5
    grid = api.RegularGrid(depth, lat, np.arange(0.0, 360.0, 2.5), {"v": fa})
    assert api.sample_regular_grid(grid, pts, lon_periodic=False, context=ctx)[1] > 1500


# ---------------------------------------------------------------------------------------------- 4. exact edges
def test_points_on_the_last_node(ctx):
    r0 = 6_000_000.0
    depth = np.array([100_000.0, 250_000.0, G.R_EARTH - r0])
    cases = [([0.0, 0.0, r0], [30.0, 60.0, 90.0], [-10.0, -5.0, 0.0], -1, -1),        # lat 90, lon 0: the last nodes
             ([0.0, 0.0, -r0], [-90.0, -60.0, -30.0], [-10.0, -5.0, 0.0], 0, -1),     # lat -90: the first node
             ([r0, 0.0, 0.0], [-30.0, -10.0, 0.0], [-10.0, -5.0, 0.0], -1, -1),       # lat 0, lon 0
             ([-r0, 0.0, 0.0], [-30.0, -10.0, 0.0], [90.0, 135.0, 180.0], -1, -1),    # lon 180
             ([0.0, r0, 0.0], [-30.0, -10.0, 0.0], [0.0, 45.0, 90.0], -1, -1),        # lon 90
             ([0.0, -r0, 0.0], [0.0, 10.0, 30.0], [-90.0, -45.0, 0.0], 0, 0)]         # lat 0 and lon -90 as first nodes
    for mode in G.MODES:
        for p, lat, lon, jl, il in cases:
            grid = G.grid_values(2, (3, 3, 3), seed=9)
            out, nmissing = ctx.sample_grid(np.array([p]), grid, depth, np.array(lat), np.array(lon), outside=mode,
                                            fill_value=-7.0, out=np.full((2, 1), -9.0) if mode == "keep" else None)
            assert nmissing == 0, (mode, p)
            assert G.same_bits(out.numpy()[:, 0], grid[:, -1, jl, il]), (mode, p)


# ---------------------------------------------------------------------------------------------- 5. affine reproduction
def test_affine_grid_is_reproduced_end_to_end(ctx):
    a, b, c, d = 0.37, -0.21, 2.5e-6, 4.0
    depth = np.array([-1_000.0, 20_000.0, 90_000.0, 200_000.0, 401_000.0])
    lat, lon = np.linspace(-9.0, 9.0, 13), np.linspace(-9.0, 9.0, 10)
    g = a * lat[None, :, None] + b * lon[None, None, :] + c * depth[:, None, None] + d
    grid = api.RegularGrid(depth, lat, lon, {"V": g})
    chunk = synth.earth_chunk(4, nlat=4, nlon=4)
    mesh = api.GllMesh(chunk["points"], 4)
    assert api.import_regular_grid(grid, mesh, outside="fill", context=ctx) == 0
    got = mesh.element_nodal_fields["V"]
    assert got.shape == chunk["points"].shape[:2]
    lld = G.latlondepth(chunk["points"])
    want = a * lld[:, 0] + b * lld[:, 1] + c * lld[:, 2] + d
    err = np.abs(got.reshape(-1) - want).max()
    print(f"affine: max error {err:.2e}")
    assert err <= (abs(a) + abs(b)) * ANGLE_TOL + 1e-13 * np.abs(g).max()


# ---------------------------------------------------------------------------------------------- 6. API paths
def _named_grid(ncomp=2):
    vals = G.grid_values(ncomp)
    return api.RegularGrid(G.DEPTH, G.LAT, G.LON, {f"P{c}": vals[c] for c in range(ncomp)})


def test_import_onto_gll_and_hex_meshes(ctx):
    grid = _named_grid()
    chunk = synth.earth_chunk(2, nlat=4, nlon=4)
    pts = chunk["points"]
    flat = pts.reshape(-1, 3)
    fill_vals, miss = api.sample_regular_grid(grid, flat, outside="fill", fill_value=-3.0, context=ctx)
    assert 0 < miss < len(flat)
    old = np.random.default_rng(4).normal(size=(2,) + pts.shape[:2])
    mesh = api.GllMesh(pts, 2, {"P0": old[0], "P1": old[1], "other": old[0] + 1.0})
    assert api.import_regular_grid(grid, mesh, context=ctx) == miss                    # keep
    outside = fill_vals[0] == -3.0
    for c, p in enumerate(("P0", "P1")):
        got = mesh.element_nodal_fields[p].reshape(-1)
        assert G.same_bits(got[~outside], fill_vals[c][~outside]) and G.same_bits(got[outside], old[c].reshape(-1)[outside])
    assert G.same_bits(mesh.element_nodal_fields["other"], old[0] + 1.0) and mesh.gll_points is not None
    assert np.array_equal(mesh.gll_points, pts)
    only = api.GllMesh(pts, 2)
    assert api.import_regular_grid(grid, only, parameters=["P1"], outside="fill", fill_value=-3.0, context=ctx) == miss
    assert list(only.element_nodal_fields) == ["P1"] and G.same_bits(only.element_nodal_fields["P1"].reshape(-1), fill_vals[1])

    hp, hc = synth.hex_mesh(6, seed=2, lo=(5.9e6, -4.0e5, -4.0e5), hi=(6.4e6, 4.0e5, 4.0e5))
    hex_mesh = api.HexMesh(hp, hc)
    clamp_vals, _ = api.sample_regular_grid(grid, hp, outside="clamp", context=ctx)
    assert api.import_regular_grid(grid, hex_mesh, outside="clamp", context=ctx) == 0
    assert G.same_bits(hex_mesh.get_nodal_field("P0"), clamp_vals[0]) and G.same_bits(hex_mesh.get_nodal_field("P1"), clamp_vals[1])


def test_import_into_a_salvus_model_and_make_spherical(ctx, tmp_path):
    grid = _named_grid()
    path = str(tmp_path / "grid.nc")
    grid.to_netcdf(path)
    chunk = synth.earth_chunk(2, nlat=4, nlon=4, ellipticity=3.35e-3, topography=3e-4)
    pts = chunk["points"]
    E, P = pts.shape[:2]
    model = np.random.default_rng(8).normal(size=(E, 4, P))
    model[:, 2, :] = chunk["z_node_1D"]

    def salvus():
        f = mio.MemoryH5()
        f.create_dataset("MODEL/coordinates", data=pts)
        mio.set_dimension_labels(f.create_dataset("MODEL/data", data=model), ["RHO", "P1", "z_node_1D", "P0"])
        return f

    for spherical in (False, True):
        f = salvus()
        mesh = api.GllMesh(pts, 2, {"z_node_1D": chunk["z_node_1D"]})
        at = api._sphere_mapped(mesh, ctx).numpy() if spherical else pts
        want, miss = api.sample_regular_grid(grid, at.reshape(-1, 3), outside="fill", fill_value=0.5, context=ctx)
        got_miss = api.import_regular_grid(path, f, outside="fill", fill_value=0.5, make_spherical=spherical, context=ctx)
        data = f["MODEL/data"][()]
        assert got_miss == miss and 0 < miss < E * P
        assert G.same_bits(data[:, 3, :].reshape(-1), want[0]) and G.same_bits(data[:, 1, :].reshape(-1), want[1])
        assert G.same_bits(data[:, 0, :], model[:, 0, :]) and G.same_bits(data[:, 2, :], model[:, 2, :])
        assert np.array_equal(f["MODEL/coordinates"][()], pts)
        # the same through a GllMesh, whose coordinates do not move either
        assert api.import_regular_grid(grid, mesh, outside="fill", fill_value=0.5, make_spherical=spherical, context=ctx) == miss
        assert G.same_bits(mesh.element_nodal_fields["P0"].reshape(-1), want[0]) and np.array_equal(mesh.gll_points, pts)
    plain, _ = api.sample_regular_grid(grid, pts.reshape(-1, 3), outside="fill", fill_value=0.5, context=ctx)
    assert not G.same_bits(plain, want)                           # the sphere map changes what is sampled
    # keep starts from the columns of the file
    f = salvus()
    assert api.import_regular_grid(grid, f, parameters=["P0"], context=ctx) > 0
    data = f["MODEL/data"][()]
    outside = plain[0] == 0.5
    col = data[:, 3, :].reshape(-1)
    assert G.same_bits(col[outside], model[:, 3, :].reshape(-1)[outside]) and G.same_bits(col[~outside], plain[0][~outside])
    assert G.same_bits(data[:, :3, :], model[:, :3, :])


def test_components_together_or_one_at_a_time(ctx):
    pts, grid = G.chunk_points(4099), G.grid_values(5)
    together, miss = ctx.sample_grid(pts, grid, G.DEPTH, G.LAT, G.LON, fill_value=-1.0)
    together = together.numpy()
    for c in range(5):
        one, miss_c = ctx.sample_grid(pts, grid[c], G.DEPTH, G.LAT, G.LON, fill_value=-1.0)
        assert miss_c == miss and G.same_bits(one.numpy()[0], together[c])
