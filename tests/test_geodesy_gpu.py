"""mm_geographic_points on the GPU against the NumPy statement of tests/geodesy_cases.py, bit for bit (NaN positions
compared, payloads not: they are the processor's), what it refuses, and the Python layer of :mod:`multimesh_amd.geodesy` on
meshes: as_geographic with the regular-grid import, the heights of an elliptical chunk's free surface, the depth of the 1-D
model, and extract_geographic_grid against the geocentric extraction."""
import ctypes as C

import numpy as np
import pytest

import geodesy_cases as GC
from multimesh_amd import api, device, synth
from multimesh_amd import geodesy as G
from multimesh_amd.api import GllMesh, RegularGrid
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

CAP_LANES = 8192 * 256          # the launch cap of the kernels: beyond, the workgroups stride
WGS84 = GC.constants()
F = GC.WGS84_F


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()      # before this module's context opens the device: torch then finds it whichever test runs first
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    with Context(0) as c:
        yield c


# -------------------------------------------------------------------------------------------------- mm_geographic_points
@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, CAP_LANES + 3))
def test_both_directions_are_the_statement_bit_for_bit(ctx, n):
    """Out of place and in place, with and without radius_d / height_out_d; the first rows hold +-0.0, +-inf, NaN, both poles
    and the centre.  8192 * 256 + 3 points: the stride loop takes a second trip, of three lanes."""
    pts = GC.points_with_specials(n, seed=n % 1000)
    rho = GC.radii(n, seed=n % 1000)
    want0, want_h = GC.to_geographic(WGS84, pts)
    want0r, _ = GC.to_geographic(WGS84, pts, radius=rho)
    want1 = GC.from_geographic(WGS84, pts)
    if n >= 255:
        assert np.isnan(want0[4]).all() and np.isfinite(want0[:4]).all() and np.isfinite(want0[20:]).all()
        assert not np.array_equal(want0[20:], want1[20:]) and not np.array_equal(want0[20:], want0r[20:])
    src = ctx.to_device(pts)
    # direction 0, out of place: plain, then with both optional arrays
    out = G.geographic_points_on_device(ctx, src, WGS84)
    assert out.ptr != src.ptr and out.shape == (n, 3)
    assert GC.same_bits_nan(out.numpy(), want0)
    heights = ctx.to_device(np.full(n, -7.0))
    out = G.geographic_points_on_device(ctx, src, WGS84, radius=ctx.to_device(rho), height_out=heights)
    assert GC.same_bits_nan(out.numpy(), want0r) and GC.same_bits_nan(heights.numpy(), want_h)
    # ... each alone
    assert GC.same_bits_nan(G.geographic_points_on_device(ctx, src, WGS84, radius=ctx.to_device(rho)).numpy(), want0r)
    heights = ctx.to_device(np.full(n, -7.0))
    assert GC.same_bits_nan(G.geographic_points_on_device(ctx, src, WGS84, height_out=heights).numpy(), want0)
    assert GC.same_bits_nan(heights.numpy(), want_h)
    # direction 1, out of place
    assert GC.same_bits_nan(G.geographic_points_on_device(ctx, src, WGS84, G.TO_CARTESIAN).numpy(), want1)
    assert np.array_equal(src.numpy().view(np.uint64), pts.view(np.uint64))                 # the input is untouched
    # in place: direction 0 with both arrays, direction 0 plain, direction 1
    heights = ctx.to_device(np.full(n, -7.0))
    same = G.geographic_points_on_device(ctx, src, WGS84, out=src, radius=ctx.to_device(rho), height_out=heights)
    assert same.ptr == src.ptr and GC.same_bits_nan(src.numpy(), want0r) and GC.same_bits_nan(heights.numpy(), want_h)
    src = ctx.to_device(pts)
    G.geographic_points_on_device(ctx, src, WGS84, out=src)
    assert GC.same_bits_nan(src.numpy(), want0)
    src = ctx.to_device(pts)
    G.geographic_points_on_device(ctx, src, WGS84, G.TO_CARTESIAN, out=src)
    assert GC.same_bits_nan(src.numpy(), want1)


def test_on_a_callers_stream_with_the_callers_tensors_off_alignment(torch):
    """Late producer, early consumer, as tests/test_caller_stream_gpu.py: under a side stream the inputs hold zeros while the
    stream spins, the true values are copied in on that stream, the library is called and its outputs are cloned and
    overwritten right after, with no host synchronisation in between.  Every array is a view that starts 8 bytes into its
    buffer (off 16-byte alignment), as in tests/test_caller_views_gpu.py."""
    n = 1000
    pts, rho = GC.points_with_specials(n, seed=9), GC.radii(n, seed=9)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    staged, staged_rho = torch.from_numpy(pts).cuda(), torch.from_numpy(rho).cuda()
    torch.cuda.synchronize()

    def view(fill, shape):
        buffer = torch.full((int(np.prod(shape)) + 1,), fill, dtype=torch.float64, device="cuda")
        v = buffer[1:].view(shape)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v

    with Context(0, stream=side.cuda_stream) as ctx, torch.cuda.stream(side):
        tin, tout, tsame = view(0.0, pts.shape), view(-7.0, pts.shape), view(0.0, pts.shape)
        trho, theights = view(0.0, (n,)), view(-7.0, (n,))
        torch.cuda._sleep(30_000_000)
        tin.copy_(staged, non_blocking=True), tsame.copy_(staged, non_blocking=True), trho.copy_(staged_rho, non_blocking=True)
        res = G.to_geographic(tin, WGS84, radius=trho, out=tout, height_out=theights, context=ctx)
        assert res.ptr == tout.data_ptr()
        G.from_geographic(tsame, WGS84, out=tsame, context=ctx)
        got, got_h, got_same = tout.clone(), theights.clone(), tsame.clone()
        tout.fill_(-7.0), theights.fill_(-7.0), tsame.fill_(-7.0), tin.fill_(-7.0), trho.fill_(-7.0)
        side.synchronize()
        got, got_h, got_same = got.cpu().numpy(), got_h.cpu().numpy(), got_same.cpu().numpy()
    want, want_h = GC.to_geographic(WGS84, pts, radius=rho)
    assert GC.same_bits_nan(got, want) and GC.same_bits_nan(got_h, want_h)
    assert GC.same_bits_nan(got_same, GC.from_geographic(WGS84, pts))


def test_every_refusal_is_a_value_error_and_writes_nothing(ctx):
    n = 100
    lib = G.bind(ctx.lib)
    pts = GC.cloud(n, seed=1)
    buf = ctx.to_device(np.concatenate([pts, np.full((n, 3), -7.0)]))                       # in: rows [0, n); out: rows [n, 2n)
    src, out = buf.rows(0, n), buf.rows(n, 2 * n)
    rho, heights = ctx.to_device(GC.radii(n)), ctx.to_device(np.full(n, -7.0))
    flat = buf.reshape(6 * n)
    before, before_h = buf.numpy().copy(), heights.numpy().copy()

    def ell(**changed):
        e = list(WGS84)
        for k, v in changed.items():
            e[int(k[1:])] = v
        return (C.c_double * 8)(*e)

    def call(handle=ctx.handle, count=n, a=src, b=out, e=ell(), direction=0, radius=None, height=None):
        device._call(lib, "mm_geographic_points", handle, count, a, b, e, direction, radius, height, arg_error=True)

    refused = {
        "null ctx": dict(handle=None),
        "negative n": dict(count=-1),
        "3 n at 2^48": dict(count=-(-(1 << 48) // 3)),
        "null in": dict(a=None),
        "null out": dict(b=None),
        "null ell": dict(e=None),
        "NaN in ell": dict(e=ell(e3=np.nan)),
        "inf in ell": dict(e=ell(e7=np.inf)),
        "a zero": dict(e=ell(e0=0.0)),
        "a negative": dict(e=ell(e0=-1.0)),
        "b zero": dict(e=ell(e1=0.0)),
        "b negative": dict(e=ell(e1=-1.0)),
        "direction 2": dict(direction=2),
        "direction -1": dict(direction=-1),
        "radius with direction 1": dict(direction=1, radius=rho),
        "height with direction 1": dict(direction=1, height=heights),
        "out one point into in": dict(b=buf.rows(1, n + 1)),
        "out ends inside in": dict(a=out, b=buf.rows(n - 1, 2 * n - 1)),
        "radius inside out": dict(radius=flat.rows(3 * n + 5, 4 * n + 5)),
        "radius over the start of out": dict(radius=flat.rows(2 * n + 1, 3 * n + 1)),
        "height inside out": dict(height=flat.rows(5 * n, 6 * n)),
        "height over the start of out": dict(height=flat.rows(2 * n + 1, 3 * n + 1)),
        "height inside out, in place": dict(b=src, height=flat.rows(0, n)),
    }
    for what, kw in refused.items():
        with pytest.raises(ValueError, match="mm_geographic_points"):
            call(**kw)
        ctx.synchronize()
        assert np.array_equal(buf.numpy().view(np.uint64), before.view(np.uint64)), what
        assert np.array_equal(heights.numpy(), before_h), what
    call(radius=rho, height=heights)                                                       # and the same arrays are accepted
    assert GC.same_bits_nan(out.numpy(), GC.to_geographic(WGS84, pts, radius=rho.numpy())[0])
    # the Python layer's own
    with pytest.raises(ValueError, match="3-D"):
        G.to_geographic(np.zeros((5, 2)), WGS84, context=ctx)
    with pytest.raises(ValueError, match="as many values"):
        G.geographic_points_on_device(ctx, src, WGS84, out=ctx.empty((50, 3), np.float64))
    with pytest.raises(ValueError, match="one value per point"):
        G.geographic_points_on_device(ctx, src, WGS84, radius=ctx.empty((50,), np.float64))
    with pytest.raises(ValueError, match="one value per point"):
        G.geographic_points_on_device(ctx, src, WGS84, height_out=ctx.empty((50,), np.float64))


def test_host_arrays_and_geodetic_coordinates(ctx):
    wgs = G.Ellipsoid.wgs84()
    pts = GC.cloud(4 * 27, seed=5, rmin=3_400_000.0).reshape(4, 27, 3)
    want, want_h = GC.to_geographic(WGS84, pts)
    heights = np.empty((4, 27))
    got = G.to_geographic(pts, wgs, height_out=heights, context=ctx)
    assert isinstance(got, np.ndarray) and got.shape == (4, 27, 3) and np.array_equal(got, want) and np.array_equal(heights, want_h)
    back = got.copy()
    assert G.from_geographic(back, wgs, out=back, context=ctx) is back and np.array_equal(back, GC.from_geographic(WGS84, want))
    assert np.abs(back - pts).max() <= 1e-7
    lat, lon, h = G.geodetic_coordinates(pts, wgs, context=ctx)
    assert lat.shape == lon.shape == h.shape == (4, 27) and np.array_equal(h, want_h)
    # the points these coordinates describe, through the textbook formulas and through direction 1
    assert np.abs(GC.textbook_points(lat, lon, h) - pts).max() <= 1e-7
    assert np.abs(G.geographic_points(lat, lon, -h, wgs, context=ctx) - pts).max() <= 1e-7
    assert G.geographic_points(np.zeros(0), 0.0, 0.0, wgs, context=ctx).shape == (0, 3)
    mesh = GllMesh(pts, 2, {})
    assert all(np.array_equal(a, b) for a, b in zip(G.geodetic_coordinates(mesh, wgs, context=ctx), (lat, lon, h)))


# ---------------------------------------------------------------------------------------------------------------- meshes
def _chunk():
    return synth.earth_chunk(order=2, nlat=4, nlon=4, lat=(40, 56), ellipticity=F)


def _cube(seed=3):
    rng = np.random.default_rng(seed)
    depth, lat, lon = np.linspace(-30_000.0, 450_000.0, 9), np.linspace(38.0, 58.0, 11), np.linspace(-10.0, 10.0, 10)
    return RegularGrid(depth, lat, lon, {"VSV": rng.uniform(3000.0, 5000.0, (9, 11, 10)), "RHO": rng.uniform(2500.0, 3500.0, (9, 11, 10))})


def test_as_geographic_with_the_regular_grid_import(ctx):
    chunk, grid, wgs = _chunk(), _cube(), G.Ellipsoid.wgs84()
    gp = chunk["points"]
    before = gp.copy()
    mesh = GllMesh(gp, 2, {"z_node_1D": chunk["z_node_1D"]})
    view = G.as_geographic(mesh, wgs, context=ctx)
    assert type(view) is GllMesh and view is not mesh and view.element_nodal_fields is mesh.element_nodal_fields
    pseudo = GC.to_geographic(WGS84, before)[0]
    assert np.array_equal(view.gll_points, pseudo) and view.gll_points is not mesh.gll_points
    assert np.array_equal(G.as_geographic(mesh, context=ctx).gll_points, pseudo)            # the default ellipsoid is WGS84
    missed = api.import_regular_grid(grid, view, outside="fill", fill_value=-1.0, context=ctx)
    want, nout = api.sample_regular_grid(grid, G.to_geographic(before, wgs, context=ctx).reshape(-1, 3), outside="fill",
                                         fill_value=-1.0, context=ctx)
    assert missed == nout == 0
    assert np.array_equal(mesh.gll_points.view(np.uint64), before.view(np.uint64))          # the caller's coordinates: unchanged
    assert sorted(mesh.element_nodal_fields) == ["RHO", "VSV", "z_node_1D"]                 # ... and the fields are the mesh's
    for p, w in zip(("VSV", "RHO"), want):
        assert np.array_equal(mesh.element_nodal_fields[p], w.reshape(gp.shape[:2])), p
    # the plain import reads other places: kilometres away in depth, up to 0.19 degrees in latitude
    plain = GllMesh(before.copy(), 2, {})
    api.import_regular_grid(grid, plain, outside="fill", fill_value=-1.0, context=ctx)
    assert not np.array_equal(plain.element_nodal_fields["VSV"], mesh.element_nodal_fields["VSV"])
    # it composes with in_frame: the identity frame changes nothing
    from multimesh_amd import frames
    assert np.array_equal(frames.in_frame(view, frames.Rotation.identity(), context=ctx).gll_points, pseudo)
    # a HexMesh: the same view, the nodal store shared
    points, conn = synth.hex_mesh(5, seed=4, lo=(6.2e6, -3e5, -3e5), hi=(6.371e6, 3e5, 3e5))
    hexmesh = HexMesh(points.copy(), conn)
    hview = G.as_geographic(hexmesh, wgs, context=ctx)
    assert type(hview) is HexMesh and hview.nodal_fields is hexmesh.nodal_fields and hview.connectivity is hexmesh.connectivity
    assert np.array_equal(hview.points, GC.to_geographic(WGS84, points)[0]) and np.array_equal(hexmesh.points, points)


def test_the_free_surface_of_an_elliptical_chunk_lies_on_the_equal_volume_ellipsoid(ctx):
    """The chunk's surface is ``r = R (1 + f (1/3 - c^2))``, c the cosine of the geocentric colatitude.  The ellipsoid of
    ``from_mean_radius`` has ``a = R (1 - f)^(-1/3) = R (1 + f/3 + 2 f^2/9 + ...)`` and, along the same direction, the radius
    ``a (1 + (2 f + 3 f^2 + ...) c^2)^(-1/2) = R (1 + f/3 - f c^2 + f^2 g(c^2) + O(f^3))`` with
    ``g(u) = 2/9 - 11 u/6 + 3 u^2/2``: the two surfaces differ radially by ``R f^2 |g|`` (20 to 24 m here) to second order,
    and the height, the distance along the normal, is no more than the radial distance.  The bound is that term per node
    plus ``4 R f^3`` (1 m) for the orders left out -- while ``6371000 - |p|``, the depth every tool reads without the view,
    is off by more than a kilometre at the same nodes."""
    chunk = _chunk()
    gp, z = chunk["points"], chunk["z_node_1D"]
    ell = G.Ellipsoid.from_mean_radius()
    surface = z == 1.0
    assert surface.sum() == 9 * 9 * 16 // 9                                                  # the top face of the 16 top elements
    lat, lon, h = G.geodetic_coordinates(gp, ell, context=ctx)
    r = np.linalg.norm(gp, axis=-1)
    u = (gp[..., 2] / r) ** 2
    g = 2.0 / 9.0 - 11.0 * u / 6.0 + 1.5 * u * u
    bound = GC.R_EARTH * F * F * np.abs(g) + 4.0 * GC.R_EARTH * F ** 3
    print(f"|height| at the surface {np.abs(h[surface]).min():.2f} .. {np.abs(h[surface]).max():.2f} m, bound "
          f"{bound[surface].min():.2f} .. {bound[surface].max():.2f} m; |6371000 - |p|| {np.abs(GC.R_EARTH - r[surface]).min():.0f} .. "
          f"{np.abs(GC.R_EARTH - r[surface]).max():.0f} m")
    assert (np.abs(h[surface]) <= bound[surface]).all() and bound[surface].max() < 26.0
    assert (np.abs(h[surface] + GC.R_EARTH * F * F * g[surface]) <= 4.0 * GC.R_EARTH * F ** 3).all()   # ... and it IS that term
    assert (np.abs(GC.R_EARTH - r[surface]) > 1000.0).all()
    geocentric = np.rad2deg(np.arcsin(gp[..., 2] / r))
    assert 0.15 < np.abs(lat - geocentric)[surface].max() < 0.2                              # degrees: up to 21 km on the ground


def test_depth_from_z_node_1d(ctx):
    """``depth="z_node_1D"``: the pseudo-point's radius is ``z_node_1D * 6371000``, bit for bit -- the view is the statement
    with exactly that product as ``radius_d``, coordinate by coordinate.  The norm of the three products
    ``((rho*cphi)*cl, (rho*cphi)*sl, rho*sphi)``, formed again, is ``rho`` only within rounding: four roundings in the
    coordinates and four in ``sqrt((x*x + y*y) + z*z)`` leave at most 2 ulp (measured: 2; 54 % of the nodes give ``rho``
    exactly), so the recomputed norm is held to that, and the exactness is asserted on the coordinates."""
    chunk = _chunk()
    gp, z = chunk["points"], chunk["z_node_1D"]
    mesh = GllMesh(gp, 2, {"z_node_1D": z})
    ell = G.Ellipsoid.from_mean_radius()
    view = G.as_geographic(mesh, ell, depth="z_node_1D", context=ctx)
    rho = z * 6371000.0
    want = GC.to_geographic(ell.constants(), gp, radius=rho)[0]
    assert np.array_equal(view.gll_points.view(np.uint64), want.view(np.uint64))
    norm = np.linalg.norm(view.gll_points, axis=-1)
    off = np.abs(norm - rho) / np.spacing(rho)
    print(f"|p'| against z_node_1D * 6371000: at most {off.max():.1f} ulp, {100.0 * (off == 0).mean():.0f} % exact")
    assert off.max() <= 2.0
    # only the direction comes from the ellipsoid: the other view has the same directions and other radii
    other = G.as_geographic(mesh, ell, context=ctx).gll_points
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    assert np.abs(unit(other) - unit(view.gll_points)).max() <= 8 * GC.EPS and np.abs(np.linalg.norm(other, axis=-1) - rho).max() > 1000.0
    assert view.element_nodal_fields is mesh.element_nodal_fields
    with pytest.raises(ValueError, match="z_node_1D"):
        G.as_geographic(GllMesh(gp, 2, {}), ell, depth="z_node_1D", context=ctx)


def test_extract_geographic_grid_against_the_geocentric_extraction(ctx):
    """A field that is linear in the GEODETIC latitude of the nodes (the NumPy statement on the host), extracted on geodetic
    axes, comes back as that function of the axis within the interpolation error of order-2 elements four degrees wide.  The
    control: a field linear in the GEOCENTRIC latitude through api.extract_regular_grid on geocentric axes.  Both errors are
    measured; the geographic one within twice the control says the POINTS are right (an error of 0.19 degrees in latitude
    would be 1.9 in the field: thousands of times the interpolation error)."""
    chunk = _chunk()
    gp = chunk["points"]
    ell = G.Ellipsoid.from_mean_radius()
    cphi, sphi, _, _ = GC.latitude_and_height(ell.constants(), gp[..., 0], gp[..., 1], gp[..., 2])
    geodetic = np.rad2deg(np.arctan2(sphi, cphi))
    geocentric = np.rad2deg(np.arcsin(gp[..., 2] / np.linalg.norm(gp, axis=-1)))
    mesh = GllMesh(gp, 2, {"GEODETIC": 3000.0 + 10.0 * geodetic, "GEOCENTRIC": 3000.0 + 10.0 * geocentric})
    lat, lon, depth = np.linspace(42.0, 54.0, 13), np.linspace(-6.0, 6.0, 7), np.linspace(20_000.0, 350_000.0, 5)
    grid = G.extract_geographic_grid(mesh, ["GEODETIC"], lat, lon, depth, ell, context=ctx)
    assert isinstance(grid, RegularGrid) and grid.nmissing == 0 and grid["GEODETIC"].shape == (5, 13, 7)
    assert np.array_equal(grid["latitude"], lat) and np.array_equal(grid["depth"], depth)
    error = np.abs(grid["GEODETIC"] - (3000.0 + 10.0 * lat)[None, :, None]).max()
    control_grid = api.extract_regular_grid(mesh, ["GEOCENTRIC", "GEODETIC"], (42.0, 54.0, 13), (-6.0, 6.0, 7),
                                            (20_000.0, 350_000.0, 5), context=ctx)
    control = np.abs(control_grid["GEOCENTRIC"] - (3000.0 + 10.0 * lat)[None, :, None]).max()
    crossed = np.abs(control_grid["GEODETIC"] - (3000.0 + 10.0 * lat)[None, :, None]).max()
    print(f"geographic extraction: error {error:.3g}; geocentric control: {control:.3g}; the geodetic field on geocentric axes: {crossed:.3g}")
    assert control_grid.nmissing == 0 and 0.0 < control < 0.1
    assert error <= 2.0 * control
    assert crossed > 1.0                                      # what the feature is for: geocentric axes read the field 0.19 degrees off
    # chunks of whole depth levels give the same grid; points outside the mesh are filled and counted
    chunked = G.extract_geographic_grid(mesh, ["GEODETIC"], lat, lon, depth, ell, chunk_points=2 * 13 * 7, context=ctx)
    assert np.array_equal(chunked["GEODETIC"], grid["GEODETIC"])
    outside = G.extract_geographic_grid(mesh, "GEODETIC", lat, [-6.0, 30.0], depth[:2], ell, fill_value=-1.0, context=ctx)
    assert outside.nmissing == 2 * 13 and (outside["GEODETIC"][:, :, 1] == -1.0).all() and (outside["GEODETIC"][:, :, 0] > 0).all()
