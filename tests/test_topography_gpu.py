"""mm_radial_stretch on the GPU against the NumPy statement of tests/topography_cases.py, and the drivers of
:mod:`multimesh_amd.topography` on meshes.

The device's acos and atan2 are the only part that cannot be bit for bit: the returned angles are compared with NumPy's
within 1e-11 degrees (the bound of tests/test_layered_gpu.py), r -- through the returned depth 6371000 - r -- bit for bit.
Everything after them -- the moved points, the radius and the count of outside nodes -- is compared bit for bit (NaN positions
compared, payloads not) by evaluating the statement on the angles the device returned.  The drivers' round trips are held to
ROUND_TRIP_BOUND of tests/test_topography.py, four times what the NumPy statement was measured to make."""
import numpy as np
import pytest

import topography_cases as TC
from multimesh_amd import api
from multimesh_amd import io as mio
from multimesh_amd import layered as LY
from multimesh_amd import synth
from multimesh_amd import topography as TP
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh
from test_topography import ROUND_TRIP_BOUND

pytestmark = pytest.mark.gpu

ANGLE_TOL = 1e-11               # degrees
CAP_LANES = 2048 * 256          # kMaxBlocks workgroups of 256 lanes: beyond, the workgroups stride
DIRECTIONS = {"apply": TC.APPLY, "flatten": TC.FLATTEN}
LATERALS = {"cell": TC.CELL, "bilinear": TC.BILINEAR}
OUTSIDES = {"keep": TC.KEEP, "clamp": TC.CLAMP}
R = TC.R_EARTH


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()      # before this module's context opens the device: torch then finds it whichever test runs first
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    with Context(0) as c:
        yield c


def _compare(got, pts, model, direction, lateral, outside, periodic, ref, start):
    """What the device returned (host arrays) against the statement on its own angles -> (points, radius, noutside)."""
    lat, lon, anchors, shifts = model
    flat = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(flat)
    lld = got["latlondepth"].reshape(n, 3)
    with np.errstate(all="ignore"):
        ref_lld, r = TC.device_view(flat, lon, periodic)
        finite = np.isfinite(flat).all(axis=1)
        dlon = np.abs(lld[finite, 1] - ref_lld[finite, 1])
        dlon = np.minimum(dlon, np.abs(dlon - 360.0))          # (a longitude within rounding of the wrap may land on either side)
        dlat = np.abs(lld[finite, 0] - ref_lld[finite, 0])
    assert n == 0 or not finite.any() or (dlat.max() <= ANGLE_TOL and dlon.max() <= ANGLE_TOL), (dlat.max(), dlon.max())
    assert TC.same_bits_nan(lld[finite, 2], R - r[finite])                                   # r, bit for bit
    want, radius, nout = TC.stretch(lld, r, flat, ref, lat, lon, anchors, shifts, DIRECTIONS[direction], LATERALS[lateral],
                                    OUTSIDES[outside])
    assert TC.same_bits_nan(got["radius"].reshape(n), radius), f"{(got['radius'].reshape(n) != radius).sum()} of {n} radii differ"
    assert TC.same_bits_nan(got["points"].reshape(n, 3), want)
    assert got["count"] == start + nout
    return want, radius, nout


def _check(ctx, pts, model, direction="apply", lateral="bilinear", outside="keep", periodic=False, ref=None, start=0, in_place=False):
    lat, lon, anchors, shifts = model
    host = np.ascontiguousarray(pts, dtype=np.float64)
    dev = ctx.to_device(host)
    count = ctx.to_device(np.array([start], dtype=np.int64))
    res = TP.radial_stretch(ctx, dev, lat, lon, anchors, shifts, lon_periodic=periodic, direction=direction, ref_radius=ref,
                            lateral=lateral, outside=outside, out=dev if in_place else None, want_radius=True,
                            want_latlondepth=True, noutside=count)
    assert (res["points"].ptr == dev.ptr) == in_place
    got = {k: a.numpy() for k, a in res.items()}
    got["count"] = int(count.numpy()[0])
    if not in_place:
        assert np.array_equal(dev.numpy().view(np.uint64), host.view(np.uint64))              # the input is left untouched
    return _compare(got, host, model, direction, lateral, outside, periodic, ref, start)


# ----------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_sizes_around_the_wave_and_the_workgroup(ctx, n):
    model = TC.regional(5, seed=n)
    for direction in DIRECTIONS:
        _, _, nout = _check(ctx, TC.cloud(n, model[2], seed=n), model, direction, start=7, in_place=n % 2 == 1)
        if n >= 63:
            assert 0 < nout < n


@pytest.mark.parametrize("direction", list(DIRECTIONS))
def test_past_the_launch_cap(ctx, direction):
    """More points than kMaxBlocks * 256 lanes: the stride loop runs (and its second step ends in a partial tile)."""
    n = CAP_LANES + 1000
    model = TC.regional(2, seed=3)
    _, _, nout = _check(ctx, TC.cloud(n, model[2], seed=1), model, direction, in_place=True)
    assert 0 < nout < n


@pytest.mark.parametrize("na", (2, 5, 64))
def test_anchor_counts(ctx, na):
    model = TC.regional(na, seed=na, spacing=3000.0)
    pts = TC.cloud(600, model[2], seed=na)
    for direction in DIRECTIONS:
        for lateral in LATERALS:
            _, radius, nout = _check(ctx, pts, model, direction, lateral)
            assert 0 < nout < 600 and (radius < model[2][-1]).any() and (radius > model[2][0]).any()


# ---------------------------------------------------------------------------------------------------------- combinations
@pytest.mark.parametrize("outside", list(OUTSIDES))
@pytest.mark.parametrize("lateral", list(LATERALS))
@pytest.mark.parametrize("direction", list(DIRECTIONS))
def test_modes_on_the_regional_and_the_periodic_map(ctx, direction, lateral, outside):
    model = TC.regional(5, seed=1)
    pts = TC.elements(40, 8, model[2], seed=5)
    _, _, nout = _check(ctx, pts, model, direction, lateral, outside, start=1234567)
    assert (0 < nout < 320) if outside == "keep" else nout == 0
    model = TC.global_map(5, seed=2)
    everywhere = TC.elements(40, 8, model[2], seed=6, lat=(-89.0, 89.0), lon=(-180.0, 180.0))
    _, radius, nout = _check(ctx, everywhere, model, direction, lateral, outside, periodic=True, in_place=True)
    assert nout == 0 and not np.array_equal(radius, TC.radius(everywhere))


@pytest.mark.parametrize("lateral", list(LATERALS))
def test_a_reference_radius(ctx, lateral):
    """ref_radius given: the node goes to the image of THAT radius along its own direction (a mesh with z_node_1D)."""
    model = TC.regional(5, seed=4)
    pts = TC.cloud(700, model[2], seed=8)
    rng = np.random.default_rng(2)
    ref = TC.radius(pts) + rng.uniform(-3000.0, 3000.0, 700)
    ref[:3] = [np.nan, model[2][0], model[2][-1]]
    for outside in OUTSIDES:
        want, radius, nout = _check(ctx, pts, model, "apply", lateral, outside, ref=ref, in_place=outside == "clamp")
        with_own, _, _ = _check(ctx, pts, model, "apply", lateral, outside)
        assert not TC.same_bits_nan(want, with_own) and (outside == "clamp" or 0 < nout < 700)
    with pytest.raises(ValueError, match="flattening computes it"):
        TP.radial_stretch(ctx, pts, *model, direction="flatten", ref_radius=ref)
    with pytest.raises(ValueError, match="one value per point"):
        TP.radial_stretch(ctx, pts, *model, ref_radius=ref[:-1])


def test_axes_of_length_one(ctx):
    lat, lon, anchors, shifts = TC.regional(5, seed=4)
    pts = TC.cloud(300, anchors, seed=2)
    for direction in DIRECTIONS:
        for outside in OUTSIDES:
            for lateral in LATERALS:
                _check(ctx, pts, (lat[3:4], lon, anchors, np.ascontiguousarray(shifts[3:4])), direction, lateral, outside)
                _check(ctx, pts, (lat, lon[4:5], anchors, np.ascontiguousarray(shifts[:, 4:5])), direction, lateral, outside)
                _, _, nout = _check(ctx, pts, (lat[:1], lon[:1], anchors, np.ascontiguousarray(shifts[:1, :1])), direction, lateral, outside)
                assert nout == 0                                      # an axis of length 1 is constant: every angle is on it


def test_axes_in_global_memory(ctx):
    """nlat + nlon > 2048: the axes are bisected in global memory."""
    lat, lon = np.array([-6.0, 0.0, 6.0]), np.linspace(-5.5, 6.5, 2050)
    model = TC.interface_tables(lat, lon, 3, seed=8)
    for direction in DIRECTIONS:
        for lateral in LATERALS:
            for outside in OUTSIDES:
                _, _, nout = _check(ctx, TC.cloud(300, model[2], seed=3), model, direction, lateral, outside, in_place=lateral == "cell")
                assert (0 < nout < 300) if outside == "keep" else nout == 0


# -------------------------------------------------------------------------------------------------------- special points
@pytest.mark.parametrize("lateral", list(LATERALS))
def test_special_points(ctx, lateral):
    lat, lon, anchors, shifts = TC.global_map(5, seed=3)
    r = anchors[1] - 700.0
    pts = TC.sphere_cloud(80, anchors, seed=4)
    pts[:12] = [[0, 0, r], [0, 0, -r], [0, 0, 0], [r, 0, 0], [-r, 0, 0], [-r, -0.0, 0], [0, r, 0], [0, -r, 0],
                [np.nan, 1.0, r], [np.inf, 0, r], [1.0, -np.inf, 2.0], [0, 0, np.inf]]
    pts[12:15] = TC.xyz(lat[2], [lon[3], lon[4], -180.0], 10000.0)            # on map nodes
    for direction in DIRECTIONS:
        for outside in OUTSIDES:
            want, radius, nout = _check(ctx, pts, (lat, lon, anchors, shifts), direction, lateral, outside, periodic=True, start=3)
            assert nout >= 2 and np.array_equal(want[2], [0.0, 0.0, 0.0]) and np.isnan(want[8, 0]) and want[8, 1] == 1.0
            assert radius[2] == 0.0 and np.isnan(radius[8]) and np.isfinite(want[[0, 1, 3, 4, 5, 6, 7]]).all()
    # the regional map: on its edge, just outside it, on a map node
    lat, lon, anchors, shifts = TC.regional(5, seed=3)
    eps = 1e-9
    edge = TC.xyz([lat[0], lat[0] - eps, lat[-1], lat[-1] + eps, 0.0, 0.0, 0.0, 0.0, lat[2]],
                  [0.0, 0.0, 0.0, 0.0, lon[0], lon[0] - eps, lon[-1], lon[-1] + eps, lon[3]], 9000.0)
    for direction in DIRECTIONS:
        for outside in OUTSIDES:
            _check(ctx, np.concatenate([edge, TC.cloud(60, anchors, seed=5)]), (lat, lon, anchors, shifts), direction, lateral, outside)


@pytest.mark.parametrize("lateral", list(LATERALS))
def test_nodes_on_the_anchors_and_on_the_interfaces(ctx, lateral):
    """Nodes at the north pole, where r = z exactly and the column is the map's last row: exactly on every anchor A_j, exactly
    on every deformed anchor B_j, above the top and below the bottom, one ulp to either side of each."""
    lat, lon = np.array([80.0, 90.0]), np.array([-180.0, 0.0, 180.0])
    anchors = TC.anchor_radii(5)
    s = np.array([300.0, -250.0, 120.0, 0.0, -400.0])
    shifts = np.ascontiguousarray(np.broadcast_to(s, (2, 3, 5)))
    B = anchors + s
    radii = np.concatenate([anchors, B, np.nextafter(anchors, 0.0), np.nextafter(anchors, np.inf), np.nextafter(B, 0.0),
                            np.nextafter(B, np.inf), [anchors[0] + 5000.0, anchors[-1] - 5000.0, B[0] + 1.0, B[-1] - 1.0]])
    pts = np.zeros((radii.size, 3))
    pts[:, 2] = radii
    _, moved, nout = _check(ctx, pts, (lat, lon, anchors, shifts), "apply", lateral, periodic=True)
    assert nout == 0 and np.array_equal(moved[:5], B)                                  # anchors land on their interfaces
    assert moved[-4] == anchors[0] + 5000.0 + s[0] and moved[-3] == anchors[-1] - 5000.0 + s[-1]
    _, flat, nout = _check(ctx, pts, (lat, lon, anchors, shifts), "flatten", lateral, periodic=True, in_place=True)
    assert nout == 0 and np.array_equal(flat[6:10], anchors[1:]) and abs(flat[5] - anchors[0]) <= np.spacing(anchors[0])
    assert flat[-2] == (B[0] + 1.0) - s[0] and flat[-1] == (B[-1] - 1.0) - s[-1]


def test_a_zero_shift_map_keeps_the_bits(ctx):
    lat, lon, anchors, shifts = TC.global_map(5, seed=1)
    pts = TC.sphere_cloud(1000, anchors, seed=2)
    for lateral in LATERALS:
        want, _, nout = _check(ctx, pts, (lat, lon, anchors, np.zeros_like(shifts)), "apply", lateral, periodic=True, in_place=True)
        assert nout == 0 and np.array_equal(want.view(np.uint64), pts.view(np.uint64))


def test_outside_nodes_keep_their_bits(ctx):
    """Rows off the map hold NaN payloads, infinities, negative zeros and subnormals: they come back bit for bit, in place and
    out of place, and the count starts from a non-zero value and is taken once."""
    model = TC.regional(5, seed=9)
    pts = TC.cloud(500, model[2], seed=9)
    odd = (np.arange(30 * 3, dtype=np.uint64).reshape(30, 3) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(0x7FF0000000000000)
    pts[:30] = odd.view(np.float64)                                                   # NaN and infinities: r is a NaN or lat is
    pts[30:33] = [[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [1.5e-310, 0.0, 0.0]]         # the centre twice; a subnormal on the x axis
    for in_place in (False, True):
        dev = ctx.to_device(pts)
        count = ctx.to_device(np.array([41], dtype=np.int64))
        res = TP.radial_stretch(ctx, dev, *model, out=dev if in_place else None, want_radius=True, want_latlondepth=True, noutside=count)
        got, lld = res["points"].numpy(), res["latlondepth"].numpy()
        _, radius, nout = TC.stretch(lld, TC.radius(pts), pts, None, *model)
        moved = got.view(np.uint64) != pts.view(np.uint64)
        valid = (lld[:, 0] >= -6.0) & (lld[:, 0] <= 6.0) & (lld[:, 1] >= -5.5) & (lld[:, 1] <= 6.5) & (TC.radius(pts) > 0.0)
        assert not valid[:33].any() and nout == (~valid).sum() and 33 < nout < 500 and int(count.numpy()[0]) == 41 + nout
        assert not moved[~valid].any() and moved[valid].any(axis=1).all()
        assert TC.same_bits_nan(res["radius"].numpy(), radius)


def test_nothing_to_do_is_valid(ctx):
    model = TC.regional(5)
    res = TP.radial_stretch(ctx, np.zeros((0, 3)), *model, want_radius=True)
    assert res["points"].shape == (0, 3) and res["radius"].shape == (0,)
    res = TP.radial_stretch(ctx, np.ones((4, 5, 3)), *model, want_points=False, want_radius=True, want_latlondepth=True)
    assert "points" not in res and res["radius"].shape == (4, 5) and res["latlondepth"].shape == (4, 5, 3)
    with pytest.raises(ValueError, match="shifts must be"):
        TP.radial_stretch(ctx, np.zeros((4, 3)), model[0], model[1], model[2], model[3][:, :4])
    with pytest.raises(ValueError, match="anchors must be"):
        TP.radial_stretch(ctx, np.zeros((4, 3)), model[0], model[1], model[2][:1], model[3][..., :1])
    with pytest.raises(ValueError, match="ascending"):
        TP.radial_stretch(ctx, np.zeros((4, 3)), model[0][::-1], model[1], model[2], model[3])
    with pytest.raises(ValueError, match="as many values"):
        TP.radial_stretch(ctx, np.zeros((4, 3)), *model, out=ctx.empty((3, 3), np.float64))


# ------------------------------------------------------------------------------- a caller's stream and caller's tensors
def test_on_a_callers_stream_with_the_callers_tensors_off_alignment(torch):
    """Late producer, early consumer, as tests/test_caller_stream_gpu.py: under a side stream the inputs hold zeros while the
    stream spins, the true values are copied in on that stream, the library is called and its outputs are cloned and
    overwritten right after, with no host synchronisation in between.  Points, reference radii, axes, anchors, shifts and
    outputs are views that start 8 bytes into their buffers (off 16-byte alignment), as in tests/test_caller_views_gpu.py."""
    lat, lon, anchors, shifts = TC.regional(5, seed=12)
    pts = TC.elements(40, 27, anchors, seed=12).reshape(-1, 3)
    n = len(pts)
    ref = TC.radius(pts) + 25.0
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    host = (pts, ref, lat, lon, anchors, shifts)
    staged = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in host]
    torch.cuda.synchronize()

    def view(shape, dtype, fill):
        buffer = torch.full((int(np.prod(shape)) + 1,), fill, dtype=dtype, device="cuda")
        v = buffer[1:].view(tuple(shape))
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v

    with Context(0, stream=side.cuda_stream) as ctx, torch.cuda.stream(side):
        tp, tr, tla, tlo, ta, ts = (view(x.shape, torch.float64, 0.0) for x in host)
        tout = view(pts.shape, torch.float64, -3.0)
        count = view((1,), torch.int64, 10)
        torch.cuda._sleep(30_000_000)
        for t, s in zip((tp, tr, tla, tlo, ta, ts), staged):
            t.copy_(s, non_blocking=True)
        res = TP.radial_stretch(ctx, tp, tla, tlo, ta, ts, ref_radius=tr, out=tout, want_radius=True, want_latlondepth=True,
                                noutside=count)
        assert res["points"].ptr == tout.data_ptr()
        got = {"points": tout.clone(), "count": count.clone()}
        extra = {k: res[k] for k in ("radius", "latlondepth")}
        tout.fill_(-7.0), count.fill_(-7)
        side.synchronize()
        got = {"points": got["points"].cpu().numpy(), "count": int(got["count"].item()), **{k: a.numpy() for k, a in extra.items()}}
    _, _, nout = _compare(got, pts, (lat, lon, anchors, shifts), "apply", "bilinear", "keep", False, ref, 10)
    assert 0 < nout < n


# ----------------------------------------------------------------------------------------------------------- the drivers
MOHO_DEPTH = 24400.0


def _chunk(order=2):
    """A chunk on its 1-D sphere whose element faces honour the surface and a Moho at 24.4 km."""
    return synth.earth_chunk(order=order, nlat=3, nlon=3, lat=(-5.0, 5.0), lon=(-5.0, 5.0),
                             radii=(6_311_000.0, R - MOHO_DEPTH, R), nrad=(1, 1))


def _crust(seed=20):
    """A layered model, given north to south, with a surface (interface 0) and a Moho (interface 3) that undulate by some
    kilometres, and a flat bottom far below."""
    rng = np.random.default_rng(seed)
    lat, lon = TC.REGIONAL_LAT, TC.REGIONAL_LON
    top = rng.uniform(-2500.0, 1500.0, (7, 9))
    moho = rng.uniform(20000.0, 30000.0, (7, 9))
    bounds = np.stack([top, top + 2000.0, top + 9000.0, moho, np.full((7, 9), 90000.0)])
    return LY.LayeredModel(lat[::-1], lon, bounds[:, ::-1], {})


def _imap(model):
    return TP.InterfaceMap.from_layered(model, {0: 0.0, 3: MOHO_DEPTH}, taper_radius=6_251_000.0)


def test_apply_then_remove_on_a_gll_mesh_a_hex_mesh_and_a_salvus_file(ctx):
    imap = _imap(_crust())
    gp = _chunk()["points"]
    # copies of shared GLL nodes are bit-equal before ...
    _, first, inverse = np.unique(gp.reshape(-1, 3).view(np.uint64), axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    assert len(first) < gp.size // 3
    mesh = GllMesh(gp.copy(), 2, {"VS": np.ones(gp.shape[:2])})
    assert TP.apply_topography(mesh, imap, reference="radius", context=ctx) == 0
    moved = mesh.gll_points.copy()
    flat = moved.reshape(-1, 3).view(np.uint64)
    assert np.array_equal(flat, flat[first][inverse])                                 # ... and after
    dr = TC.radius(moved) - TC.radius(gp)
    assert dr.max() > 1000.0 and dr.min() < -1000.0 and np.array_equal(mesh.element_nodal_fields["VS"], np.ones(gp.shape[:2]))
    lld = TP.radial_stretch(ctx, gp, imap.lat, imap.lon, imap.anchors, imap.packed(), want_points=False, want_latlondepth=True)["latlondepth"]
    want, _, _ = TC.stretch(lld.numpy(), TC.radius(gp), gp, None, imap.lat, imap.lon, imap.anchors, imap.packed())
    assert TC.same_bits_nan(moved.reshape(-1, 3), want)
    assert TP.remove_topography(mesh, imap, context=ctx) == 0
    worst = np.abs(mesh.gll_points - gp).max()
    print(f"GLL mesh, there and back: {worst:.4g} m")
    assert worst <= ROUND_TRIP_BOUND and not np.array_equal(mesh.gll_points, moved)
    back = mesh.gll_points.reshape(-1, 3).view(np.uint64)
    assert np.array_equal(back, back[first][inverse])
    # with z_node_1D as the reference: the same image, whatever radius the node has now
    squashed = GllMesh(gp * 0.999, 2, {"z_node_1D": _chunk()["z_node_1D"]})
    assert TP.apply_topography(squashed, imap, context=ctx) == 0
    assert np.abs(squashed.gll_points - moved).max() <= ROUND_TRIP_BOUND
    # a hex mesh: nodal points [N, 3], some of them off the map
    points, conn = synth.hex_mesh(6, seed=1, lo=(6.26e6, -8e5, -8e5), hi=(6.371e6, 8e5, 8e5))
    hexmesh = HexMesh(points.copy(), conn)
    nout = TP.apply_topography(hexmesh, imap, reference="radius", context=ctx)
    assert 0 < nout < len(points) and TP.remove_topography(hexmesh, imap, context=ctx) == nout
    assert np.abs(hexmesh.points - points).max() <= ROUND_TRIP_BOUND and not np.array_equal(hexmesh.points, points)
    assert TP.apply_topography(HexMesh(points.copy(), conn), imap, reference="radius", outside="clamp", context=ctx) == 0
    # a Salvus file in memory: MODEL/coordinates are assigned, MODEL/data is untouched
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=gp)
    data = np.ascontiguousarray(np.stack([_chunk()["z_node_1D"], np.ones(gp.shape[:2])]).transpose(1, 0, 2))
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=data), ["z_node_1D", "VS"])
    assert TP.apply_topography(f, imap, context=ctx) == 0                             # (its z_node_1D column is the reference)
    assert np.abs(np.array(f["MODEL/coordinates"][()]) - moved).max() <= ROUND_TRIP_BOUND
    assert TP.remove_topography(f, imap, context=ctx) == 0
    assert np.abs(np.array(f["MODEL/coordinates"][()]) - gp).max() <= ROUND_TRIP_BOUND
    assert np.array_equal(np.array(f["MODEL/data"][()]), data)


def test_attach_z_node_1d_then_map_to_sphere(ctx):
    """A mesh that arrives with its topography applied and without z_node_1D: attach_z_node_1d computes the field and
    api.map_to_sphere then puts every surface node back at 6 371 000 m."""
    imap = _imap(_crust(seed=21))
    chunk = _chunk()
    gp, z = chunk["points"], chunk["z_node_1D"]
    mesh = GllMesh(gp.copy(), 2, {})
    TP.apply_topography(mesh, imap, reference="radius", context=ctx)
    with pytest.raises(ValueError, match="no z_node_1D"):
        api.map_to_sphere(mesh, context=ctx)
    rho = TP.reference_radius(mesh, imap, context=ctx)
    assert rho.shape == gp.shape[:2] and np.abs(rho - z * R).max() <= ROUND_TRIP_BOUND
    assert TP.attach_z_node_1d(mesh, imap, context=ctx) is mesh
    assert np.array_equal(mesh.element_nodal_fields["z_node_1D"], rho / R)
    api.map_to_sphere(mesh, context=ctx)
    surface = z == 1.0
    assert surface.sum() >= 9 * 9
    worst = np.abs(TC.radius(mesh.gll_points[surface]) - R).max()
    print(f"surface nodes after map_to_sphere: {worst:.4g} m off 6371000")
    assert worst <= ROUND_TRIP_BOUND and np.abs(mesh.gll_points - gp).max() <= ROUND_TRIP_BOUND
    # a hex mesh gets a nodal field, a Salvus file its column
    points, conn = synth.hex_mesh(5, seed=2, lo=(6.3e6, -3e5, -3e5), hi=(6.371e6, 3e5, 3e5))
    hexmesh = TP.attach_z_node_1d(HexMesh(points, conn), imap, context=ctx)
    assert np.array_equal(hexmesh.nodal_fields["z_node_1D"], TP.reference_radius(points, imap, context=ctx) / R)
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=gp)
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=np.zeros((gp.shape[0], 1, gp.shape[1]))), ["z_node_1D"])
    TP.attach_z_node_1d(f, imap, context=ctx)
    assert np.array_equal(np.array(f["MODEL/data"][()])[:, 0, :], TP.reference_radius(gp, imap, context=ctx) / R)


def test_a_mesh_follows_the_moho_of_a_layered_model(ctx):
    """apply_topography with InterfaceMap.from_layered, then layered.layer_index(pick="node"): the nodes that sat on the 1-D
    Moho radius now sit on the model's Moho -- the bottom of layer 2 or the top of layer 3 at their column."""
    model = _crust(seed=22)
    chunk = _chunk()
    on_moho = chunk["z_node_1D"] == (R - MOHO_DEPTH) / R
    on_surface = chunk["z_node_1D"] == 1.0
    assert on_moho.sum() >= 2 * 9 * 9 and on_surface.sum() >= 9 * 9
    mesh = GllMesh(chunk["points"].copy(), 2, {"z_node_1D": chunk["z_node_1D"]})
    assert TP.apply_topography(mesh, _imap(model), context=ctx) == 0
    layer, span = LY.layer_index(model, mesh, pick="node", context=ctx)
    depth = R - TC.radius(mesh.gll_points).reshape(layer.shape)
    assert set(layer[on_moho]) <= {2, 3} and set(layer[on_surface]) <= {-1, 0}
    moho = np.where(layer == 2, span[..., 1], span[..., 0])
    worst = np.abs(depth[on_moho] - moho[on_moho]).max()
    print(f"nodes of the 1-D Moho against the model's Moho: {worst:.4g} m")
    assert worst <= ROUND_TRIP_BOUND and np.abs(moho[on_moho] - MOHO_DEPTH).max() > 1000.0
    on_top = on_surface & (layer == 0)
    assert np.abs(depth[on_top] - span[on_top][:, 0]).max() <= ROUND_TRIP_BOUND
