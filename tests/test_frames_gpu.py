"""mm_rotate_points, mm_rotate_vectors and mm_local_components on the GPU against the NumPy statement of
tests/frames_cases.py, bit for bit (NaN positions compared, payloads not: they are the processor's), and the Python layer
of :mod:`multimesh_amd.frames` on meshes: rotate_mesh, in_frame with the regular-grid import, local_components."""
import numpy as np
import pytest

import frames_cases as FC
from multimesh_amd import api, synth
from multimesh_amd import frames as F
from multimesh_amd.api import GllMesh, RegularGrid
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

CAP_LANES = 8192 * 256          # the launch cap of the three kernels: beyond, the workgroups stride


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()      # before this module's context opens the device: torch then finds it whichever test runs first
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    with Context(0) as c:
        yield c


def _points_with_specials(n, seed):
    pts = FC.cloud(n, seed=seed)
    special = FC.special_rows()
    k = min(n, len(special))
    pts[:k] = special[:k]
    return pts


# ------------------------------------------------------------------------------------------------------ mm_rotate_points
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_rotate_points_around_the_wave_and_the_workgroup(ctx, n):
    """Both transposes, out of place and in place; the first rows hold NaN, +-inf, -0.0 and denormals."""
    R = FC.matrix(n)
    pts = _points_with_specials(n, seed=n)
    for transpose in (False, True):
        want = FC.rotate_points(R, pts, transpose)
        src = ctx.to_device(pts)
        out = F.rotate_points(ctx, src, R, transpose=transpose)
        assert out.ptr != src.ptr and out.shape == (n, 3)
        assert FC.same_bits_nan(out.numpy(), want)
        assert np.array_equal(src.numpy().view(np.uint64), pts.view(np.uint64))             # the input is untouched
        same = F.rotate_points(ctx, src, R, transpose=transpose, out=src)
        assert same.ptr == src.ptr and FC.same_bits_nan(src.numpy(), want)
    if n >= 63:
        assert not np.array_equal(FC.rotate_points(R, pts[12:]), FC.rotate_points(R, pts[12:], True))


def test_rotate_points_past_the_launch_cap(ctx):
    """One point more than 8192 * 256 lanes: the stride loop runs, and its second step is one lane."""
    n = CAP_LANES + 1
    R = FC.matrix(77)
    pts = FC.cloud(n, seed=77)
    src = ctx.to_device(pts)
    want = FC.rotate_points(R, pts)
    assert np.array_equal(F.rotate_points(ctx, src, R).numpy(), want)
    F.rotate_points(ctx, src, R, transpose=True, out=src)
    assert np.array_equal(src.numpy(), FC.rotate_points(R, pts, True))


def test_rotate_points_keeps_the_element_nodal_shape_and_refuses_partial_overlap(ctx):
    R = FC.matrix(5)
    pts = FC.cloud(4 * 27, seed=5).reshape(4, 27, 3)
    out = F.rotate_points(ctx, pts, R)
    assert out.shape == (4, 27, 3) and np.array_equal(out.numpy(), FC.rotate_points(R, pts))
    buf = ctx.to_device(np.zeros((101, 3)))
    with pytest.raises(ValueError, match="overlaps"):
        F.rotate_points(ctx, buf.rows(0, 100), R, out=buf.rows(1, 101))
    with pytest.raises(ValueError, match="not finite"):
        F.rotate_points(ctx, buf, np.where(np.eye(3) > 0, np.inf, 0.0))
    with pytest.raises(ValueError, match="3-D"):
        F.rotate_points(ctx, np.zeros((5, 2)), R)
    with pytest.raises(ValueError, match="as many values"):
        F.rotate_points(ctx, buf, R, out=ctx.empty((50, 3), np.float64))


def test_rotate_points_on_a_callers_stream_with_the_callers_tensors_off_alignment(torch):
    """Late producer, early consumer, as tests/test_caller_stream_gpu.py: under a side stream the input holds zeros while the
    stream spins, the true values are copied in on that stream, the library is called and its output is cloned and
    overwritten right after, with no host synchronisation in between.  Input and output are views that start 8 bytes into
    their buffers (off 16-byte alignment), as in tests/test_caller_views_gpu.py."""
    R = FC.matrix(9)
    pts = _points_with_specials(1000, seed=9)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    staged = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()

    def view(fill):
        buffer = torch.full((pts.size + 1,), fill, dtype=torch.float64, device="cuda")
        v = buffer[1:].view(pts.shape)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v

    with Context(0, stream=side.cuda_stream) as ctx, torch.cuda.stream(side):
        tin, tout, tsame = view(0.0), view(-7.0), view(0.0)
        torch.cuda._sleep(30_000_000)
        tin.copy_(staged, non_blocking=True), tsame.copy_(staged, non_blocking=True)
        res = F.rotate_points(ctx, tin, R, out=tout)
        assert res.ptr == tout.data_ptr()
        F.Rotation(R).apply(tsame, out=tsame, backwards=True, context=ctx)
        got, got_same = tout.clone(), tsame.clone()
        tout.fill_(-7.0), tsame.fill_(-7.0), tin.fill_(-7.0)
        side.synchronize()
        got, got_same = got.cpu().numpy(), got_same.cpu().numpy()
    assert FC.same_bits_nan(got, FC.rotate_points(R, pts))
    assert FC.same_bits_nan(got_same, FC.rotate_points(R, pts, True))


# ----------------------------------------------------------------------------------------------------- mm_rotate_vectors
def _plane_layout(a, E, P):
    return (a, P, E * P, (0, 1, 2))


@pytest.mark.parametrize("P", (1, 27, 125))
@pytest.mark.parametrize("E", (0, 1, 3))
def test_rotate_vectors_on_planes_and_on_rows(ctx, E, P):
    R = FC.matrix(10 * E + P)
    v = FC.vectors((E, P), seed=P + E)
    if E:
        v[:, 0, 0] = FC.special_rows()[E]
    for transpose in (False, True):
        want = FC.rotate_vectors(R, v, transpose)
        # field planes [3][E][P], out of place and in place
        src = ctx.to_device(v)
        dst = ctx.to_device(np.full(v.shape, -7.0))
        F.rotate_vectors_on_device(ctx, R, E, P, _plane_layout(src, E, P), _plane_layout(dst, E, P), transpose=transpose)
        assert FC.same_bits_nan(dst.numpy(), want)
        F.rotate_vectors_on_device(ctx, R, E, P, _plane_layout(src, E, P), _plane_layout(src, E, P), transpose=transpose)
        assert FC.same_bits_nan(src.numpy(), want)
        # MODEL/data rows [E][5][P] with permuted columns: into other rows with other columns, then in place
        cols, ocols = (3, 0, 2), (1, 4, 0)
        rows = FC.rows_of(v, 5, cols, seed=P)
        src = ctx.to_device(rows)
        before = np.full((E, 6, P), -7.0)
        dst = ctx.to_device(before)
        F.rotate_vectors_on_device(ctx, R, E, P, (src, 5 * P, P, cols), (dst, 6 * P, P, ocols), transpose=transpose)
        got = dst.numpy()
        assert FC.same_bits_nan(got[:, ocols, :].transpose(1, 0, 2), want)
        assert (got[:, [2, 3, 5], :] == -7.0).all()                                         # the other columns are untouched
        F.rotate_vectors_on_device(ctx, R, E, P, (src, 5 * P, P, cols), (src, 5 * P, P, cols), transpose=transpose)
        got = src.numpy()
        assert FC.same_bits_nan(got[:, cols, :].transpose(1, 0, 2), want)
        assert np.array_equal(got[:, [1, 4], :], rows[:, [1, 4], :])
        # ... in place with the columns permuted on the way out
        src = ctx.to_device(rows)
        F.rotate_vectors_on_device(ctx, R, E, P, (src, 5 * P, P, cols), (src, 5 * P, P, (2, 3, 0)), transpose=transpose)
        assert FC.same_bits_nan(src.numpy()[:, (2, 3, 0), :].transpose(1, 0, 2), want)


def test_apply_to_vectors(ctx):
    rot = F.Rotation(FC.matrix(21))
    v = FC.vectors((7, 27), seed=21)
    want = FC.rotate_vectors(rot.matrix, v)
    got = rot.apply_to_vectors(v, context=ctx)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert np.array_equal(rot.apply_to_vectors(v.reshape(3, -1), backwards=True, context=ctx), FC.rotate_vectors(rot.matrix, v.reshape(3, -1), True))
    dev = ctx.to_device(v)
    same = rot.apply_to_vectors(dev, out=dev, context=ctx)
    assert same.ptr == dev.ptr and np.array_equal(dev.numpy(), want)
    rows = FC.rows_of(v, 4, (3, 1, 0), seed=2)
    got = rot.apply_to_vectors(rows, columns=(3, 1, 0), context=ctx)
    assert np.array_equal(got[:, (3, 1, 0), :].transpose(1, 0, 2), want) and np.array_equal(got[:, 2, :], rows[:, 2, :])
    with pytest.raises(ValueError, match=r"\[3, \.\.\.\]"):
        rot.apply_to_vectors(np.zeros((2, 5)), context=ctx)
    with pytest.raises(ValueError, match="columns must be three"):
        rot.apply_to_vectors(rows, columns=(0, 1, 4), context=ctx)
    with pytest.raises(ValueError, match="the layout reaches"):
        F.rotate_vectors_on_device(ctx, rot.matrix, 7, 27, (dev, 27, 7 * 27, (0, 1, 3)), (dev, 27, 7 * 27, (0, 1, 2)))


# --------------------------------------------------------------------------------------------------- mm_local_components
@pytest.mark.parametrize("basis", ("rtp", "zne"))
@pytest.mark.parametrize("inverse", (False, True))
def test_local_components(ctx, inverse, basis):
    """Generic positions with, at their head, both poles (s = 0), the centre (r = 0) and NaN coordinates; planes with
    P = 27 (two groups straddle a wave) and a flat cloud (P = 1); out of place and in place."""
    direction, basis_id = (FC.TO_CARTESIAN if inverse else FC.TO_LOCAL), F.BASIS[basis]
    special = FC.special_positions()
    for shape in ((11, 27), (300,)):
        n = int(np.prod(shape))
        pos = FC.cloud(n, seed=n)
        pos[:len(special)] = special
        pos = pos.reshape(shape + (3,))
        v = FC.vectors(shape, seed=n)
        want = FC.local_components(pos, v, direction, basis_id)
        assert np.isnan(want[0].reshape(-1)[3]) and np.isfinite(want[:, :3].reshape(3, -1)[:, :3]).all()
        got = F.local_components(pos, v, basis=basis, inverse=inverse, context=ctx)
        assert isinstance(got, np.ndarray) and FC.same_bits_nan(got, want)
        dev, dpos = ctx.to_device(v), ctx.to_device(pos)
        same = F.local_components(dpos, dev, basis=basis, inverse=inverse, out=dev, context=ctx)
        assert same.ptr == dev.ptr and FC.same_bits_nan(dev.numpy(), want)
        assert np.array_equal(dpos.numpy().view(np.uint64), pos.view(np.uint64))


def test_local_components_on_rows_past_the_launch_cap_and_on_a_mesh(ctx):
    # MODEL/data rows with permuted columns
    E, P = 3, 125
    pos = FC.cloud(E * P, seed=31).reshape(E, P, 3)
    v = FC.vectors((E, P), seed=31)
    rows = FC.rows_of(v, 5, (4, 1, 2), seed=31)
    src, dst = ctx.to_device(rows), ctx.to_device(np.full((E, 3, P), -7.0))
    F.local_components_on_device(ctx, ctx.to_device(pos), E, P, (src, 5 * P, P, (4, 1, 2)), (dst, 3 * P, P, (2, 0, 1)), basis="zne")
    assert FC.same_bits_nan(dst.numpy()[:, (2, 0, 1), :].transpose(1, 0, 2), FC.local_components(pos, v, FC.TO_LOCAL, FC.ZNE))
    # one node past the launch cap
    n = CAP_LANES + 1
    pos, v = FC.cloud(n, seed=32), FC.vectors((n,), seed=32)
    assert np.array_equal(F.local_components(pos, v, context=ctx), FC.local_components(pos, v))
    # the fields of a mesh by name
    gp = synth.earth_chunk(order=2, nlat=2, nlon=2)["points"]
    fields = dict(zip(("UX", "UY", "UZ"), FC.vectors(gp.shape[:2], seed=33)))
    mesh = GllMesh(gp, 2, fields)
    got = F.local_components(mesh, ["UX", "UY", "UZ"], basis="zne", context=ctx)
    assert got.shape == (3,) + gp.shape[:2]
    assert np.array_equal(got, FC.local_components(gp, np.stack([fields[k] for k in ("UX", "UY", "UZ")]), FC.TO_LOCAL, FC.ZNE))
    with pytest.raises(ValueError, match="over the positions"):
        F.local_components(gp, np.zeros((3, 5)), context=ctx)
    with pytest.raises(ValueError, match="points overlap out"):
        buf = ctx.to_device(np.zeros((3, 100)))
        F.local_components_on_device(ctx, buf.reshape(100, 3), 100, 1, (ctx.to_device(np.zeros((3, 100))), 1, 100, (0, 1, 2)),
                                     (buf, 1, 100, (0, 1, 2)))


# ---------------------------------------------------------------------------------------------------------------- meshes
def _chunk(order=2):
    return synth.earth_chunk(order=order, nlat=3, nlon=3, lat=(-6.0, 6.0), lon=(-6.0, 6.0),
                             radii=(6_171_000.0, 6_271_000.0, 6_371_000.0), nrad=(1, 1))["points"]


def test_rotate_mesh(ctx):
    rot = F.Rotation.to_north_pole(35.0, -120.0)
    gp = _chunk()
    mesh = GllMesh(gp.copy(), 2, {"VS": np.ones(gp.shape[:2])})
    assert F.rotate_mesh(mesh, rot, context=ctx) is mesh
    assert np.array_equal(mesh.gll_points, FC.rotate_points(rot.matrix, gp)) and not np.array_equal(mesh.gll_points, gp)
    assert np.array_equal(mesh.element_nodal_fields["VS"], np.ones(gp.shape[:2]))
    forward = mesh.gll_points.copy()
    F.rotate_mesh(mesh, rot, backwards=True, context=ctx)
    assert np.array_equal(mesh.gll_points, FC.rotate_points(rot.matrix, forward, transpose=True))
    assert np.abs(mesh.gll_points - gp).max() < 1e-8 and not np.array_equal(mesh.gll_points, gp)      # there and back: not the same bits
    points, conn = synth.hex_mesh(5, seed=2, lo=(6.2e6, -2e5, -2e5), hi=(6.371e6, 2e5, 2e5))
    hexmesh = HexMesh(points.copy(), conn)
    F.rotate_mesh(hexmesh, rot, backwards=True, context=ctx)
    assert np.array_equal(hexmesh.points, FC.rotate_points(rot.matrix, points, transpose=True))

    class Salvus:                      # a Salvus mesh object: points and whatever else
        pass

    salvus = Salvus()
    salvus.points = gp.copy()
    salvus.points.setflags(write=False)                 # points that cannot be assigned in place are replaced
    F.rotate_mesh(salvus, rot, context=ctx)
    assert np.array_equal(salvus.points, FC.rotate_points(rot.matrix, gp))


def _cube(seed=3):
    rng = np.random.default_rng(seed)
    depth, lat, lon = np.linspace(-30_000.0, 260_000.0, 7), np.linspace(-12.0, 12.0, 9), np.linspace(-13.0, 13.0, 10)
    return RegularGrid(depth, lat, lon, {"VSV": rng.uniform(3000.0, 5000.0, (7, 9, 10)), "RHO": rng.uniform(2500.0, 3500.0, (7, 9, 10))})


def test_in_frame_with_the_regular_grid_import(ctx):
    """A chunk that lies around (lat 40, lon 25) and a cube given around (0, 0) in the frame in which that place is the
    origin of latitude and longitude: the import through in_frame is the cube sampled at the host-rotated points."""
    grid = _cube()
    to_pole = F.Rotation.to_north_pole(40.0, 25.0)
    pole_to_origin = F.Rotation.from_axis_angle([0.0, 1.0, 0.0], 90.0)                     # the pole to (lat 0, lon 0)
    rot = pole_to_origin @ to_pole
    gp = FC.rotate_points(rot.matrix, _chunk(), transpose=True)                             # the chunk, placed at the event
    before = gp.copy()
    mesh = GllMesh(gp, 2, {"QMU": np.full(gp.shape[:2], 600.0)})
    view = F.in_frame(mesh, rot, context=ctx)
    assert type(view) is GllMesh and view is not mesh and view.element_nodal_fields is mesh.element_nodal_fields
    rotated = FC.rotate_points(rot.matrix, before)
    assert np.array_equal(view.gll_points, rotated) and view.gll_points is not mesh.gll_points
    missed = api.import_regular_grid(grid, view, outside="fill", fill_value=-1.0, context=ctx)
    want, nout = api.sample_regular_grid(grid, rotated.reshape(-1, 3), outside="fill", fill_value=-1.0, context=ctx)
    assert missed == nout == 0
    assert np.array_equal(mesh.gll_points.view(np.uint64), before.view(np.uint64))          # the caller's coordinates: unchanged
    assert sorted(mesh.element_nodal_fields) == ["QMU", "RHO", "VSV"]                       # ... and the fields are the mesh's
    for p, w in zip(("VSV", "RHO"), want):
        assert np.array_equal(mesh.element_nodal_fields[p], w.reshape(gp.shape[:2])), p
    # in the mesh's own frame the cube does not reach the chunk at all
    own, nown = api.sample_regular_grid(grid, before.reshape(-1, 3), outside="fill", fill_value=-1.0, context=ctx)
    assert nown == before.size // 3 and (own == -1.0).all()
    # the identity reproduces a plain import
    plain, framed = GllMesh(rotated, 2, {}), GllMesh(rotated, 2, {})
    api.import_regular_grid(grid, plain, outside="fill", context=ctx)
    api.import_regular_grid(grid, F.in_frame(framed, F.Rotation.identity(), context=ctx), outside="fill", context=ctx)
    for p in ("VSV", "RHO"):
        assert np.array_equal(framed.element_nodal_fields[p], plain.element_nodal_fields[p])
        assert np.array_equal(plain.element_nodal_fields[p], mesh.element_nodal_fields[p])
    # a HexMesh: nodal fields land in the original's store
    points, conn = synth.hex_mesh(5, seed=4, lo=(6.2e6, -3e5, -3e5), hi=(6.371e6, 3e5, 3e5))
    placed = FC.rotate_points(to_pole.inverse().matrix @ pole_to_origin.inverse().matrix, points)
    hexmesh = HexMesh(placed.copy(), conn)
    hview = F.in_frame(hexmesh, rot, context=ctx)
    assert type(hview) is HexMesh and hview.nodal_fields is hexmesh.nodal_fields and hview.connectivity is hexmesh.connectivity
    api.import_regular_grid(grid, hview, parameters=["VSV"], outside="fill", context=ctx)
    want, _ = api.sample_regular_grid(grid, FC.rotate_points(rot.matrix, placed), parameters=["VSV"], context=ctx)
    assert np.array_equal(hexmesh.nodal_fields["VSV"], want[0]) and np.isfinite(want).all()
    assert np.array_equal(hexmesh.points, placed)
