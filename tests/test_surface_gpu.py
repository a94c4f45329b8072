"""mm_boundary_triangles, mm_surface_distance and multimesh_amd.surface on the GPU, bit for bit against the NumPy statements
of tests/surface_cases.py (a brute-force minimum over every triangle: no grid there).  Every point is compared, none is
left out.  The raw clouds are built to break a pruning rule of the ring walk, not to look like meshes."""
import numpy as np
import pytest

import boundary_cases as BC
import surface_cases as SC
from multimesh_amd import boundary, surface, synth
from multimesh_amd import device as _device
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

CHUNK = dict(order=2, nlat=3, nlon=3, nrad=(1, 2), topography=3e-4, ellipticity=3.35e-3)
UP = (0.0, 0.0, 1.0)
INF = np.inf


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()      # before this module's context opens the device: torch then finds it whichever test runs first
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    with Context(0) as c:
        yield c


def _statement_boundary(gp, order, up):
    corners = np.ascontiguousarray(gp[:, BC.corner_nodes(order)])
    faces, _ = BC.boundary_faces(BC.corner_ids(corners)[0])
    return faces, BC.classify(corners, faces, up=up)


def _triangles(ctx, gp, order, faces, side, mask):
    """mm_boundary_triangles on host arrays -> f64[T, 3, 3] (NumPy)"""
    pts, fd = ctx.to_device(gp), ctx.to_device(np.asarray(faces, np.int64))
    sd = None if side is None else ctx.to_device(np.asarray(side, np.int32))
    out = ctx.empty((len(faces) * 2 * order * order, 3, 3), np.float64)
    T = _device._call(surface.bind(ctx.lib), "mm_boundary_triangles", ctx.handle, pts, len(gp), order, fd, sd, len(faces),
                      mask, out, arg_error=True)
    return out.rows(0, T).numpy()


def _check(ctx, pts, tri, cutoffs):
    """every cutoff against the statement; returns the statement's unbounded distance"""
    least, _ = SC.surface_distance(pts, tri, INF)
    for cutoff in cutoffs:
        ref, ref_count = SC.with_cutoff(least, cutoff)
        d, count = surface.distance_to_triangles(pts, tri, cutoff, context=ctx)
        assert d.shape == np.shape(pts)[:-1] and count == ref_count, (cutoff, count, ref_count)
        got = d.numpy().reshape(-1)
        assert SC.same_bits(got, ref), (cutoff, int((got != ref).sum()), np.flatnonzero(got != ref)[:5])
    return least


def _outside_cloud(lo, hi, n, seed):
    """seeded points reaching 1.5 box sizes outside [lo, hi]"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    return lo + (np.random.default_rng(seed).uniform(-1.5, 2.5, (n, 3))) * (hi - lo)


# -------------------------------------------------------------------------------------------------------- triangles
@pytest.mark.parametrize("order", [1, 2, 4])
def test_triangles_of_gll_meshes(ctx, order):
    gp = synth.gll_mesh(4, order)
    faces, side = _statement_boundary(gp, order, UP)
    for mask in (0, 2, 5, 7):
        ref = SC.boundary_triangles(gp, order, faces, side, mask)
        assert SC.same_bits(_triangles(ctx, gp, order, faces, side, mask), ref), (order, mask)
    assert len(ref) == 54 * 2 * order * order
    assert SC.same_bits(_triangles(ctx, gp, order, faces, None, 0), ref)             # no sides: every face
    assert _triangles(ctx, gp, order, faces[:0], side[:0], 7).shape == (0, 3, 3)     # nb == 0
    with pytest.raises(ValueError, match="code outside"):
        _triangles(ctx, gp, order, np.array([0, 6 * len(gp)]), None, 7)
    with pytest.raises(ValueError, match="side outside"):
        _triangles(ctx, gp, order, faces[:2], np.array([0, 3]), 7)


def test_triangles_of_a_chunk_and_a_hexmesh_through_the_module(ctx):
    chunk = synth.earth_chunk(**CHUNK)["points"]
    faces, side = _statement_boundary(chunk, 2, None)
    bnd = boundary.mesh_boundary(GllMesh(chunk, 2), context=ctx)
    for sides, mask in ((("side", "bottom"), 5), ("top", 2), (("side", "top", "bottom"), 7), ((), 0)):
        tri = surface.boundary_triangles(bnd, sides)
        assert tri.ctx is ctx and SC.same_bits(tri.numpy(), SC.boundary_triangles(chunk, 2, faces, side, mask)), mask
    pts, conn = synth.hex_mesh(4)
    tensor = conn[:, BC.EXODUS_TO_TENSOR]
    h = boundary.mesh_boundary(HexMesh(pts, conn), up=UP, context=ctx)
    faces, _ = BC.boundary_faces(tensor)
    side = BC.classify(pts[tensor], faces, up=UP)
    assert SC.same_bits(surface.boundary_triangles(h).numpy(), SC.boundary_triangles(pts[tensor], 1, faces, side, 5))


# ----------------------------------------------------------------------------------------------- distance on meshes
def _mesh_case(kind):
    if kind == "chunk":
        gp, order, up = synth.earth_chunk(**CHUNK)["points"], 2, None
        width = min(np.linalg.norm(gp[-1, p] - gp[-1, 0]) for p in (2, 6, 18))       # the least edge of an element
    else:
        order = int(kind[-1])
        gp, up = synth.gll_mesh(4 if order < 4 else 3, order, seed=2), UP
        width = 1.0 / (3 if order < 4 else 2)
    return gp, order, up, width


@pytest.mark.parametrize("kind", ["cube1", "cube2", "cube4", "chunk"])
def test_distance_of_a_mesh_and_a_cloud_to_its_boundary_surface(ctx, kind):
    gp, order, up, width = _mesh_case(kind)
    faces, side = _statement_boundary(gp, order, up)
    tri = SC.boundary_triangles(gp, order, faces, side, 0b101)
    flat = gp.reshape(-1, 3)
    pts = np.concatenate([flat, _outside_cloud(flat.min(axis=0), flat.max(axis=0), 2000, seed=order)])
    least = _check(ctx, pts, tri, [0.3 * width, width, 3 * width, 10 * width, INF])
    nodes = np.unique(BC.boundary_nodes(gp, order, faces, side, 0b101), axis=0)
    on_boundary = (flat[:, None, :] == nodes[None, :, :]).all(axis=2).any(axis=1)
    d = surface.distance_to_triangles(flat, tri, context=ctx)[0].numpy()
    assert on_boundary.sum() >= len(nodes) and (d[on_boundary] == 0.0).all() and not np.signbit(d[on_boundary]).any()
    assert (least[:len(flat)][~on_boundary] > 0.0).any()


# ------------------------------------------------------------------------ clouds built to break a pruning rule
def _random_triangles(rng, n, lo, hi, size):
    a = rng.uniform(lo, hi, (n, 1, 3))
    return a + np.concatenate([np.zeros((n, 1, 3)), rng.uniform(-size, size, (n, 2, 3))], axis=1)


def test_a_graded_mesh_whose_nearest_triangle_lies_rings_away(ctx):
    gp = synth.gll_mesh(6, 1, jitter=0.0) ** 2                                       # u -> u^2 per axis: elements 1/25 .. 9/25 wide
    faces, side = _statement_boundary(gp, 1, UP)
    tri = SC.boundary_triangles(gp, 1, faces, side, 7)
    pts = np.concatenate([gp.reshape(-1, 3), _outside_cloud([0, 0, 0], [1, 1, 1], 2000, seed=7),
                          np.random.default_rng(8).uniform(0.0, 1.0, (1500, 3))])
    least = _check(ctx, pts, tri, [0.03, 0.2, INF])
    assert least.max() > 1.5 and (least > 0.2).sum() > 100


@pytest.mark.parametrize("sheet", [False, True])
def test_small_triangles_whose_grid_is_enlarged_to_its_caps(ctx, sheet):
    """triangles of size 2^-13 in the unit box: cells of their size would pass the caps of the grid -- 2^22 cells in all in
    3-D, 1024 per axis on a sheet --, so the edge is enlarged before the entries are counted"""
    rng = np.random.default_rng(41)
    tri = _random_triangles(rng, 300, 0.0, 1.0, 2.0 ** -14)
    if sheet:
        tri[:, :, 2] = 0.5
    corners = tri.reshape(-1, 3)
    near = corners[rng.integers(0, 900, 500)] + rng.uniform(-1e-4, 1e-4, (500, 3))   # within 2e-4 of a vertex
    pts = np.concatenate([corners, near, rng.uniform(0.0, 1.0, (2000, 3))])
    least = _check(ctx, pts, tri, [3e-4, 0.2, INF])
    assert (least < 3e-4).sum() >= 1400                                              # (else the least cutoff checks nothing)


def test_one_face_fifty_times_larger_than_the_others(ctx):
    rng = np.random.default_rng(21)
    small = _random_triangles(rng, 400, 0.0, 1.0, 0.02)                              # 200 faces' worth
    o, u, v = np.array([0.0, 0.0, -0.5]), np.array([1.0, 0.0, 0.6]), np.array([0.0, 1.0, 0.6])    # a tilted unit quad
    big = np.array([[o, o + u, o + u + v], [o, o + u + v, o + v]])
    tri = np.concatenate([small[:200], big, small[200:]])
    pts = np.concatenate([rng.uniform(-0.3, 1.3, (3000, 3)), _outside_cloud([0, 0, -0.5], [1, 1, 1], 500, seed=22)])
    _check(ctx, pts, tri, [0.01, 0.15, INF])
    _check(ctx, pts, tri[rng.permutation(len(tri))], [0.15])                         # the set alone defines the result


def test_few_coplanar_and_degenerate_triangles(ctx):
    rng = np.random.default_rng(31)
    pts = rng.uniform(-1.0, 2.0, (2000, 3))
    one = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, 0.5]]])
    pts[:3] = one[0]                                                                 # on the vertices
    assert (_check(ctx, pts, one, [0.4, INF])[:3] == 0.0).all()                      # T = 1
    two = np.concatenate([one, one + 0.125])
    _check(ctx, pts, two, [0.4, INF])                                                # T = 2 in one cell
    flat = _random_triangles(rng, 300, 0.0, 1.0, 0.1)
    flat[:, :, 2] = 0.25                                                             # a sheet: no extent on one axis
    _check(ctx, pts, flat, [0.05, 0.5, INF])
    mixed = _random_triangles(rng, 200, 0.0, 1.0, 0.1)
    mixed[50, 1] = mixed[50, 0]                                                      # a = b
    mixed[51, 2] = mixed[51, 1]                                                      # b = c
    mixed[52] = mixed[52, 0]                                                         # a point
    _check(ctx, pts, mixed, [0.05, INF])
    points_only = np.repeat(rng.uniform(0.0, 1.0, (5, 1, 3)), 3, axis=1)             # every triangle a point; the box of one too
    _check(ctx, pts, points_only, [0.3, INF])
    _check(ctx, pts, points_only[:1], [0.3, INF])


def test_points_on_cell_faces_far_points_and_a_nan(ctx):
    """coordinates on a binary lattice: the cell edge is a power of two and the box starts on the lattice, so lattice points
    lie exactly on cell faces; points beyond the cutoff from the box, far points and points that are not finite beside them"""
    rng = np.random.default_rng(41)
    tri = rng.integers(0, 33, (300, 1, 3)) / 16.0 + rng.integers(-2, 3, (300, 3, 3)) / 16.0
    tri[0, 0] = [0.0, 0.0, 0.0]
    lattice = np.stack(np.meshgrid(*[np.arange(-8, 49) / 16.0] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[::7]
    far = rng.uniform(-1.0, 1.0, (60, 3)) * 10.0 ** rng.integers(1, 12, (60, 1))
    odd = np.zeros((6, 3))
    odd[0, 0], odd[1, 1], odd[2], odd[3, 2], odd[4, 0] = np.nan, np.nan, np.nan, np.inf, -np.inf
    odd[5] = [1e200, -1e200, 1e200]                                                  # the squares overflow: r = inf
    pts = np.concatenate([lattice, far, odd])
    for cutoff in (0.07, 0.5, 4.0):
        d, _ = surface.distance_to_triangles(pts, tri, cutoff, context=ctx)
        assert (d.numpy()[-6:] == cutoff).all()
    least = _check(ctx, pts, tri, [0.07, 0.5, 4.0, INF])
    assert (least[-6:] == INF).all() and np.isfinite(least[:-6]).all()


def test_metre_scale_triangles_at_earth_scale_coordinates(ctx):
    """a cloud offset by 6e6 from the origin: the stopping bound's absolute margin is what keeps it exact there"""
    rng = np.random.default_rng(51)
    offset = np.array([6.0e6, -6.0e6, 6.0e6])
    tri = _random_triangles(rng, 500, 0.0, 40.0, 1.5) + offset
    pts = rng.uniform(-20.0, 60.0, (4000, 3)) + offset
    pts[:20] = tri[:20, 1]
    least = _check(ctx, pts, tri, [0.5, 5.0, 50.0, INF])
    assert (least[:20] == 0.0).all()


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing_and_the_next_call_is_served(ctx):
    rng = np.random.default_rng(61)
    tri, pts = _random_triangles(rng, 50, 0.0, 1.0, 0.2), rng.uniform(0.0, 1.0, (100, 3))
    lib = surface.bind(ctx.lib)
    pts_d, dist = ctx.to_device(pts), ctx.to_device(np.full(100, 77.0))
    for bad in (np.nan, np.inf, -np.inf):
        wrong = tri.copy()
        wrong[17, 2, 1] = bad
        rc = lib.mm_surface_distance(ctx.handle, pts_d.ptr, 100, ctx.to_device(wrong).ptr, 50, 0.5, dist.ptr)
        assert rc == -1 and b"mm_surface_distance: 1 triangle vertices are not finite" in lib.mm_last_error()
        with pytest.raises(ValueError, match="not finite"):
            surface.distance_to_triangles(pts, wrong, 0.5, context=ctx)
    tri_d = ctx.to_device(tri)
    for cutoff in (0.0, -1.0, np.nan, 1e-200):
        assert lib.mm_surface_distance(ctx.handle, pts_d.ptr, 100, tri_d.ptr, 50, cutoff, dist.ptr) == -1
        with pytest.raises(ValueError, match="cutoff"):
            surface.distance_to_triangles(pts, tri, cutoff, context=ctx)
    assert (dist.numpy() == 77.0).all()                                              # nothing was written
    _check(ctx, pts, tri, [0.1, INF])                                                # the next call is served
    for cutoff in (0.25, INF):                                                       # T == 0
        d, count = surface.distance_to_triangles(pts, np.zeros((0, 3, 3)), cutoff, context=ctx)
        assert count == 0 and (d.numpy() == cutoff).all()
    d, count = surface.distance_to_triangles(np.zeros((0, 3)), tri, 0.25, context=ctx)   # n == 0
    assert count == 0 and d.shape == (0,)
    with pytest.raises(ValueError, match=r"\[T, 3, 3\]"):
        surface.distance_to_triangles(pts, tri.reshape(-1, 3), context=ctx)


# ---------------------------------------------------------------------------------------------------- Python layer
def test_depth_below_the_mesh_s_own_surface(ctx):
    chunk = synth.earth_chunk(**CHUNK)["points"]
    faces, side = _statement_boundary(chunk, 2, None)
    mesh = GllMesh(chunk, 2)
    depth = surface.depth_below_surface(mesh, context=ctx)
    ref, _ = SC.surface_distance(chunk, SC.boundary_triangles(chunk, 2, faces, side, 0b010), INF)
    assert depth.shape == chunk.shape[:2] and SC.same_bits(depth.reshape(-1), ref)
    radial = synth.R_EARTH - np.linalg.norm(chunk, axis=2)
    assert np.abs(depth - radial).max() > 1000.0                                     # topography and ellipticity: kilometres
    bnd = boundary.mesh_boundary(mesh, context=ctx)
    assert SC.same_bits(surface.depth_below_surface(mesh, boundary=bnd), depth)
    assert SC.same_bits(surface.distance_to_surface(mesh, bnd, None, sides="top", context=ctx), depth)
    # a chunk of a sphere: its surface nodes are at depth 0 by both measures, within the slack of the statement at |p| = R
    from test_surface import SLACK
    plain = synth.earth_chunk(order=2, nlat=3, nlon=3, nrad=(1, 2))["points"]
    d = surface.depth_below_surface(GllMesh(plain, 2), context=ctx)
    faces, side = _statement_boundary(plain, 2, None)
    top = np.unique(BC.boundary_nodes(plain, 2, faces, side, 0b010), axis=0)
    at_top = (plain.reshape(-1, 1, 3) == top[None]).all(axis=2).any(axis=1)
    radial = (synth.R_EARTH - np.linalg.norm(plain, axis=2)).reshape(-1)
    assert at_top.sum() >= len(top) and (np.abs(d.reshape(-1)[at_top] - radial[at_top]) <= SLACK * synth.R_EARTH).all()
    assert (d.reshape(-1)[at_top] == 0.0).all()


def test_taper_to_surface(ctx):
    gp = synth.gll_mesh(4, 2, seed=2)
    faces, side = _statement_boundary(gp, 2, UP)
    rng = np.random.default_rng(1)
    fields = {"K": rng.normal(size=gp.shape[:2]), "L": rng.normal(size=gp.shape[:2])}
    mesh = GllMesh(gp, 2, fields)
    bnd = boundary.mesh_boundary(mesh, up=UP, context=ctx)
    inner, outer = 0.05, 0.3
    values, ntapered = surface.taper_to_surface(mesh, ["K", "L"], inner, outer, boundary=bnd, context=ctx)
    tri = SC.boundary_triangles(gp, 2, faces, side, 0b101)
    d, _ = SC.surface_distance(gp, tri, outer)
    stacked = np.stack([fields["K"], fields["L"]])
    ref, w, ref_count = BC.distance_taper(d, inner, outer, stacked)
    assert values.shape == stacked.shape and ntapered == ref_count and SC.same_bits(values.reshape(2, -1), ref)
    assert SC.same_bits(surface.distance_to_surface(mesh, bnd, outer, context=ctx).reshape(-1), d)
    nodes = np.unique(BC.boundary_nodes(gp, 2, faces, side, 0b101), axis=0)
    on_boundary = (gp.reshape(-1, 1, 3) == nodes[None]).all(axis=2).any(axis=1)
    assert on_boundary.sum() > 0 and (values.reshape(2, -1)[:, on_boundary] == 0.0).all()       # exactly 0 on the boundary
    beyond = d >= outer
    assert beyond.sum() > 0 and SC.same_bits(values.reshape(2, -1)[:, beyond], stacked.reshape(2, -1)[:, beyond])
    assert SC.same_bits(mesh.element_nodal_fields["K"], fields["K"])                            # the mesh is untouched
    with Context(0) as other:
        with pytest.raises(ValueError, match="another context"):
            surface.distance_to_surface(mesh, bnd, outer, context=other)
        with pytest.raises(ValueError, match="another context"):
            surface.taper_to_surface(mesh, "K", inner, outer, boundary=bnd, context=other)


def test_blend_models_by_the_surface_distance(ctx):
    host_pts = synth.earth_chunk(order=2, nlat=6, nlon=6, lat=(-12.0, 12.0), lon=(-12.0, 12.0),
                                 radii=(5_771_000.0, 6_171_000.0, synth.R_EARTH), nrad=(2, 1))["points"]
    reg_pts = synth.earth_chunk(order=4, nlat=3, nlon=3, lat=(-6.0, 6.0), lon=(-6.0, 6.0))["points"]
    f_host = 1.0 + 1e-7 * host_pts[..., 0] + 2e-7 * host_pts[..., 1]
    f_reg = 5.0 - 3e-7 * reg_pts[..., 2] + 1e-7 * reg_pts[..., 1]
    host, regional = GllMesh(host_pts, 2, {"VP": f_host}), GllMesh(reg_pts, 4, {"VP": f_reg})
    inner, outer = 50e3, 250e3
    values, info = surface.blend_models(regional, host, "VP", inner, outer, context=ctx)
    uniq, inv = ctx.unique_points(host_pts.reshape(-1, 3), ordered=False)
    vals, elem, _, _ = ctx.interpolate_gll(4, reg_pts, uniq, f_reg[None], want_operator=True)
    inverse = inv.numpy()
    a, el = vals.numpy()[inverse].T, elem.numpy()[inverse]
    faces, side = _statement_boundary(reg_pts, 4, None)
    d, _ = SC.surface_distance(uniq.numpy(), SC.boundary_triangles(reg_pts, 4, faces, side, 0b101), outer)
    ref, w, _ = BC.distance_taper(d[inverse], inner, outer, a, b=f_host.reshape(1, -1), elem=el)
    assert values.shape == (1,) + f_host.shape and SC.same_bits(values.reshape(1, -1), ref)
    assert info == {"nlocated": int((el >= 0).sum()), "nblended": int(((w > 0) & (w < 1)).sum()),
                    "nreplaced": int((w == 1).sum())}
    assert info["nblended"] > 0 and info["nreplaced"] > 0
    by_nodes, _ = boundary.blend_models(regional, host, "VP", inner, outer, context=ctx)
    assert not SC.same_bits(by_nodes, values)                                        # the two distances differ


# ---------------------------------------------------------------------------------------------------- caller arrays
@pytest.mark.parametrize("misaligned", [False, True])
def test_caller_tensors_off_sixteen_bytes(torch, ctx, misaligned):
    from test_caller_views_gpu import SENTINEL, Buffers
    rng = np.random.default_rng(71)
    gp = synth.gll_mesh(3, 2)
    faces, side = _statement_boundary(gp, 2, UP)
    pts = np.concatenate([gp.reshape(-1, 3), rng.uniform(-0.5, 1.5, (301, 3))])
    ref_tri = SC.boundary_triangles(gp, 2, faces, side, 0b101)
    bufs = Buffers(torch, misaligned)
    gp_t, faces_t, side_t = bufs.view(gp.shape, np.float64, gp), bufs.view(faces.shape, np.int64, faces), \
        bufs.view(side.shape, np.int32, side)
    tri_t = bufs.view((len(faces) * 8, 3, 3), np.float64)
    pts_t, dist_t = bufs.view(pts.shape, np.float64, pts), bufs.view((len(pts),), np.float64)
    torch.cuda.synchronize()
    lib = surface.bind(ctx.lib)
    T = lib.mm_boundary_triangles(ctx.handle, gp_t.data_ptr(), len(gp), 2, faces_t.data_ptr(), side_t.data_ptr(), len(faces), 5,
                                  tri_t.data_ptr())
    assert T == len(ref_tri)
    tri_np = tri_t.cpu().numpy()
    assert SC.same_bits(tri_np[:T], ref_tri) and (tri_np[T:] == SENTINEL).all()
    ref, ref_count = SC.surface_distance(pts, ref_tri, 0.2)
    count = lib.mm_surface_distance(ctx.handle, pts_t.data_ptr(), len(pts), tri_t.data_ptr(), T, 0.2, dist_t.data_ptr())
    assert count == ref_count and SC.same_bits(dist_t.cpu().numpy(), ref)
    d, count = surface.distance_to_triangles(pts_t, tri_t[:T], 0.2, context=ctx)      # tensors through the module
    assert count == ref_count and SC.same_bits(d.numpy(), ref)
    bufs.check_borders("surface")
