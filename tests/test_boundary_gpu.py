"""mm_boundary_faces, mm_boundary_classify, mm_boundary_nodes, mm_cutoff_distance, mm_distance_taper and
multimesh_amd.boundary on the GPU, bit for bit against the NumPy statements of tests/boundary_cases.py (np.unique over
every face key, a brute-force minimum over every source: no table and no grid there)."""
import numpy as np
import pytest

import boundary_cases as BC
from multimesh_amd import boundary, synth
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

CHUNK = dict(order=2, nlat=3, nlon=3, nrad=(1, 2), ellipticity=0.0033, topography=3e-4)
UP = (0.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def cube():
    """gll_mesh(5, 4): 64 elements; its statement-side boundary (faces, side with up = z, every boundary node)"""
    gp = synth.gll_mesh(5, 4, seed=2)
    corners = gp[:, BC.corner_nodes(4)]
    faces, _ = BC.boundary_faces(BC.corner_ids(corners)[0])
    side = BC.classify(corners, faces, up=UP)
    return gp, faces, side, BC.boundary_nodes(gp, 4, faces, side, 7)


def _check_mesh(ctx, gp, order, up):
    """faces, sides and nodes of a GLL mesh through the Context methods against the statements; returns the statement's"""
    corners = np.ascontiguousarray(gp[:, BC.corner_nodes(order)])
    ids, nnodes = BC.corner_ids(corners)
    ref_faces, ref_nonmanifold = BC.boundary_faces(ids)
    faces, nonmanifold = ctx.boundary_faces(ids, nnodes)
    assert nonmanifold == ref_nonmanifold and np.array_equal(faces.numpy(), ref_faces)
    ref_side = BC.classify(corners, ref_faces, up=up)
    side = ctx.boundary_classify(corners, faces, up=up)
    assert side.numpy().dtype == np.int32 and np.array_equal(side.numpy(), ref_side)
    for mask in range(8):
        ref = BC.boundary_nodes(gp, order, ref_faces, ref_side, mask)
        got = ctx.boundary_nodes(gp, order, faces, side, mask).numpy()
        assert BC.same_bits(got, ref), (order, mask)
    assert BC.same_bits(ctx.boundary_nodes(gp, order, faces).numpy(), BC.boundary_nodes(gp, order, ref_faces, ref_side, 7))
    return ref_faces, ref_side


# ------------------------------------------------------------------------------------------- faces, sides, nodes
@pytest.mark.parametrize("order", [1, 2, 4])
def test_faces_sides_and_nodes_of_gll_meshes(ctx, order):
    gp = synth.gll_mesh(4, order)
    faces, side = _check_mesh(ctx, gp, order, UP)
    assert len(faces) == 54 and np.bincount(side, minlength=3).tolist() == [36, 9, 9]
    faces_h, _ = _check_mesh(ctx, BC.holed(gp), order, UP)
    assert len(faces_h) == 60
    perm = np.random.default_rng(order).permutation(len(gp))
    faces_p, side_p = _check_mesh(ctx, np.ascontiguousarray(gp[perm]), order, UP)
    back = perm[faces_p // 6] * 6 + faces_p % 6
    assert np.array_equal(np.sort(back), faces) and np.array_equal(side_p[np.argsort(back)], side)
    one, _ = _check_mesh(ctx, gp[:1], order, UP)
    assert one.tolist() == [0, 1, 2, 3, 4, 5]
    two, _ = _check_mesh(ctx, np.ascontiguousarray(gp[[0, 26]]), order, UP)          # two elements that do not touch
    assert len(two) == 12


def test_mesh_boundary_of_the_three_kinds_of_mesh(ctx):
    chunk = synth.earth_chunk(**CHUNK)["points"]
    b = boundary.mesh_boundary(GllMesh(chunk, 2), context=ctx)                       # radial up
    corners = chunk[:, BC.corner_nodes(2)]
    ref_faces, _ = BC.boundary_faces(BC.corner_ids(corners)[0])
    ref_side = BC.classify(corners, ref_faces)
    assert np.array_equal(b.element * 6 + b.face, ref_faces) and np.array_equal(b.side, ref_side) and b.nonmanifold == 0
    assert (b.count("side"), b.count("top"), b.count("bottom")) == (36, 9, 9) and len(b) == 54
    assert BC.same_bits(b.nodes(), BC.boundary_nodes(chunk, 2, ref_faces, ref_side, 0b101))
    assert BC.same_bits(b.nodes(sides="top"), BC.boundary_nodes(chunk, 2, ref_faces, ref_side, 0b010))
    pts, conn = synth.hex_mesh(4)
    h = boundary.mesh_boundary(HexMesh(pts, conn), up=UP, context=ctx)
    tensor = conn[:, BC.EXODUS_TO_TENSOR]
    ref_faces, _ = BC.boundary_faces(tensor)
    ref_side = BC.classify(pts[tensor], ref_faces, up=UP)
    assert np.array_equal(h.element * 6 + h.face, ref_faces) and np.array_equal(h.side, ref_side)
    assert (h.count("side"), h.count("top"), h.count("bottom")) == (36, 9, 9)
    assert BC.same_bits(h.nodes(("side", "top", "bottom")), BC.boundary_nodes(pts[tensor], 1, ref_faces, ref_side, 7))


def test_a_shared_face_too_many_warns(ctx):
    ids = np.array([np.arange(8), np.arange(8) + 8, np.arange(8) + 16])
    ids[1, BC.FACE_CORNERS[0]] = ids[0, BC.FACE_CORNERS[1]]
    ids[2, BC.FACE_CORNERS[2]] = ids[0, BC.FACE_CORNERS[1]]
    faces, nonmanifold = ctx.boundary_faces(ids, 24)
    ref_faces, ref_nonmanifold = BC.boundary_faces(ids)
    assert nonmanifold == ref_nonmanifold == 3 and np.array_equal(faces.numpy(), ref_faces)
    gp = synth.gll_mesh(2, 1)
    with pytest.warns(UserWarning, match="not a manifold"):
        b = boundary.mesh_boundary(GllMesh(np.concatenate([gp, gp, gp]), 1), up=UP, context=ctx)
    assert b.nonmanifold == 18 and len(b) == 0


def test_an_id_out_of_range_is_refused_and_the_next_call_served(ctx):
    ids, nnodes = BC.corner_ids(synth.gll_mesh(3, 1))
    for bad in (nnodes, -1, 1 << 40):
        wrong = ids.copy()
        wrong[5, 3] = bad
        faces_d = ctx.to_device(np.full(6 * len(ids), 77, np.int64))
        rc = ctx.lib.mm_boundary_faces(ctx.handle, ctx.to_device(wrong).ptr, len(ids), nnodes, faces_d.ptr, None)
        assert rc == -1 and b"mm_boundary_faces: 3 faces have a corner id outside" in ctx.lib.mm_last_error()
        assert (faces_d.numpy() == 77).all()                                         # nothing is written
        with pytest.raises(ValueError, match="corner id outside"):
            ctx.boundary_faces(wrong, nnodes)
    faces, _ = ctx.boundary_faces(ids, nnodes)
    assert np.array_equal(faces.numpy(), BC.boundary_faces(ids)[0])
    corners = synth.gll_mesh(3, 1)
    with pytest.raises(ValueError, match="face codes outside"):
        ctx.boundary_classify(corners, np.array([0, 6 * len(ids)]), up=UP)
    with pytest.raises(ValueError, match="code outside"):
        ctx.boundary_nodes(corners, 1, np.array([-1, 3]))
    with pytest.raises(ValueError, match="side outside"):
        ctx.boundary_nodes(corners, 1, np.array([0, 3]), np.array([0, 3], np.int32))
    assert ctx.boundary_faces(np.zeros((0, 8), np.int64), 0)[0].shape == (0,)


# -------------------------------------------------------------------------------------------------- cutoff_distance
def _check_distance(ctx, pts, src, cutoff):
    ref, ref_count = BC.cutoff_distance(pts, src, cutoff)
    d, count = ctx.cutoff_distance(pts, src, cutoff)
    assert d.shape == np.shape(pts)[:-1] and count == ref_count
    assert BC.same_bits(d.numpy().reshape(-1), ref), (np.shape(pts), np.shape(src), cutoff)
    return ref


@pytest.mark.parametrize("widths", [0.3, 1.0, 3.0])
def test_distance_of_a_mesh_to_its_own_boundary(ctx, cube, widths):
    gp, _, _, nodes = cube
    ref = _check_distance(ctx, gp, nodes, widths * 0.25)                             # (an element is 0.25 wide)
    assert ref.min() == 0.0 and (ref.max() == widths * 0.25) == (widths < 2)          # the middle is 2 elements deep


def _clouds():
    """3001 sources in the unit box and 5003 targets around it, corner cases among the first 65"""
    rng = np.random.default_rng(11)
    src = rng.uniform(0.0, 1.0, (3001, 3))
    pts = rng.uniform(-0.5, 1.5, (5003, 3))                                          # a cloud larger than the box
    pts[:50] = rng.uniform(-1.0, 1.0, (50, 3)) * 1e9                                 # ... and targets far outside
    pts[50:60] = src[:10]                                                            # ... and on sources
    pts[60, 0], pts[61, 1], pts[62] = np.nan, np.nan, np.nan
    pts[63, 2], pts[64, 0] = np.inf, -np.inf
    return src, pts


def test_distance_of_clouds_and_corner_cases(ctx):
    src, pts = _clouds()
    for cutoff in (0.01, 0.06, 0.7, 50.0):                                           # (0.01: 101 cells per axis, no cap yet)
        ref = _check_distance(ctx, pts, src, cutoff)
        assert (ref[60:65] == cutoff).all() and (ref[50:60] == 0.0).all()
    _check_distance(ctx, pts, src[:1], 0.5)                                          # K = 1
    d, count = ctx.cutoff_distance(pts, np.zeros((0, 3)), 0.25)                      # K = 0
    assert count == 0 and (d.numpy() == 0.25).all()
    assert ctx.cutoff_distance(np.zeros((0, 3)), src, 0.25)[1] == 0                  # n = 0
    plane = src.copy()
    plane[:, 2] = 0.5                                                                # a sheet: no extent on one axis
    _check_distance(ctx, pts, plane, 0.1)
    wrong = src.copy()
    wrong[17, 1] = np.nan
    with pytest.raises(ValueError, match="1 sources are not finite"):
        ctx.cutoff_distance(pts, wrong, 0.1)
    _check_distance(ctx, pts[:100], src, 0.1)                                        # the next call is served


@pytest.mark.parametrize("sheet, cutoff", [(False, 0.004), (True, 0.0005)])
def test_distance_on_a_grid_enlarged_to_its_caps(ctx, sheet, cutoff):
    """cutoffs whose cells would pass a cap of the grid, so that the edge is enlarged: 0.004 on the unit cloud (251^3 cells
    pass 2^22 in all: two enlargements, 161^3) and 0.0005 on the sheet (2001 cells pass 1024 per axis: four, 821 x 821 x 2)"""
    src, pts = _clouds()
    if sheet:
        src[:, 2] = 0.5
    # 500 targets within 0.87 cutoff of a source (a random cloud has next to none that close)
    pts[-500:] = src[:500] + np.random.default_rng(12).uniform(-0.5, 0.5, (500, 3)) * cutoff
    ref, ref_count = BC.cutoff_distance(pts, src, cutoff)
    assert ref_count >= 500                                                          # (else the case checks nothing)
    d, count = ctx.cutoff_distance(pts, src, cutoff)
    assert count == ref_count and BC.same_bits(d.numpy(), ref)


def test_distance_on_an_earth_chunk_far_from_the_origin(ctx):
    gp = synth.earth_chunk(**CHUNK)["points"]                                        # |x| ~ 6.3e6 m
    corners = gp[:, BC.corner_nodes(2)]
    faces, _ = BC.boundary_faces(BC.corner_ids(corners)[0])
    side = BC.classify(corners, faces)
    # the least edge of the last element (100 km, radial; 550 km along the two others): half of it leaves nodes beyond reach
    width = min(np.linalg.norm(gp[-1, p] - gp[-1, 0]) for p in (2, 6, 18))
    for mask in (0b101, 0b111):
        nodes = BC.boundary_nodes(gp, 2, faces, side, mask)
        ref = _check_distance(ctx, gp, nodes, 0.5 * width)
        assert 0 < (ref < 0.5 * width).sum() < ref.size


def test_sources_at_the_cutoff_to_the_last_bits(ctx):
    """sources at cutoff * (1 +- 2^-50) from a target -- along an axis, along a diagonal, across cell faces wherever the
    targets happen to lie in their cells -- are inside or outside as their ROUNDED distance says"""
    rng = np.random.default_rng(5)
    eps = 2.0 ** -50
    for cutoff, scale, offset in ((1.0, 20.0, 0.0), (0.37, 9.0, 6.3e6), (1.0 / 3.0, 5.0, -1e3)):
        targets = rng.uniform(0.0, scale, (200, 3)) + offset
        targets[:20] = np.floor(targets[:20] / cutoff) * cutoff                      # some near multiples of the cutoff
        axes = np.eye(3)[rng.integers(0, 3, 200)] * rng.choice([-1.0, 1.0], 200)[:, None]
        diag = rng.normal(size=(200, 3))
        diag /= np.linalg.norm(diag, axis=1)[:, None]
        src = np.concatenate([targets + axes * (cutoff * (1 - eps)), targets - axes * (cutoff * (1 + eps)),
                              targets + diag * (cutoff * (1 - eps)), targets - diag * (cutoff * (1 + eps)),
                              targets + axes * cutoff])
        ref = _check_distance(ctx, targets, src, cutoff)
        assert 0 < (ref < cutoff).sum()
        _check_distance(ctx, targets, src[rng.permutation(len(src))], cutoff)        # the set alone defines the result


def test_a_cutoff_too_small_for_the_margin_is_refused(ctx):
    pts = np.zeros((4, 3))
    with pytest.raises(ValueError, match="cutoff below 2\\^-500"):
        ctx.cutoff_distance(pts, pts, 1e-200)
    for cutoff in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="positive and finite"):
            ctx.cutoff_distance(pts, pts, cutoff)


# --------------------------------------------------------------------------------------------------- distance_taper
def test_distance_taper_and_blend(ctx):
    rng = np.random.default_rng(8)
    n = 4099
    d = rng.uniform(0.0, 3.0, n)
    d[:7] = [0.0, 1.0, 2.0, 1.0 - 2 ** -53, 2.0 + 2 ** -51, 1.5, 3.0]
    a, b = rng.normal(size=(3, n)), rng.normal(size=(3, n))
    elem = rng.integers(-1, 5, n)
    for inner, outer in ((1.0, 2.0), (1.5, 1.5), (0.0, 0.0), (0.0, 2.5)):                 # (1.5, 1.5): a hard cut
        ref, ref_w, ref_count = BC.distance_taper(d, inner, outer, a)
        out, count, w = ctx.distance_taper(d, inner, outer, a, want_weight=True)
        assert count == ref_count and BC.same_bits(w.numpy(), ref_w) and BC.same_bits(out.numpy(), ref)
        ref, ref_w, ref_count = BC.distance_taper(d, inner, outer, a, b=b, elem=elem)
        out, count, w = ctx.distance_taper(d, inner, outer, a, b=b, elem=elem, want_weight=True)
        assert count == ref_count and BC.same_bits(w.numpy(), ref_w) and BC.same_bits(out.numpy(), ref)
    hard = BC.taper_weight(d, 1.5, 1.5)
    assert set(hard.tolist()) == {0.0, 1.0}
    # rows that were not located hold a NaN in a: it never leaks
    a_nan = a.copy()
    a_nan[:, elem < 0] = np.nan
    ref, _, _ = BC.distance_taper(d, 1.0, 2.0, a_nan, b=b, elem=elem)
    out, _ = ctx.distance_taper(d, 1.0, 2.0, a_nan, b=b, elem=elem)
    assert not np.isnan(ref).any() and BC.same_bits(out.numpy(), ref)
    assert BC.same_bits(out.numpy()[:, elem < 0], b[:, elem < 0])
    # in place on a and on b
    for target in ("a", "b"):
        a_d, b_d = ctx.to_device(a), ctx.to_device(b)
        out, _ = ctx.distance_taper(d, 1.0, 2.0, a_d, b=b_d, elem=elem, out=a_d if target == "a" else b_d)
        ref, _, _ = BC.distance_taper(d, 1.0, 2.0, a, b=b, elem=elem)
        assert BC.same_bits((a_d if target == "a" else b_d).numpy(), ref)
        assert BC.same_bits((b_d if target == "a" else a_d).numpy(), b if target == "a" else a)
    a_d = ctx.to_device(a)
    ctx.distance_taper(d, 1.0, 2.0, a_d, out=a_d)
    assert BC.same_bits(a_d.numpy(), BC.distance_taper(d, 1.0, 2.0, a)[0])
    _, count, w = ctx.distance_taper(d, 1.0, 2.0, None, want_weight=True)             # the weight alone
    assert BC.same_bits(w.numpy(), BC.taper_weight(d, 1.0, 2.0)) and count == int((w.numpy() < 1).sum())
    with pytest.raises(ValueError, match="radii"):
        ctx.distance_taper(d, 2.0, 1.0, a)


# ------------------------------------------------------------------------------------------------ taper_to_boundary
def test_taper_to_boundary(ctx, cube):
    gp, faces, side, _ = cube
    rng = np.random.default_rng(1)
    fields = {"K": rng.normal(size=gp.shape[:2]), "L": rng.normal(size=gp.shape[:2])}
    mesh = GllMesh(gp, 4, fields)
    bnd = boundary.mesh_boundary(mesh, up=UP, context=ctx)
    inner, outer = 0.05, 0.4
    values, ntapered = boundary.taper_to_boundary(mesh, ["K", "L"], inner, outer, boundary=bnd, context=ctx)
    nodes = BC.boundary_nodes(gp, 4, faces, side, 0b101)
    d, _ = BC.cutoff_distance(gp, nodes, outer)
    stacked = np.stack([fields["K"], fields["L"]])
    ref, w, ref_count = BC.distance_taper(d, inner, outer, stacked)
    assert values.shape == stacked.shape and ntapered == ref_count and BC.same_bits(values.reshape(2, -1), ref)
    assert BC.same_bits(boundary.distance_to_boundary(mesh, bnd, outer, context=ctx).reshape(-1), d)
    flat = gp.reshape(-1, 3)
    on_boundary = (flat[:, None, :] == np.unique(nodes, axis=0)[None, :, :]).all(axis=2).any(axis=1)
    assert on_boundary.sum() > 0 and (values.reshape(2, -1)[:, on_boundary] == 0.0).all()       # exactly 0 on its own nodes
    beyond = d >= outer
    assert beyond.sum() > 0 and BC.same_bits(values.reshape(2, -1)[:, beyond], stacked.reshape(2, -1)[:, beyond])
    # the free surface is left alone: top nodes away from the sides keep weight 1 ...
    top = (flat[:, 2] == 1.0) & (np.abs(flat[:, :2] - 0.5) < 0.05).all(axis=1)
    assert top.sum() > 0 and (w[top] == 1.0).all()
    # ... unless it is asked for
    values_top, _ = boundary.taper_to_boundary(mesh, "K", inner, outer, sides=("side", "top", "bottom"), boundary=bnd,
                                               context=ctx)
    assert (values_top.reshape(-1)[top] == 0.0).all()
    assert BC.same_bits(mesh.element_nodal_fields["K"], fields["K"])                            # the mesh is untouched
    with Context(0) as other:                                   # the faces and nodes live on the boundary's context
        with pytest.raises(ValueError, match="another context"):
            boundary.distance_to_boundary(mesh, bnd, outer, context=other)
        with pytest.raises(ValueError, match="another context"):
            boundary.taper_to_boundary(mesh, "K", inner, outer, boundary=bnd, context=other)


# ----------------------------------------------------------------------------------------------------- blend_models
def test_blend_models(ctx):
    host_pts = synth.earth_chunk(order=2, nlat=6, nlon=6, lat=(-12.0, 12.0), lon=(-12.0, 12.0),
                                 radii=(5_771_000.0, 6_171_000.0, synth.R_EARTH), nrad=(2, 1))["points"]
    reg_pts = synth.earth_chunk(order=4, nlat=3, nlon=3, lat=(-6.0, 6.0), lon=(-6.0, 6.0))["points"]
    f_host = 1.0 + 1e-7 * host_pts[..., 0] + 2e-7 * host_pts[..., 1]
    f_reg = 5.0 - 3e-7 * reg_pts[..., 2] + 1e-7 * reg_pts[..., 1]
    host, regional = GllMesh(host_pts, 2, {"VP": f_host}), GllMesh(reg_pts, 4, {"VP": f_reg})
    inner, outer = 50e3, 250e3
    values, info = boundary.blend_models(regional, host, "VP", inner, outer, context=ctx)
    # the composition: the Context's own interpolation, then the statements
    uniq, inv = ctx.unique_points(host_pts.reshape(-1, 3), ordered=False)
    vals, elem, _, _ = ctx.interpolate_gll(4, reg_pts, uniq, f_reg[None], want_operator=True)
    inverse = inv.numpy()
    a = vals.numpy()[inverse].T
    el = elem.numpy()[inverse]
    corners = reg_pts[:, BC.corner_nodes(4)]
    faces, _ = BC.boundary_faces(BC.corner_ids(corners)[0])
    side = BC.classify(corners, faces)
    nodes = BC.boundary_nodes(reg_pts, 4, faces, side, 0b101)
    d, _ = BC.cutoff_distance(uniq.numpy(), nodes, outer)
    ref, w, _ = BC.distance_taper(d[inverse], inner, outer, a, b=f_host.reshape(1, -1), elem=el)
    assert values.shape == (1,) + f_host.shape and BC.same_bits(values.reshape(1, -1), ref)
    assert info == {"nlocated": int((el >= 0).sum()), "nblended": int(((w > 0) & (w < 1)).sum()),
                    "nreplaced": int((w == 1).sum())}
    assert info["nlocated"] > 0 and info["nblended"] > 0 and info["nreplaced"] > 0 and (el < 0).sum() > 0
    out, b = values.reshape(-1), f_host.reshape(-1)
    assert BC.same_bits(out[el < 0], b[el < 0])                                       # outside the region: the host's bits
    deep = (el >= 0) & (d[inverse] >= outer)
    assert deep.sum() > 0 and BC.same_bits(out[deep], a[0][deep])                     # deeper than outer: the interpolated value
    slack = 4 * np.finfo(np.float64).eps * np.maximum(np.abs(a[0]), np.abs(b))
    inside = el >= 0
    assert (np.minimum(a[0], b)[inside] - slack[inside] <= out[inside]).all()
    assert (out[inside] <= np.maximum(a[0], b)[inside] + slack[inside]).all()
