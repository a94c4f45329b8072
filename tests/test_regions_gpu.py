"""mm_region_distance on the GPU against the NumPy statement of tests/regions_cases.py, bit for bit -- the signed distance, the
flags, the return value and info --, and the drivers of :mod:`multimesh_amd.regions` against their NumPy compositions.

Edge counts 0, 1, 3, 12 and one below, at, one above and two-and-a-bit times the chunk of 32 edges that shares a bounding ball
on the device; groups of 1, 8, 27 and 125 nodes in counts that are no multiple of a workgroup's 256 / P; nodes on vertices, on
edges' great circles inside and outside the arc, at the anchor and its antipode, at the centre, with NaN and inf coordinates,
and beyond a vertex as seen from the anchor, built from the vertex's own bits (regions_cases.special_nodes)."""
import numpy as np
import pytest

import regions_cases as RC
from multimesh_amd import frames
from multimesh_amd import regions as RG
from multimesh_amd import synth
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

R = RC.R_EARTH
SHAPES = ((1, 1), (1, 333), (8, 1), (8, 77), (27, 10), (27, 301), (125, 3), (125, 5))     # (P, ngroups): 256 // P is 256, 32, 9, 2


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()      # before this module's context opens the device: torch then finds it whichever test runs first
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    with Context(0) as c:
        yield c


def _check(ctx, pts, edges, anchor, flag, cutoff, scale, block=1):
    res, ninside = RG.region_distance_call(ctx, pts, edges, anchor, flag, cutoff, scale, want_inside=True, want_info=True)
    s, inside, ni, nhit, ninvalid = RC.region_distance(pts, edges, anchor, flag, cutoff, scale, block=block)
    lead = np.shape(pts)[:-1]
    assert res["signed"].shape == lead and res["inside"].shape == lead
    got_s, got_i = res["signed"].numpy().reshape(-1), res["inside"].numpy().reshape(-1)
    bad = np.flatnonzero(got_s.view(np.uint64) != s.view(np.uint64))
    assert bad.size == 0, (bad[:5], got_s[bad[:5]], s[bad[:5]])
    assert np.array_equal(got_i, inside) and ninside == ni
    assert res["info"].numpy().tolist() == [nhit, ninvalid]
    return s, inside, nhit, ninvalid


@pytest.mark.parametrize("nedges", RC.EDGE_COUNTS)
def test_against_the_statement(ctx, nedges):
    edges, anchor, flag = RC.edge_table(nedges)
    for q, (P, ngroups) in enumerate(SHAPES):
        pts = RC.node_groups(ngroups, P, edges, anchor, seed=nedges + q)
        cutoff, scale = ((0.05, R), (0.3, 1.0))[q % 2]
        s, inside, nhit, ninvalid = _check(ctx, pts, edges, anchor, flag, cutoff, scale)
        if ngroups * P >= 8:
            assert ninvalid == 5                                  # the centre, a NaN, two infs, a node below 2^-500
        if nedges >= 3 and ngroups * P > 300:
            assert 0 < inside.sum() < inside.size and 0 < nhit < inside.size
        if nedges == 0:
            valid = np.isfinite(np.linalg.norm(pts.reshape(-1, 3), axis=1)) & (np.linalg.norm(pts.reshape(-1, 3), axis=1) > 0)
            assert nhit == 0 and (inside[valid] == flag).all() and (np.abs(s) == scale * cutoff).all()


def test_a_cutoff_nobody_reaches_and_one_everybody_reaches(ctx):
    reg = RC.region_with(2 * RC.CHUNK + 7)
    pts = RC.node_groups(700, 1, reg.edges, reg.anchor, seed=5)[100:]        # generic nodes only
    s, inside, nhit, _ = _check(ctx, pts, reg.edges, reg.anchor, reg.anchor_inside, 1e-9, R)
    assert nhit == 0 and (np.abs(s) == R * 1e-9).all()
    _, _, nhit, _ = _check(ctx, pts, reg.edges, reg.anchor, reg.anchor_inside, 2.0, R)       # (past 60 degrees: no distance cull)
    assert nhit == len(pts)
    _, _, nhit, _ = _check(ctx, pts, reg.edges, reg.anchor, reg.anchor_inside, 0.999, 1.0)   # (about the largest cutoff with the cull)
    assert 0.9 * len(pts) < nhit <= len(pts)


def test_nodes_at_the_rims_of_the_culls(ctx):
    """Nodes at distance cutoff from the outline, give or take a few ulp, and nodes whose great circle through the anchor
    grazes a vertex: where a cull with too small a margin would drop the deciding edge."""
    reg = RC.region_with(4 * RC.CHUNK + 3, wiggle=0.1)
    a = reg.anchor
    cutoff = 0.03
    nodes = []
    for row in reg.edges[::3]:
        U, V, N = row[0:3], row[3:6], row[6:9]
        mid = (U + V) / np.linalg.norm(U + V)
        for sign in (1.0, -1.0):
            for k in (-3, -1, 0, 1, 3):                          # the chord cutoff is reached at the angle 2 asin(cutoff / 2)
                ang = 2.0 * np.arcsin(cutoff / 2.0) * (1.0 + k * 2.0 ** -52)
                nodes.append(np.cos(ang) * mid + sign * np.sin(ang) * N)
        side = np.cross(a, U)
        for k in (-2e-16, 0.0, 2e-16):
            nodes.append(((2.0 * (a @ U)) * U - a) + k * side)
            nodes.append(U + (U - a) * 0.5 + k * side)
    pts = np.array(nodes) * R
    s, inside, nhit, _ = _check(ctx, pts, reg.edges, a, reg.anchor_inside, cutoff, R)
    assert 0 < nhit < len(pts)
    _check(ctx, pts.reshape(-1, 8, 3)[:, :, :], reg.edges, a, reg.anchor_inside, cutoff, 1.0)


def test_three_batches_of_chunks_on_coherent_groups_and_at_the_rims_of_the_tile_tests(ctx):
    """2 * 256 * 32 + 7 edges are 513 chunks: the chunk loop of the kernel runs three batches (256, 256, 1), so its lists are
    reused and a batch without a survivor is passed over.  The groups are the elements of a small Earth chunk across the outline
    -- tiles a degree or two wide against chunks of 0.15 degrees, so the tile's own tests reject nearly every chunk -- and
    clusters an ulp wide, each a call of its own, where those tests turn over (regions_cases.tile_rim_groups).  Bit for bit."""
    reg = RC.big_region()
    a, flag = reg.anchor, reg.anchor_inside
    mesh = synth.earth_chunk(order=2, nlat=3, nlon=3, lat=(3.5, 7.5), lon=(28.0, 32.0), radii=(6_171_000.0, 6_271_000.0, R), nrad=(1, 1))
    gp = np.ascontiguousarray(mesh["points"])                          # 18 elements of 27 nodes: tiles of 9 elements
    cutoff = 0.01
    rims = RC.tile_rim_groups(reg.edges, a, cutoff, nodes=4, chunks=(0, 255, 256, 512))
    nmesh = gp.shape[0] * gp.shape[1]
    want = RC.region_distance(np.concatenate([gp.reshape(-1, 3), rims.reshape(-1, 3)]), reg.edges, a, flag, cutoff, R, block=512)
    assert 0 < want[1][:nmesh].sum() < nmesh and 0 < (np.abs(want[0][:nmesh]) < R * cutoff).sum() < nmesh
    for pts in (gp, gp.reshape(-1, 3)):                                # (P = 1: one tile of 256 nodes and one of 230)
        res, _ = RG.region_distance_call(ctx, pts, reg.edges, a, flag, cutoff, R, want_inside=True)
        assert RC.same_bits(res["signed"].numpy().reshape(-1), want[0][:nmesh])
        assert np.array_equal(res["inside"].numpy().reshape(-1), want[1][:nmesh])
    for g, group in enumerate(rims):
        res, _ = RG.region_distance_call(ctx, group[None], reg.edges, a, flag, cutoff, R, want_inside=True)
        sl = slice(nmesh + g * group.shape[0], nmesh + (g + 1) * group.shape[0])
        assert RC.same_bits(res["signed"].numpy().reshape(-1), want[0][sl]), g
        assert np.array_equal(res["inside"].numpy().reshape(-1), want[1][sl]), g


def test_either_output_alone_and_the_refusals(ctx):
    reg = RC.region_with(RC.CHUNK + 1)
    pts = RC.node_groups(40, 8, reg.edges, reg.anchor, seed=9)
    args = (reg.edges, reg.anchor, reg.anchor_inside, 0.1, R)
    s, inside, ni, _, _ = RC.region_distance(pts, *args)
    res, n = RG.region_distance_call(ctx, pts, *args)
    assert set(res) == {"signed"} and n == ni and RC.same_bits(res["signed"].numpy().reshape(-1), s)
    res, n = RG.region_distance_call(ctx, pts, *args, want_signed=False, want_inside=True)
    assert set(res) == {"inside"} and n == ni and np.array_equal(res["inside"].numpy().reshape(-1), inside)
    # every refusal leaves the outputs as they were
    sig, flg, info = ctx.to_device(np.full(320, -3.0)), ctx.to_device(np.full(320, -3, np.int32)), ctx.to_device(np.full(2, -3, np.int64))

    def refused(match, edges=reg.edges, anchor=reg.anchor, flag=reg.anchor_inside, cutoff=0.1, scale=R, both_null=False,
                ngroups=40, P=8, E=None, null=()):
        lib = RG.bind(ctx.lib)
        e, a, p = ctx.to_device(edges), ctx.to_device(anchor), ctx.to_device(pts)
        rc = lib.mm_region_distance(None if "ctx" in null else ctx.handle, None if "points" in null else p.ptr, ngroups, P,
                                    None if "edges" in null else e.ptr, len(edges) if E is None else E,
                                    None if "anchor" in null else a.ptr, flag, cutoff, scale,
                                    None if both_null else sig.ptr, None if both_null else flg.ptr, info.ptr)
        assert rc == -1 and match in ctx.lib.mm_last_error(), ctx.lib.mm_last_error()
        assert (sig.numpy() == -3.0).all() and (flg.numpy() == -3).all() and (info.numpy() == -3).all()

    refused(b"both outputs", both_null=True)
    for what in ("ctx", "points", "edges", "anchor"):
        refused(b"null", null=(what,))
    for kw in (dict(P=0), dict(P=257), dict(ngroups=-1), dict(ngroups=1 << 48), dict(E=-1), dict(E=(1 << 20) + 1), dict(cutoff=0.0),
               dict(cutoff=float("nan")), dict(scale=0.0), dict(scale=-1.0), dict(flag=-1)):
        refused(b"mm_region_distance", **kw)
    refused(b"cutoff", cutoff=2.5)
    refused(b"scale", scale=np.inf)
    refused(b"anchor_inside", flag=3)
    for col in (0, 4, 8):
        bad = reg.edges.copy()
        bad[-1, col] = np.nan
        refused(b"edge table", edges=bad)
    bad = reg.edges.copy()
    bad[5, 6:9] = -bad[5, 6:9]
    refused(b"edge table", edges=bad)                                 # N is not the stated normal
    bad = reg.edges.copy()
    bad[7, 0:3] *= 1.0 + 1e-9
    refused(b"edge table", edges=bad)                                 # U is no unit vector
    bad = reg.edges.copy()
    bad[3, 3:6] = bad[3, 0:3]
    refused(b"edge table", edges=bad)                                 # an edge of no length
    refused(b"edge table", anchor=np.array([np.inf, 0.0, 0.0]))
    refused(b"edge table", anchor=reg.anchor * 1.001)
    with pytest.raises(ValueError, match="mm_region_distance"):
        RG.region_distance_call(ctx, pts, bad, reg.anchor, 1, 0.1, R)
    with pytest.raises(ValueError, match="f64\\[E, 9\\]"):
        RG.region_distance_call(ctx, pts, reg.edges[:, :8], reg.anchor, 1, 0.1, R)
    res, n = RG.region_distance_call(ctx, np.zeros((0, 3)), *args, want_info=True)           # ngroups == 0 is valid
    assert n == 0 and res["signed"].shape == (0,) and res["info"].numpy().tolist() == [0, 0]


def test_on_a_callers_stream_with_the_callers_tensors_off_alignment(torch):
    """Late producer, early consumer, as tests/test_caller_stream_gpu.py; points, edges, anchor and outputs are views that start
    8 bytes into their buffers (the int32 flags: 4 bytes), as in tests/test_caller_views_gpu.py."""
    reg = RC.region_with(2 * RC.CHUNK + 7)
    pts = RC.node_groups(150, 27, reg.edges, reg.anchor, seed=3)
    host = (pts, reg.edges, reg.anchor)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    staged = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in host]
    torch.cuda.synchronize()

    def view(shape, dtype, fill):
        buffer = torch.full((int(np.prod(shape)) + 1,), fill, dtype=dtype, device="cuda")
        v = buffer[1:].view(tuple(shape))
        assert v.data_ptr() % 16 == (8 if dtype != torch.int32 else 4) and v.is_contiguous()
        return v

    with Context(0, stream=side.cuda_stream) as ctx, torch.cuda.stream(side):
        tp, te, ta = (view(x.shape, torch.float64, 0.0) for x in host)
        ts, ti = view(pts.shape[:2], torch.float64, -3.0), view(pts.shape[:2], torch.int32, -3)
        torch.cuda._sleep(30_000_000)
        for t, s in zip((tp, te, ta), staged):
            t.copy_(s, non_blocking=True)
        res, ninside = RG.region_distance_call(ctx, tp, te, ta, reg.anchor_inside, 0.1, R, signed_out=ts, inside_out=ti, want_info=True)
        assert res["signed"].ptr == ts.data_ptr() and res["inside"].ptr == ti.data_ptr()
        got_s, got_i = ts.clone(), ti.clone()
        ts.fill_(-7.0), ti.fill_(-7)
        side.synchronize()
        info = res["info"].numpy().tolist()
    s, inside, ni, nhit, ninvalid = RC.region_distance(pts, reg.edges, reg.anchor, reg.anchor_inside, 0.1, R)
    assert RC.same_bits(got_s.cpu().numpy().reshape(-1), s) and np.array_equal(got_i.cpu().numpy().reshape(-1), inside)
    assert ninside == ni and info == [nhit, ninvalid]


# ----------------------------------------------------------------------------------------------------------- the drivers
def _chunk_mesh(order=2):
    c = synth.earth_chunk(order=order, nlat=5, nlon=5, lat=(-8.0, 8.0), lon=(-8.0, 8.0))
    gp = c["points"]
    rng = np.random.default_rng(order)
    return GllMesh(gp, order, {"VP": 8000.0 + rng.standard_normal(gp.shape[:2]), "RHO": 3000.0 + rng.standard_normal(gp.shape[:2])})


def _hex_mesh():
    pts, conn = synth.hex_mesh(9, seed=2)
    c = RG.unit_vectors(np.array([[1.0, 2.0]]))[0]
    pts = (pts - pts.mean(axis=0)) * 2.0e6 + c[None] * 6.0e6           # a block 2 000 km wide under (1, 2) degrees
    mesh = HexMesh(pts, conn)
    mesh.attach_field("VP", 8000.0 + np.random.default_rng(4).standard_normal(len(pts)))
    return mesh


def _compose(mesh_points, region, taper_m):
    """(signed chord distance, weight) by the statement and mm_distance_taper's formula, as the module composes them."""
    unit = 2.0 * R * np.sin(taper_m / (2.0 * R)) / R
    cutoff = unit if unit > 0.0 else 2.0 ** -20
    d = RC.region_distance(mesh_points, region.edges, region.anchor, region.anchor_inside, cutoff, R)[0]
    return d, RC.taper_weight(d, 0.0, R * unit)


@pytest.mark.parametrize("kind", ("gll", "hex"))
def test_mask_taper_and_blend_against_their_compositions(ctx, kind):
    mesh = _chunk_mesh() if kind == "gll" else _hex_mesh()
    pts = mesh.gll_points if kind == "gll" else mesh.points
    lead = pts.shape[:-1]
    region = RG.Region.circle(1.0, 2.0, 5.0e5, n=90)
    names = ["VP", "RHO"] if kind == "gll" else ["VP"]
    store = mesh.element_nodal_fields if kind == "gll" else mesh.nodal_fields
    host = np.stack([store[k] for k in names])
    before = host.copy()
    for taper_m in (0.0, 2.0e5):
        d, w = _compose(pts, region, taper_m)
        assert 0 < (w == 1.0).sum() and 0 < (w == 0.0).sum() and (taper_m == 0.0 or ((w > 0) & (w < 1)).sum() > 0)
        dist = RG.region_distance(mesh, region, taper_m or 1.0e5, context=ctx)
        assert dist.shape == lead
        if taper_m:
            assert RC.same_bits(dist.numpy().reshape(-1), d)
        assert np.array_equal(RG.contains(mesh, region, context=ctx).numpy().reshape(-1), (d > 0).astype(np.int32))
        mask = RG.region_mask(mesh, region, taper_m, context=ctx)
        assert mask.shape == lead and RC.same_bits(mask.numpy().reshape(-1), w)
        values, ntapered = RG.taper_to_region(mesh, names, region, taper_m, context=ctx)
        assert values.shape == host.shape and ntapered == (w < 1.0).sum()
        flat, hflat = values.reshape(len(names), -1), host.reshape(len(names), -1)
        assert RC.same_bits(flat, w[None] * hflat) and RC.same_bits(flat[:, w == 1.0], hflat[:, w == 1.0])
        regional = host * 1.02 + 5.0
        regional.reshape(len(names), -1)[:, w == 0.0] = np.nan              # garbage outside never leaks
        located = np.arange(w.size, dtype=np.int64)
        located[::7] = -1
        wl = np.where(located < 0, 0.0, w)
        out, info = RG.blend_into(mesh, names, regional, region, taper_m, located=located.reshape(lead), context=ctx)
        oflat, rflat = out.reshape(len(names), -1), regional.reshape(len(names), -1)
        with np.errstate(invalid="ignore"):
            assert RC.same_bits(oflat, RC.blend(wl[None], rflat, hflat))
        assert RC.same_bits(oflat[:, wl == 0.0], hflat[:, wl == 0.0]) and RC.same_bits(oflat[:, wl == 1.0], rflat[:, wl == 1.0])
        assert info == {"nblended": int(((wl > 0) & (wl < 1)).sum()), "nreplaced": int((wl == 1.0).sum())}
        assert np.array_equal(np.stack([store[k] for k in names]), before)       # the mesh's fields are untouched


def test_through_a_rotated_frame(ctx):
    """An outline given in a rotated frame: the queries on frames.in_frame(mesh, R) are the statement on the rotated points."""
    mesh = _chunk_mesh(order=1)
    rot = frames.Rotation.from_axis_angle([0.3, -0.5, 0.8], 37.0)
    view = frames.in_frame(mesh, rot, context=ctx)
    centre = view.gll_points.reshape(-1, 3).mean(axis=0)
    lat = 90.0 - np.rad2deg(np.arccos(centre[2] / np.linalg.norm(centre)))
    lon = np.rad2deg(np.arctan2(centre[1], centre[0]))
    region = RG.Region.circle(lat, lon, 6.0e5, n=60)
    d, w = _compose(view.gll_points, region, 1.5e5)
    assert 0 < (w == 1.0).sum() < w.size and (w == 0.0).sum() > 0
    assert RC.same_bits(RG.region_mask(view, region, 1.5e5, context=ctx).numpy().reshape(-1), w)
    values, _ = RG.taper_to_region(view, ["VP"], region, 1.5e5, context=ctx)
    assert RC.same_bits(values.reshape(-1), w * mesh.element_nodal_fields["VP"].reshape(-1))
