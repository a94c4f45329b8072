"""mm_idw_gather, Context.idw_gather and multimesh_amd.scattered on the GPU: every value bit for bit against the NumPy
statement of tests/scattered_cases.py, evaluated on the rows (idx, dist) the device's own mm_knn_query produced."""
import numpy as np
import pytest
import torch   # (before the library is loaded, as in a run of the whole suite: its HIP runtime is the process's first)

import boundary_cases as BC
import scattered_cases as SC
from multimesh_amd import io as mio
from multimesh_amd import scattered, synth
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context, DeviceArray
from multimesh_amd.mesh import HexMesh
from multimesh_amd.scattered import PointCloud

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
FULL_GRID = 2048 * 256 + 5            # five targets past a full grid of workgroups: the grid stride runs
NSRC = 300


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def base(ctx):
    """300 samples with 5 fields, their index, and 257 targets (some outside the cloud's box)"""
    src, fields = SC.cloud(NSRC, ncomp=5, seed=11)
    return src, fields, ctx.knn_build(src), SC.targets(257, seed=12), ctx.to_device(fields)


def _both_layouts(ctx, fields, idx, dist, want, **kw):
    """Context.idw_gather in both layouts against want = SC.idw(...)"""
    ref, ref_out, ref_near, ref_used = want
    for point_major in (False, True):
        out, nout, near, used = ctx.idw_gather(fields, idx, dist, point_major=point_major, want_nearest=True,
                                               want_count=True, **kw)
        got = out.numpy().T if point_major else out.numpy()
        assert nout == ref_out and SC.same_bits(got, ref), (point_major, kw)
        assert SC.same_bits(near.numpy(), ref_near) and used.numpy().dtype == np.int32
        assert np.array_equal(used.numpy(), ref_used)


# ------------------------------------------------------------------------------ sizes, k, components, powers, layouts
@pytest.mark.parametrize("k", [1, 2, 8, 20, 21, 64])
def test_sizes_components_powers_and_layouts(ctx, base, k):
    _, fields, index, tgt, fields_d = base
    idx, dist = index.query(tgt, k, want_dist=True)
    idx_h, dist_h = idx.numpy(), dist.numpy()
    for power in (1, 2, 3, 8):
        ref, _, near, used = SC.idw(fields, idx_h, dist_h, NSRC, power=power)
        for n in SIZES:
            for ncomp in (1, 3, 4, 5):
                want = (ref[:ncomp, :n], 0, near[:n], used[:n])
                _both_layouts(ctx, fields_d.rows(0, ncomp), idx.rows(0, n), dist.rows(0, n), want, power=power)


def test_past_a_full_grid_of_workgroups(ctx, base):
    _, fields, index, _, fields_d = base
    tgt = SC.targets(FULL_GRID, seed=13)
    idx, dist = index.query(tgt, 8, want_dist=True)
    cut = 0.12
    want = SC.idw(fields[:3], idx.numpy(), dist.numpy(), NSRC, power=2, max_distance=cut, fill=-5.0)
    assert 0 < want[1] < FULL_GRID
    out, nout, near, used = ctx.idw_gather(fields_d.rows(0, 3), idx, dist, max_distance=cut, fill_value=-5.0,
                                           want_nearest=True, want_count=True)
    assert nout == want[1] and SC.same_bits(out.numpy(), want[0]) and SC.same_bits(near.numpy(), want[2])
    assert np.array_equal(used.numpy(), want[3])
    # the same on every run: integer counts, no float atomics
    again, nagain = ctx.idw_gather(fields_d.rows(0, 3), idx, dist, max_distance=cut, fill_value=-5.0)
    assert nagain == nout and BC.same_bits(again.numpy(), out.numpy())


def test_three_sources_give_padded_rows(ctx):
    src = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]])
    fields = np.array([[1.0, 2.0, 4.0], [-1.0, 0.5, 8.0]])
    tgt = SC.targets(70, seed=5)
    idx, dist = ctx.knn_build(src).query(tgt, 8, want_dist=True)
    assert (idx.numpy()[:, 3:] == 3).all() and np.isinf(dist.numpy()[:, 3:]).all()
    want = SC.idw(fields, idx.numpy(), dist.numpy(), 3, power=3)
    assert want[1] == 0 and (want[3] == 3).all()
    _both_layouts(ctx, fields, idx, dist, want, power=3)


# ------------------------------------------------------------------------------------------- max_distance, outside modes
@pytest.mark.parametrize("which", ["nobody", "partly", "wholly"])
def test_max_distance_and_both_outside_modes(ctx, base, which):
    _, fields, index, tgt, fields_d = base
    idx, dist = index.query(tgt, 8, want_dist=True)
    dist_h = dist.numpy()
    cut = {"nobody": float(dist_h.max()), "partly": float(np.sort(dist_h[:, 0])[-1]),
           "wholly": float(np.sort(dist_h[:, 0])[200])}[which]
    prior = np.random.default_rng(3).standard_normal((5, 257))
    fill = SC.idw(fields, idx.numpy(), dist_h, NSRC, max_distance=cut, fill=123.5)
    keep = SC.idw(fields, idx.numpy(), dist_h, NSRC, max_distance=cut, outside=SC.KEEP, prior=prior)
    assert fill[1] == keep[1] == {"nobody": 0, "partly": 0, "wholly": 56}[which]
    assert (fill[3] == 8).all() == (which == "nobody") and (fill[3] > 0).all() == (which != "wholly")
    _both_layouts(ctx, fields_d, idx, dist, fill, max_distance=cut, fill_value=123.5)
    for point_major in (False, True):
        mine = ctx.to_device(np.ascontiguousarray(prior.T) if point_major else prior)
        out, nout, used = ctx.idw_gather(fields_d, idx, dist, max_distance=cut, outside="keep", out=mine,
                                         point_major=point_major, want_count=True)
        got = out.numpy().T if point_major else out.numpy()
        assert out is mine and nout == keep[1] and SC.same_bits(got, keep[0]) and np.array_equal(used.numpy(), keep[3])
        assert BC.same_bits(got[:, keep[3] == 0], prior[:, keep[3] == 0])           # keep leaves the prior bits
    with pytest.raises(ValueError):
        ctx.idw_gather(fields_d, idx, dist, outside="keep")


# ---------------------------------------------------------------------------------------- exact hits, NaNs, hand-made rows
def test_targets_that_are_sources_and_duplicated_sources(ctx):
    src, fields = SC.cloud(120, ncomp=3, seed=21)
    src[40:50] = src[30:40]                                         # ten samples twice, with other values
    src[50] = src[30]                                               # ... one of them three times
    index = ctx.knn_build(src)
    for k in (1, 3, 8):
        idx, dist = index.query(src, k, want_dist=True)
        want = SC.idw(fields, idx.numpy(), dist.numpy(), 120)
        assert (dist.numpy()[:, 0] == 0.0).all() and want[1] == 0
        expect = np.arange(120)
        expect[40:51] = np.r_[30:40, 30]                            # a duplicate's value is the lowest index's
        assert BC.same_bits(want[0], fields[:, expect])
        _both_layouts(ctx, fields, idx, dist, want)


def test_nan_target_and_nan_source_coordinate(ctx):
    src, fields = SC.cloud(50, ncomp=2, seed=22)
    src[7, 1] = np.nan
    tgt = SC.targets(66, seed=23)
    tgt[5, 0] = np.nan
    tgt[65, 2] = np.nan
    idx, dist = ctx.knn_build(src).query(tgt, 8, want_dist=True)
    want = SC.idw(fields, idx.numpy(), dist.numpy(), 50, fill=-9.0)
    assert want[1] == 2 and want[3][[5, 65]].tolist() == [0, 0] and (want[0][:, [5, 65]] == -9.0).all()
    assert not (idx.numpy()[np.isfinite(tgt).all(axis=1)] == 7).any()      # the NaN source is nobody's neighbour
    _both_layouts(ctx, fields, idx, dist, want, fill_value=-9.0)


def test_nan_field_under_a_zero_weight_and_under_a_cut_neighbour(ctx):
    src = np.array([[1e-50, 0.0, 0.0], [1.0, 0.0, 0.0]])
    fields = np.array([[3.0, np.nan]])
    idx, dist = ctx.knn_build(src).query(np.zeros((1, 3)), 2, want_dist=True)
    assert idx.numpy().tolist() == [[0, 1]] and dist.numpy()[0, 1] == 1.0 and 0.0 < dist.numpy()[0, 0] < 1e-49
    zero_weight = SC.idw(fields, idx.numpy(), dist.numpy(), 2, power=8)
    assert np.isnan(zero_weight[0]).all() and zero_weight[3].tolist() == [2]      # (1e-50)^8 is 0.0, and 0.0 * NaN is NaN
    _both_layouts(ctx, fields, idx, dist, zero_weight, power=8)
    cut = SC.idw(fields, idx.numpy(), dist.numpy(), 2, power=8, max_distance=0.5)
    assert cut[0].tolist() == [[3.0]] and cut[3].tolist() == [1]                  # never read
    _both_layouts(ctx, fields, idx, dist, cut, power=8, max_distance=0.5)


def test_unsorted_hand_made_rows(ctx):
    """any contents are served: unsorted rows, indices out of range on either side, NaN, inf and negative distances, a zero
    behind the first valid entry, a row without a valid entry"""
    rng = np.random.default_rng(31)
    n, nsrc = 130, 9
    fields = rng.standard_normal((4, nsrc))
    for k in (5, 6):                                              # rows read 8 and 16 bytes at a time
        idx = rng.integers(-2, nsrc + 2, size=(n, k))
        dist = rng.random((n, k)) * 3.0
        dist[rng.random((n, k)) < 0.1] = np.nan
        dist[rng.random((n, k)) < 0.1] = 0.0
        dist[rng.random((n, k)) < 0.05] = np.inf
        dist[rng.random((n, k)) < 0.05] = -1.0
        idx[3], dist[4] = nsrc, np.nan
        for power in (1, 2, 8):
            for cut in (np.inf, 2.0):
                want = SC.idw(fields, idx, dist, nsrc, power=power, max_distance=cut, fill=0.25)
                assert want[1] >= 2
                _both_layouts(ctx, fields, idx, dist, want, power=power, max_distance=cut, fill_value=0.25)


def test_a_two_dimensional_cloud(ctx):
    src, fields = SC.cloud(90, ndim=2, ncomp=2, seed=41)
    tgt = SC.targets(77, ndim=2, seed=42)
    cloud = PointCloud(src, {"A": fields[0], "B": fields[1]})
    idx, dist = cloud.index(ctx).query(tgt, 6, want_dist=True)
    assert idx.shape == (77, 6) and cloud.index(ctx).ndim == 2
    want = SC.idw(fields, idx.numpy(), dist.numpy(), 90, power=3)
    _both_layouts(ctx, fields, idx, dist, want, power=3)
    got, nout = scattered.interpolate_scattered(cloud, tgt, k=6, power=3, context=ctx)
    assert nout == 0 and got.shape == (77, 2) and SC.same_bits(got.T, want[0])


# ---------------------------------------------------------------------------------------------------- the public module
def test_interpolate_scattered_does_not_depend_on_the_chunk_size(ctx, base):
    src, fields, _, tgt, _ = base
    cloud = PointCloud(src, fields.T, ["A", "B", "C", "D", "E"])
    idx, dist = cloud.index(ctx).query(tgt, 8, want_dist=True)
    assert cloud.index(ctx) is cloud.index(ctx)                                  # built once
    cut = float(np.sort(dist.numpy()[:, 0])[230])
    want = SC.idw(fields[[4, 1]], idx.numpy(), dist.numpy(), NSRC, power=2, max_distance=cut, fill=-2.0)
    for chunk in (1, 7, 256, 258, None):                                         # 1, 7, N - 1, N + 1 and all at once
        got, nout = scattered.interpolate_scattered(cloud, tgt, ["E", "B"], max_distance=cut, fill_value=-2.0, context=ctx,
                                                    chunk_points=chunk)
        assert nout == want[1] == 26 and SC.same_bits(got.T, want[0]), chunk
    one, _ = scattered.interpolate_scattered(cloud, tgt, "C", k=1, context=ctx)   # nearest neighbour: the sample's bits
    assert BC.same_bits(one[:, 0], fields[2, idx.numpy()[:, 0]])


def _mesh_cloud():
    """an order-2 GLL mesh of 27 elements over the unit cube and a cloud that covers part of it"""
    gp = synth.gll_mesh(4, 2, seed=3)
    rng = np.random.default_rng(51)
    src = rng.random((400, 3)) * [0.6, 1.0, 1.0]
    vals = rng.standard_normal((2, 400))
    return gp, PointCloud(src, {"VP": vals[0], "RHO": vals[1]}), vals


def _shared_copies_agree(points, values):
    """copies of a node (rows of points with equal bits) carry equal bits; some nodes do have copies"""
    flat = np.ascontiguousarray(points.reshape(-1, 3))
    _, inverse, counts = np.unique(flat.view(np.uint64), axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    assert counts.max() >= 8
    first = np.full(len(counts), -1)
    first[inverse[::-1]] = np.arange(len(flat))[::-1]
    v = np.ascontiguousarray(values.reshape(-1)).view(np.uint64)
    assert np.array_equal(v, v[first[inverse]])


def test_import_point_cloud_onto_the_three_kinds_of_mesh(ctx):
    gp, cloud, vals = _mesh_cloud()
    E, P = gp.shape[:2]
    cut = 0.15
    idx, dist = cloud.index(ctx).query(gp.reshape(-1, 3), 8, want_dist=True)
    old = np.random.default_rng(52).standard_normal((2, E, P))
    keep = SC.idw(vals, idx.numpy(), dist.numpy(), 400, max_distance=cut, outside=SC.KEEP, prior=old.reshape(2, -1))
    fill = SC.idw(vals, idx.numpy(), dist.numpy(), 400, max_distance=cut, fill=0.5)
    assert 0 < keep[1] < E * P
    # a GllMesh, keep (the default) and fill
    mesh = GllMesh(gp, 2, {"VP": old[0], "RHO": old[1], "QMU": old[0]})
    assert scattered.import_point_cloud(cloud, mesh, max_distance=cut, context=ctx) == keep[1]
    got = np.stack([mesh.element_nodal_fields["VP"], mesh.element_nodal_fields["RHO"]])
    assert got.shape == (2, E, P) and SC.same_bits(got.reshape(2, -1), keep[0])
    assert BC.same_bits(mesh.element_nodal_fields["QMU"], old[0]) and np.array_equal(mesh.gll_points, gp)
    _shared_copies_agree(gp, SC.idw(vals[:1], idx.numpy(), dist.numpy(), 400)[0])
    bare = GllMesh(gp, 2)
    with pytest.raises(ValueError):
        scattered.import_point_cloud(cloud, bare, "VP", max_distance=cut, context=ctx)      # nothing to keep
    assert scattered.import_point_cloud(cloud, bare, "RHO", max_distance=cut, outside="fill", fill_value=0.5,
                                        context=ctx) == fill[1]
    assert SC.same_bits(bare.element_nodal_fields["RHO"].reshape(-1), fill[0][1]) and list(bare.element_nodal_fields) == ["RHO"]
    _shared_copies_agree(gp, bare.element_nodal_fields["RHO"])
    # a HexMesh: nodal fields
    pts, conn = synth.hex_mesh(6, seed=4)
    hexa = HexMesh(pts, conn, {"VP": np.arange(216.0)})
    hidx, hdist = cloud.index(ctx).query(pts, 4, want_dist=True)
    want = SC.idw(vals[:1], hidx.numpy(), hdist.numpy(), 400, power=1, max_distance=cut, outside=SC.KEEP,
                  prior=np.arange(216.0)[None])
    assert scattered.import_point_cloud(cloud, hexa, "VP", k=4, power=1, max_distance=cut, context=ctx) == want[1] > 0
    assert SC.same_bits(hexa.nodal_fields["VP"], want[0][0])
    # a Salvus model: the named columns of MODEL/data, the others stay
    model = np.random.default_rng(53).standard_normal((E, 3, P))
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=gp)
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=model), ["RHO", "QMU", "VP"])
    want = SC.idw(vals, idx.numpy(), dist.numpy(), 400, max_distance=cut, outside=SC.KEEP,
                  prior=np.stack([model[:, 2, :], model[:, 0, :]]).reshape(2, -1))
    assert scattered.import_point_cloud(cloud, f, max_distance=cut, context=ctx) == want[1]
    data = f["MODEL/data"][()]
    assert SC.same_bits(data[:, 2, :].reshape(-1), want[0][0]) and SC.same_bits(data[:, 0, :].reshape(-1), want[0][1])
    assert BC.same_bits(data[:, 1, :], model[:, 1, :]) and np.array_equal(f["MODEL/coordinates"][()], gp)
    with pytest.raises(ValueError):
        scattered.import_point_cloud(PointCloud(cloud.points, {"ETA": vals[0]}), f, context=ctx)


@pytest.mark.parametrize("outside", ["keep", "fill"])
def test_blend_is_the_statement_followed_by_the_distance_taper(ctx, outside):
    gp, cloud, vals = _mesh_cloud()
    E, P = gp.shape[:2]
    cut, inner, outer = 0.15, 0.04, 0.09
    idx, dist = cloud.index(ctx).query(gp.reshape(-1, 3), 8, want_dist=True)
    old = np.random.default_rng(54).standard_normal((2, E * P))
    imported, nout, nearest, used = SC.idw(vals, idx.numpy(), dist.numpy(), 400, max_distance=cut,
                                           outside=SC.KEEP if outside == "keep" else SC.FILL, fill=np.nan, prior=old)
    want, w, _ = BC.distance_taper(nearest, inner, outer, old, b=imported)
    assert (w == 0.0).any() and ((w > 0.0) & (w < 1.0)).any() and ((w == 1.0) & (used > 0)).any() and nout > 0
    mesh = GllMesh(gp, 2, {"VP": old[0].reshape(E, P), "RHO": old[1].reshape(E, P)})
    assert scattered.import_point_cloud(cloud, mesh, max_distance=cut, outside=outside, blend=(inner, outer),
                                        context=ctx) == nout
    got = np.stack([mesh.element_nodal_fields["VP"], mesh.element_nodal_fields["RHO"]]).reshape(2, -1)
    assert SC.same_bits(got, want)
    beyond = nearest >= outer                                                    # outside nodes are at +inf
    assert (used[beyond] == 0).any() and BC.same_bits(got[:, beyond], old[:, beyond])
    assert BC.same_bits(got[:, nearest <= inner], imported[:, nearest <= inner])


# ------------------------------------------------------------------------------- caller's stream, tensors, views, errors
def test_a_callers_stream_and_torch_tensors(base):
    src, fields, _, tgt, _ = base
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream), Context(0, stream=stream.cuda_stream) as c:
        t_fields = torch.from_numpy(fields).cuda()
        t_tgt = torch.from_numpy(tgt).cuda()
        index = c.knn_build(torch.from_numpy(src).cuda())
        idx, dist = index.query(t_tgt, 8, want_dist=True)
        t_idx = torch.from_numpy(idx.numpy()).cuda()
        t_dist = torch.from_numpy(dist.numpy()).cuda()
        t_out = torch.full((5, 257), -1.0, dtype=torch.float64, device="cuda")
        stream.synchronize()
        out, nout, near = c.idw_gather(t_fields, t_idx, t_dist, power=3, out=t_out, want_nearest=True)
        want = SC.idw(fields, idx.numpy(), dist.numpy(), NSRC, power=3)
        assert out.ptr == t_out.data_ptr() and nout == want[1]
        assert SC.same_bits(t_out.cpu().numpy(), want[0]) and SC.same_bits(near.numpy(), want[2])
        index.free()


def _view(ctx, array, off=1):
    """the array on the device in a buffer of its own, starting `off` elements in: 8 (int32: 4) bytes off 16"""
    a = np.ascontiguousarray(array)
    whole = ctx.zeros((a.size + off + 3,), a.dtype)
    assert whole.ptr % 16 == 0
    view = DeviceArray(ctx, whole.ptr + off * a.dtype.itemsize, a.shape, a.dtype, owner=False, keepalive=whole)
    if a.nbytes:
        ctx.lib.mm_copy_h2d(ctx.handle, view.ptr, a.ctypes.data, a.nbytes)
    return view


@pytest.mark.parametrize("k", [8, 5])
def test_views_one_element_off_16_byte_alignment(ctx, base, k):
    _, fields, index, tgt, _ = base
    idx, dist = index.query(tgt, k, want_dist=True)
    idx_h, dist_h = idx.numpy(), dist.numpy()
    cut = float(np.sort(dist_h[:, 0])[240])
    prior = np.full((5, 257), 6.5)
    want = SC.idw(fields, idx_h, dist_h, NSRC, max_distance=cut, outside=SC.KEEP, prior=prior)
    hosts = {"fields": fields, "idx": idx_h, "dist": dist_h, "out": prior, "nearest": np.zeros(257),
             "nused": np.zeros(257, dtype=np.int32)}
    for shifted in list(hosts) + ["all"]:
        d = {name: _view(ctx, a, 1 if shifted in (name, "all") else 0) for name, a in hosts.items()}
        for name, v in d.items():
            assert (v.ptr % 16 != 0) == (shifted in (name, "all")), (shifted, name)
        rc = ctx.lib.mm_idw_gather(ctx.handle, d["fields"].ptr, NSRC, 5, d["idx"].ptr, d["dist"].ptr, 257, k, 2, cut, 2, 0.0,
                                   d["out"].ptr, 0, d["nearest"].ptr, d["nused"].ptr)
        assert rc == want[1] == 16, shifted
        assert SC.same_bits(d["out"].numpy(), want[0]) and SC.same_bits(d["nearest"].numpy(), want[2]), shifted
        assert np.array_equal(d["nused"].numpy(), want[3]), shifted


def test_every_argument_error_leaves_the_outputs_alone(ctx, base):
    _, fields, index, tgt, fields_d = base
    idx, dist = index.query(tgt[:40], 8, want_dist=True)
    out = ctx.to_device(np.full((5, 40), 4.25))
    near = ctx.to_device(np.full(40, 4.25))
    used = ctx.to_device(np.full(40, 77, dtype=np.int32))
    h, f, i, d, o, nr, nu = ctx.handle, fields_d.ptr, idx.ptr, dist.ptr, out.ptr, near.ptr, used.ptr
    inf, nan = np.inf, np.nan
    #        ctx fields nsrc ncomp idx dist n  k  power max outside fill out pm nearest nused
    good = [h, f, NSRC, 5, i, d, 40, 8, 2, inf, 0, 0.0, o, 0, nr, nu]
    bad = {"null context": {0: None}, "null idx": {4: None}, "null dist": {5: None}, "null fields": {1: None},
           "null out": {12: None}, "negative nsrc": {2: -1}, "negative ncomp": {3: -1}, "negative npoints": {6: -1},
           "k = 0": {7: 0}, "k = 65": {7: 65}, "power 0": {8: 0}, "power 9": {8: 9}, "NaN max_distance": {9: nan},
           "negative max_distance": {9: -1.0}, "outside 1": {10: 1}, "outside 3": {10: 3}, "ncomp 65536": {3: 65536}}
    for what, change in bad.items():
        args = list(good)
        for at, value in change.items():
            args[at] = value
        assert ctx.lib.mm_idw_gather(*args) == -1, what
        assert b"mm_idw_gather" in ctx.lib.mm_last_error(), what
        assert (out.numpy() == 4.25).all() and (near.numpy() == 4.25).all() and (used.numpy() == 77).all(), what
    # the method refuses the same before it calls, with ValueError
    for kw in (dict(power=0), dict(power=2.5), dict(max_distance=nan), dict(max_distance=-1.0), dict(outside="clamp")):
        with pytest.raises(ValueError):
            ctx.idw_gather(fields_d, idx, dist, **kw)
    with pytest.raises(ValueError):
        ctx.idw_gather(fields_d, idx, dist.rows(0, 39))
    # what is valid: no targets, no components (the distances and counts alone)
    assert ctx.lib.mm_idw_gather(h, f, NSRC, 5, None, None, 0, 8, 2, inf, 0, 0.0, None, 0, None, None) == 0
    assert ctx.lib.mm_idw_gather(h, None, NSRC, 0, i, d, 40, 8, 2, 0.05, 0, 0.0, None, 0, nr, nu) == \
        int((dist.numpy()[:, 0] > 0.05).sum())
    assert BC.same_bits(near.numpy(), np.where(dist.numpy()[:, 0] <= 0.05, dist.numpy()[:, 0], inf))
    assert np.array_equal(used.numpy(), (dist.numpy() <= 0.05).sum(axis=1))
    assert (out.numpy() == 4.25).all()
