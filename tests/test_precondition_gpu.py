"""mm_point_taper, mm_order_statistics, mm_clamp and multimesh_amd.precondition on the GPU, bit for bit against the NumPy
statements of tests/precondition_cases.py (which loop over every centre and sort every key: nothing is skipped there)."""
import numpy as np
import pytest

import precondition_cases as PC
from multimesh_amd import precondition, synth
from multimesh_amd.api import GllMesh, latlondepth_to_xyz
from multimesh_amd.device import POINT_TAPER_BATCH, Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def meshes():
    """order -> f64[216, P, 3] (6 x 6 x 6 elements), made once"""
    return {order: synth.gll_mesh(7, order, seed=4) for order in (1, 2, 4)}


def _check_taper(ctx, pts, centres, inner, outer, ncomp=2, seed=0):
    """One call with values and weights against the statement; returns (w, count)."""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    inner = np.broadcast_to(np.asarray(inner, dtype=np.float64), (len(centres),)).copy()
    outer = np.broadcast_to(np.asarray(outer, dtype=np.float64), (len(centres),)).copy()
    n = pts.size // 3
    vals = np.random.default_rng(seed).normal(size=(ncomp, n))
    ref_out, ref_w, ref_count = PC.taper_apply(pts, centres, inner, outer, vals)
    out, count, w = ctx.point_taper(pts, centres, inner, outer, values_in=vals if ncomp else None, want_weight=True)
    assert count == ref_count == np.count_nonzero(ref_w < 1)
    assert w.shape == pts.shape[:-1] and PC.same_bits(w.numpy().reshape(-1), ref_w)
    if ncomp:
        assert out.shape == (ncomp,) + pts.shape[:-1] and PC.same_bits(out.numpy().reshape(ncomp, -1), ref_out)
    else:
        assert out is None
    return ref_w, ref_count


def _centres_in(pts, k, seed):
    """k centres with radii, some on nodes, the rest about the mesh, overlapping"""
    rng = np.random.default_rng(seed)
    flat = pts.reshape(-1, 3)
    lo, hi = flat.min(axis=0), flat.max(axis=0)
    c = rng.uniform(lo, hi, (k, 3))
    c[::3] = flat[rng.integers(0, len(flat), len(c[::3]))]
    inner = rng.uniform(0.0, 0.08, k) * (hi - lo).max()
    inner[::4] = 0.0
    outer = inner + rng.uniform(0.0, 0.15, k) * (hi - lo).max()
    outer[1::5] = inner[1::5]                                     # hard cuts among them
    return c, inner, outer


@pytest.mark.parametrize("order", [1, 2, 4])
def test_taper_on_gll_meshes(ctx, meshes, order):
    full = meshes[order]
    tile = 256 // (order + 1) ** 3
    for nelem in (tile + 1, 3 * tile - 1, 1, 0):
        pts = full[:nelem]
        for k in (0, 1, 3, POINT_TAPER_BATCH + 1):
            c, ri, ro = _centres_in(full[:max(nelem, 1)], k, seed=10 * order + k)
            if k == 3:
                c[1] = c[0] + 0.01                                # three overlapping centres
                c[2] = c[0] - 0.02
                ro[:] = ri + 0.3
            _check_taper(ctx, pts, c, ri, ro, seed=nelem)
    # the whole mesh, a few small balls: most elements are skipped, the result is the statement's all the same
    c, ri, ro = _centres_in(full, 5, seed=77)
    w, count = _check_taper(ctx, full, c, ri * 0.2, ri * 0.2 + 0.05, ncomp=1)
    assert 0 < count < w.size // 4


def test_taper_on_clouds_and_hex8_nodes(ctx, meshes):
    flat = meshes[2].reshape(-1, 3)
    for n in (257, 767, 1, 0):
        pts = flat[:n]
        for k in (0, 1, 3, POINT_TAPER_BATCH + 1):
            c, ri, ro = _centres_in(flat[:max(n, 1)], k, seed=n + k)
            _check_taper(ctx, pts, c, ri, ro, ncomp=1, seed=n)
    # a shuffled cloud: every tile's box is the whole cloud
    pts = np.random.default_rng(1).permutation(flat)[:3000]
    c, ri, ro = _centres_in(pts, 40, seed=3)
    _check_taper(ctx, pts, c, ri, ro)


def _axis_nodes(centre, inner, outer):
    """nodes on the x axis through the centre at d == outer, one ulp below and above, the same at inner, and both sides"""
    cx, cy, cz = centre
    xs = []
    for r in (outer, inner):
        for sign in (1.0, -1.0):
            x = cx + sign * r
            xs += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    xs += [cx, cx + 0.5 * (inner + outer), cx + 2 * outer, cx - 3 * outer]
    return np.array([[x, cy, cz] for x in xs])


def test_taper_placement_cases(ctx, meshes):
    full = meshes[1]
    node = full[40, 3].copy()
    # a centre exactly on a node: inner = 0 (only d == 0 is cut to zero) and inner > 0
    for inner in (0.0, 0.05):
        w, count = _check_taper(ctx, full[:70], [node], inner, 0.2)
        assert (w == 0).any() and count > 0
    # outer == inner: a hard cut, 0 or 1 and nothing between
    w, _ = _check_taper(ctx, full[:70], [node, full[3, 0]], [0.15, 0.0], [0.15, 0.0])
    assert set(np.unique(w)) == {0.0, 1.0} and (w == 0).sum() >= 2
    # nodes on a coordinate axis at exactly d == outer / inner and one ulp to either side: exact distances
    centre, inner, outer = (0.0, 2.0, 3.0), 0.25, 0.75      # (x = 0: x itself is dx, and its neighbours are d's)
    nodes = _axis_nodes(centre, inner, outer)                    # 16 nodes: two order-1 elements, or a cloud
    d = np.abs(nodes[:, 0] - centre[0])
    assert (d == outer).sum() == 2 and (d == inner).sum() == 2
    for pts in (nodes.reshape(2, 8, 3), nodes):
        w, _ = _check_taper(ctx, pts, [centre], inner, outer)
        assert (w[d >= outer] == 1).all() and (w[d <= inner] == 0).all() and ((w[(d > inner) & (d < outer)] > 0).all())
    # an element of which a single corner lies one ulp inside outer, the box test at its margin: the box's nearest corner
    # IS that node, so the box distance is the node's distance bit for bit; outer one ulp above it must cut, at it must not
    lo, hi = np.array([2.1, 2.3, 2.7]), np.array([3.3, 3.1, 3.9])
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for k in (0, 1) for j in (0, 1) for i in (0, 1)])
    c0 = np.array([0.1, -0.2, 0.3])
    for sign in (1.0, -1.0):                                     # the box on either side of the centre
        el = (c0 + sign * (corners - c0)).reshape(1, 8, 3)
        dx = el[0, 0] - c0
        dmin = np.sqrt((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2])
        up, down = np.nextafter(dmin, np.inf), np.nextafter(dmin, 0.0)
        w, count = _check_taper(ctx, el, [c0], up, up)           # a hard cut one ulp beyond the corner
        assert count == 1 and w[0] == 0.0
        w, count = _check_taper(ctx, el, [c0], dmin, dmin)       # d == inner == outer: d <= inner is asked first
        assert count == 1 and w[0] == 0.0
        assert _check_taper(ctx, el, [c0], down, down)[1] == 0
        assert _check_taper(ctx, el, [c0], 0.5 * dmin, dmin)[1] == 0      # d == outer > inner: 1.0
        _check_taper(ctx, el, [c0], 0.5 * dmin, up)              # (the smoothstep one ulp inside outer rounds to 1.0)
        w, count = _check_taper(ctx, el, [c0], 0.5 * dmin, 1.001 * dmin)
        assert count == 1 and 0.0 < w[0] < 1.0
    # an element that encloses the whole ball: the box is hit, no node is
    big = (np.array([0.5, 0.5, 0.5]) + 20.0 * (corners - corners.mean(axis=0))).reshape(1, 8, 3)
    w, count = _check_taper(ctx, big, [[0.5, 0.5, 0.5]], 0.5, 1.0)
    assert count == 0
    # a NaN coordinate in one node: that node keeps w = 1, its element's other nodes are cut as ever
    pts = full[:70].copy()
    pts[40, 5, 1] = np.nan
    w, count = _check_taper(ctx, pts, [node], 0.1, 0.4)
    assert w.reshape(70, 8)[40, 5] == 1.0 and (w.reshape(70, 8)[40] < 1).sum() >= 6
    pts[41] = np.nan                                             # and an element without a finite coordinate
    _check_taper(ctx, pts, [node], 0.1, 0.4)


def test_taper_data_paths(ctx, meshes):
    full = meshes[2][:50]
    n = full.shape[0] * full.shape[1]
    c, ri, ro = _centres_in(full, 4, seed=9)
    for ncomp in (0, 1, 3):
        _check_taper(ctx, full, c, ri, ro, ncomp=ncomp)
    vals = np.random.default_rng(2).normal(size=(3, n))
    ref_out, ref_w, ref_count = PC.taper_apply(full, c, ri, ro, vals)
    # in place
    d = ctx.to_device(vals)
    out, count = ctx.point_taper(full, c, ri, ro, values_in=d, out=d)
    assert out is d and count == ref_count and PC.same_bits(d.numpy(), ref_out)
    # a single component of the points' shape, and the API
    out, count = ctx.point_taper(full, c, ri, ro, values_in=vals[0].reshape(full.shape[:2]))
    assert out.shape == (1,) + full.shape[:2] and PC.same_bits(out.numpy().reshape(-1), ref_out[0])
    mesh = GllMesh(full, 2, {"a": vals[0].reshape(full.shape[:2]), "b": vals[1].reshape(full.shape[:2])})
    w = precondition.taper_around_points(mesh, c, ri, ro, context=ctx)
    assert w.shape == full.shape[:2] and PC.same_bits(w.reshape(-1), ref_w)
    cut, ncut = precondition.cut_around_points(mesh, ["b", "a"], c, ri, ro, context=ctx)
    assert ncut == ref_count and cut.shape == (2,) + full.shape[:2] and PC.same_bits(cut.reshape(2, -1), ref_out[[1, 0]])
    assert PC.same_bits(mesh.element_nodal_fields["a"].reshape(-1), vals[0])           # the mesh's fields are untouched
    hexmesh = HexMesh(full.reshape(-1, 3)[:64], np.arange(64).reshape(8, 8), {"a": vals[0][:64]})
    cut, ncut = precondition.cut_around_points(hexmesh, ["a"], c, ri, ro, context=ctx)
    assert cut.shape == (1, 64) and PC.same_bits(cut, PC.taper_apply(full.reshape(-1, 3)[:64], c, ri, ro, vals[:1, :64])[0])
    # an in-place call whose centres hit nothing leaves the array's bits alone, NaN payloads and all
    odd = vals.copy()
    odd.view(np.uint64)[0, :5] = [0x7FF0000000000001, 0xFFF8000000000123, 0x8000000000000000, 0x7FF4000000000000, 1]
    d = ctx.to_device(odd)
    out, count = ctx.point_taper(full, [[50.0, 50.0, 50.0]], 0.1, 0.2, values_in=d, out=d)
    assert count == 0 and np.array_equal(d.numpy().view(np.uint64), odd.view(np.uint64))
    # refusals write nothing
    for bad_c, bad_i, bad_o in (([[np.nan, 0, 0]], 0.1, 0.2), ([[0.0, np.inf, 0]], 0.1, 0.2), ([[0.2, 0.2, 0.2]], -0.1, 0.2),
                                ([[0.2, 0.2, 0.2]], 0.3, 0.2), ([[0.2, 0.2, 0.2]], 0.1, np.inf), ([[0.2, 0.2, 0.2]], np.nan, 0.2)):
        d = ctx.to_device(vals)
        wd = ctx.to_device(np.full(n, 7.0))
        good = np.array([[0.3, 0.3, 0.3]])
        cc = np.concatenate([good, np.asarray(bad_c, dtype=np.float64)])
        held = [ctx.to_device(full), ctx.to_device(cc), ctx.to_device(np.array([0.1, bad_i])),
                ctx.to_device(np.array([0.5, bad_o]))]
        rc = ctx.lib.mm_point_taper(ctx.handle, held[0].ptr, full.shape[0], full.shape[1], held[1].ptr, held[2].ptr,
                                    held[3].ptr, 2, 3, d.ptr, d.ptr, wd.ptr)
        assert rc == -1 and b"mm_point_taper" in ctx.lib.mm_last_error()
        assert PC.same_bits(d.numpy(), vals) and (wd.numpy() == 7.0).all()
        with pytest.raises(ValueError):
            ctx.point_taper(full, cc, [0.1, bad_i], [0.5, bad_o], want_weight=True)


# ------------------------------------------------------------------------------------------------ order statistics
def _rows(n, seed):
    """f64[9, n]: the kinds of data the select must be exact on, one per row"""
    rng = np.random.default_rng(seed)
    rows = np.empty((9, n))
    rows[0] = 3.25                                                # all equal: every pass keeps everything
    a = 1.0 + 2.0 ** -30
    rows[1] = np.where(rng.random(n) < 0.5, a, np.nextafter(a, 2.0))            # differ in the last mantissa bit
    rows[2] = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    rows[3] = rng.choice([np.inf, -np.inf, 1.0, -1.0, 0.0], n)
    rows[4] = rng.integers(-40, 40, n) * 5e-324                   # denormals of both signs, zeros among them
    rows[5] = rng.normal(size=n)
    nan = rng.random(n) < 0.3
    rows[5][nan] = np.where(rng.random(nan.sum()) < 0.5, np.nan, -np.nan)       # NaNs of both signs
    rows[6] = np.nan                                              # all NaN
    rows[7] = 1.0 + rng.random(n)                                 # one binade of smooth data
    rows[8] = rng.normal(size=n) * 10.0 ** rng.uniform(-300, 300, n)            # 600 decades
    rows[6].view(np.uint64)[::2] |= np.uint64(1) << np.uint64(63)
    return rows


Q4 = [0.0, 0.5, 0.999, 1.0]
Q16 = [0.0, 0.5, 0.5, 0.999, 1.0, 1.0, 0.25, 0.75, 0.1, 0.9, 0.5, 0.001, 0.3333333333333333, 0.999, 0.0, 0.6]


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097, 100003])
def test_order_statistics(ctx, n):
    rows = _rows(n, seed=n)
    d = ctx.to_device(rows)
    for absolute in (False, True):
        for method in ("lower", "higher"):
            for q in ([0.999], Q4, Q16):
                ref, ref_nvalid = PC.order_statistics(rows, q, absolute=absolute, method=method)
                out, nvalid = ctx.order_statistics(d, q, absolute=absolute, method=method)
                assert out.shape == (9, len(q)) and np.array_equal(nvalid.numpy(), ref_nvalid)
                assert PC.same_bits_nan(out.numpy(), ref), (n, absolute, method, len(q))
    # ... and against np.sort of the valid values with the statement's rank (== : np.sort does not order the zeros' signs)
    out = ctx.order_statistics(d, Q4, method="higher")[0].numpy()
    for c in (0, 1, 3, 5, 7, 8):
        valid = np.sort(rows[c][~np.isnan(rows[c])])
        assert np.array_equal(out[c], valid[PC.ranks(Q4, valid.size, "higher")]), (n, c)
    assert np.isnan(out[6]).all()
    # a single row given flat, a q that is on the device already
    one, nv = ctx.order_statistics(rows[8], ctx.to_device(np.array(Q4)))
    assert one.shape == (1, 4) and PC.same_bits(one.numpy(), PC.order_statistics(rows[8], Q4)[0]) and nv.numpy()[0] == n


def test_order_statistics_refusals_and_quantiles(ctx):
    rows = _rows(1000, seed=5)
    for q in ([-0.1], [1.0000001], [np.nan], [0.5, 2.0]):
        qd = ctx.to_device(np.array(q))
        out = ctx.to_device(np.full((9, len(q)), 7.0))
        nv = ctx.to_device(np.full(9, 7, dtype=np.int64))
        vd = ctx.to_device(rows)
        rc = ctx.lib.mm_order_statistics(ctx.handle, vd.ptr, 1000, 9, 0, qd.ptr, len(q), 0, out.ptr, nv.ptr)
        assert rc == -1 and b"q must lie" in ctx.lib.mm_last_error()
        assert (out.numpy() == 7.0).all() and (nv.numpy() == 7).all()
    # n == 0 and no components
    out, nv = ctx.order_statistics(np.zeros((2, 0)), [0.5])
    assert np.isnan(out.numpy()).all() and nv.numpy().tolist() == [0, 0]
    # field_quantiles: lower / higher are the statistics, linear is formed from them as NumPy does
    v = rows[[5, 7, 8]]
    for method in ("lower", "higher"):
        got = precondition.field_quantiles(v, Q4, method=method, context=ctx)
        assert PC.same_bits(got, PC.order_statistics(v, Q4, method=method)[0])
    lin = precondition.field_quantiles(v, Q4, context=ctx)
    lo, nvalid = PC.order_statistics(v, Q4, method="lower")
    hi, _ = PC.order_statistics(v, Q4, method="higher")
    pos = np.array(Q4)[None, :] * (nvalid[:, None] - 1).astype(np.float64)
    assert PC.same_bits(lin, np.where(hi == lo, lo, lo + (hi - lo) * (pos - np.floor(pos))))
    for c in range(3):
        valid = v[c][~np.isnan(v[c])]
        assert np.allclose(lin[c], np.quantile(valid, Q4), rtol=1e-12, atol=0)
    mesh = GllMesh(synth.gll_mesh(3, 1), 1, {"k": np.arange(64.0).reshape(8, 8)})
    assert precondition.field_quantiles(mesh, 0.5, params=["k"], absolute=True, context=ctx).tolist() == [[31.5]]


# --------------------------------------------------------------------------------------------------------- the clamp
@pytest.mark.parametrize("n", [1, 257, 100003])
def test_clamp(ctx, n):
    rng = np.random.default_rng(n)
    v = rng.normal(size=(3, n)) * np.array([[1.0], [1e-3], [1e6]])
    v[0, ::11] = np.nan
    v[1, ::5] = -0.0
    v[2, ::13] = np.inf
    d = ctx.to_device(v)
    # bounds taken straight from the select's device output
    stat, _ = ctx.order_statistics(d, [0.9], absolute=True, method="higher")
    ref_bound = PC.order_statistics(v, [0.9], absolute=True, method="higher")[0][:, 0]
    out, changed = ctx.clamp(d, upper=stat.reshape(3), symmetric=True)
    ref, ref_changed = PC.clamp(v, upper=ref_bound, symmetric=True)
    assert PC.same_bits_nan(stat.numpy()[:, 0], ref_bound)
    assert PC.same_bits_nan(out.numpy(), ref) and np.array_equal(changed.numpy(), ref_changed)
    assert np.array_equal(np.signbit(out.numpy()[1, ::5]), np.ones(len(v[1, ::5]), dtype=bool))   # -0.0 is kept
    assert PC.same_bits_nan(d.numpy(), v)                         # not in place: the input is as it was
    # one-sided bounds, from the host
    for lower, upper in ((None, [0.5, 0.0, 1e5]), ([-0.5, 0.0, -np.inf], None), ([-1.0, -1e-3, 0.0], [0.5, 1e-4, np.inf])):
        out, changed = ctx.clamp(d, lower=lower, upper=upper)
        ref, ref_changed = PC.clamp(v, lower=lower, upper=upper)
        assert PC.same_bits_nan(out.numpy(), ref) and np.array_equal(changed.numpy(), ref_changed)
    # in place, without the count
    out, changed = ctx.clamp(d, upper=[0.5, 1e-4, 2.0], symmetric=True, out=d, want_count=False)
    assert out is d and changed is None and PC.same_bits_nan(d.numpy(), PC.clamp(v, upper=[0.5, 1e-4, 2.0], symmetric=True)[0])
    with pytest.raises(ValueError):
        ctx.clamp(d, lower=[0.0] * 3, upper=[1.0] * 3, symmetric=True)


# ------------------------------------------------------------------------------------------------------ composition
@pytest.fixture(scope="module")
def chunk():
    ch = synth.earth_chunk(order=2)
    pts = ch["points"]
    rng = np.random.default_rng(8)
    r = np.linalg.norm(pts, axis=2)
    fields = {"VSV": rng.normal(size=pts.shape[:2]) * (1.0 + 50.0 * (r > 6.3e6)), "RHO": rng.normal(size=pts.shape[:2]) * 1e-9}
    return GllMesh(pts, 2, fields)


def test_clip_fields_is_statement_after_statement(ctx, chunk):
    names = ["RHO", "VSV"]
    v = np.stack([chunk.element_nodal_fields[k] for k in names]).reshape(2, -1)
    bound = PC.order_statistics(v, [0.99], absolute=True, method="higher")[0][:, 0]
    ref, ref_changed = PC.clamp(v, upper=bound, symmetric=True)
    out, b, nclipped = precondition.clip_fields(chunk, names, quantile=0.99, context=ctx)
    assert out.shape == (2,) + chunk.gll_points.shape[:2] and PC.same_bits(out.reshape(2, -1), ref)
    assert PC.same_bits(b, bound) and np.array_equal(nclipped, ref_changed) and (nclipped > 0).all()
    out, b, nclipped = precondition.clip_fields(v[1], upper=1.5, context=ctx)
    ref, ref_changed = PC.clamp(v[1], upper=[1.5], symmetric=True)
    assert out.shape == (1, v.shape[1]) and PC.same_bits(out, ref) and b.tolist() == [1.5] and nclipped[0] == ref_changed[0]
    out, b, nclipped = precondition.clip_fields(v, lower=[-1e-9, 0.0], upper=[2e-9, np.inf], symmetric=False, context=ctx)
    assert PC.same_bits(out, PC.clamp(v, lower=[-1e-9, 0.0], upper=[2e-9, np.inf])[0])


def test_precondition_kernel_is_the_composition(ctx, chunk):
    sources = np.array([[0.0, 0.0, 10_000.0], [3.0, -2.0, 150_000.0]])
    receivers = np.array([[2.0, 3.0, 0.0], [-5.0, 5.0, 0.0], [0.5, 0.2, 0.0]])
    names = ["VSV", "RHO"]
    v = np.stack([chunk.element_nodal_fields[k] for k in names]).reshape(2, -1)
    centres = np.concatenate([latlondepth_to_xyz(sources), latlondepth_to_xyz(receivers)])
    inner = np.array([50e3, 50e3, 20e3, 20e3, 20e3])
    outer = np.array([300e3, 300e3, 100e3, 100e3, 100e3])
    cut, w, ncut = PC.taper_apply(chunk.gll_points, centres, inner, outer, v)
    assert 0 < ncut < w.size
    bound = PC.order_statistics(cut, [0.995], absolute=True, method="higher")[0][:, 0]
    ref, ref_changed = PC.clamp(cut, upper=bound, symmetric=True)
    out, report = precondition.precondition_kernel(chunk, names, sources=sources, receivers=receivers,
                                                   source_cut=(50e3, 300e3), receiver_cut=(20e3, 100e3),
                                                   clip_quantile=0.995, context=ctx)
    assert list(out) == names and report["ncut"] == ncut
    for c, name in enumerate(names):
        assert out[name].shape == chunk.gll_points.shape[:2] and PC.same_bits(out[name].reshape(-1), ref[c]), name
        assert report["bound"][name] == bound[c] and report["nclipped"][name] == ref_changed[c] > 0
    assert PC.same_bits(chunk.element_nodal_fields["VSV"].reshape(-1), v[0])          # the mesh's fields are untouched
    # receivers alone, no clipping; nothing at all
    out, report = precondition.precondition_kernel(chunk, ["RHO"], receivers=receivers, receiver_cut=(20e3, 100e3), context=ctx)
    ref_cut, _, n2 = PC.taper_apply(chunk.gll_points, centres[2:], inner[2:], outer[2:], v[1:])
    assert PC.same_bits(out["RHO"].reshape(-1), ref_cut[0]) and report == {"ncut": n2, "bound": {"RHO": None}, "nclipped": {"RHO": 0}}
    out, report = precondition.precondition_kernel(chunk, ["RHO"], context=ctx)
    assert PC.same_bits(out["RHO"].reshape(-1), v[1]) and report["ncut"] == 0
