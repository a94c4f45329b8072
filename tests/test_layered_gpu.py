"""mm_layered_model_apply on the GPU against the NumPy statement of tests/layered_cases.py.

The device's acos and atan2 are the only part that cannot be bit for bit: the returned angles are compared with NumPy's
within 1e-11 degrees (the bound of tests/test_grid_import_gpu.py), the depth bit for bit.  Everything after them -- values,
layer, span and the count of outside nodes -- is compared bit for bit (NaN positions compared, payloads not) by evaluating
the statement on the coordinates the device returned."""
import numpy as np
import pytest

import harmonic_cases as HC
import layered_cases as LC
from multimesh_amd import harmonics as H
from multimesh_amd import io as mio
from multimesh_amd import layered as LY
from multimesh_amd import synth
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

ANGLE_TOL = 1e-11               # degrees
CAP_LANES = 2048 * 256          # kMaxBlocks workgroups of 256 lanes: beyond, the workgroups stride
LATERALS = {"cell": LC.CELL, "bilinear": LC.BILINEAR}
PICKS = {"node": LC.NODE, "element": LC.ELEMENT}
OUTSIDES = {"fill": LC.FILL, "clamp": LC.CLAMP, "keep": LC.KEEP}


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()      # before this module's context opens the device: torch then finds it whichever test runs first
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    with Context(0) as c:
        yield c


def _prefill(ncomp, n):
    return np.random.default_rng(ncomp * 1000 + n).normal(size=(ncomp, n))


def _compare(got, pts, model, lateral, pick, outside, fill, periodic, prefilled, start):
    """What the device returned (host arrays) against the statement on its own coordinates -> (want..., inside)."""
    lat, lon, bounds, values = model
    flat = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(flat)
    lld = got["latlondepth"].reshape(n, 3)
    with np.errstate(all="ignore"):
        ref = LC.latlondepth(flat)
        if periodic:
            ref[:, 1] = LC.wrap(ref[:, 1], lon[0])
        finite = np.isfinite(flat).all(axis=1)
        dlon = np.abs(lld[finite, 1] - ref[finite, 1])
        dlon = np.minimum(dlon, np.abs(dlon - 360.0))          # (a longitude within rounding of the wrap may land on either side)
        dlat = np.abs(lld[finite, 0] - ref[finite, 0])
    assert n == 0 or not finite.any() or (dlat.max() <= ANGLE_TOL and dlon.max() <= ANGLE_TOL), (dlat.max(), dlon.max())
    assert LC.same_bits_nan(lld[finite, 2], ref[finite, 2])
    dp = LC.element_depth(pts) if pick == "element" and np.ndim(pts) == 3 else None
    want, layer, span, nout = LC.model_apply(lld, dp, lat, lon, bounds, values, LATERALS[lateral],
                                             PICKS[pick] if dp is not None else LC.NODE, OUTSIDES[outside], fill, prefilled)
    assert np.array_equal(got["layer"].reshape(n), layer), f"{(got['layer'].reshape(n) != layer).sum()} of {n} layers differ"
    assert LC.same_bits_nan(got["span"].reshape(n, 2), span)
    assert LC.same_bits_nan(got["out"].reshape(want.shape), want)
    assert got["count"] == start + nout
    if outside == "keep" and want.size:
        assert LC.same_bits_nan(got["out"].reshape(want.shape)[:, layer < 0], prefilled[:, layer < 0])
    return want, layer, span, nout


def _check(ctx, pts, model, lateral="bilinear", pick="node", outside="fill", fill=np.nan, periodic=False, start=0):
    lat, lon, bounds, values = model
    ncomp = 0 if values is None else values.shape[3]
    n = int(np.prod(np.shape(pts)[:-1]))
    prefilled = _prefill(ncomp, n)
    count = ctx.to_device(np.array([start], dtype=np.int64))
    res = LY.layered_model_apply(ctx, pts, lat, lon, bounds, values, lon_periodic=periodic, lateral=lateral, pick=pick,
                                 outside=outside, fill_value=fill, out=ctx.to_device(prefilled) if outside == "keep" else None,
                                 want_layers=True, want_span=True, want_latlondepth=True, noutside=count)
    got = {k: a.numpy() for k, a in res.items()}
    got["count"] = int(count.numpy()[0])
    return _compare(got, pts, model, lateral, pick, outside, fill, periodic, prefilled, start)


# ----------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_sizes_around_the_wave_and_the_workgroup(ctx, n):
    _, layer, _, nout = _check(ctx, LC.cloud(n, seed=n), LC.regional(5, 2, seed=n), start=7)
    if n >= 63:
        assert 0 < nout < n and len(set(layer)) >= 4


@pytest.mark.parametrize("P", (5, 27, 125))
@pytest.mark.parametrize("pick", ("node", "element"))
def test_elements(ctx, P, pick):
    pts = LC.elements(-(-257 // P), P, seed=P)
    for lateral in ("cell", "bilinear"):
        _, layer, _, nout = _check(ctx, pts, LC.regional(5, 2, seed=P), lateral=lateral, pick=pick)
        assert 0 < nout < layer.size


def test_past_the_launch_cap(ctx):
    """More points than kMaxBlocks * 256 lanes at P = 1: the stride loop runs (and its second step ends in a partial tile)."""
    n = CAP_LANES + 1000
    _, layer, _, nout = _check(ctx, LC.cloud(n, seed=1, depth=(-4000.0, 14000.0)), LC.regional(2, 1, seed=3))
    assert 0 < nout < n


# ---------------------------------------------------------------------------------------------------------- combinations
@pytest.mark.parametrize("outside", ("fill", "clamp", "keep"))
@pytest.mark.parametrize("pick", ("node", "element"))
@pytest.mark.parametrize("lateral", ("cell", "bilinear"))
def test_modes_on_the_regional_and_the_periodic_model(ctx, lateral, pick, outside):
    pts = LC.elements(40, 8, seed=5)
    _, layer, _, nout = _check(ctx, pts, LC.regional(5, 3, seed=1), lateral, pick, outside, fill=-12345.5, start=1234567)
    assert (nout > 0 or outside == "clamp") and (layer >= 0).any()
    everywhere = LC.elements(40, 8, seed=6, lat=(-89.0, 89.0), lon=(-180.0, 180.0))
    _, layer, _, nout = _check(ctx, everywhere, LC.global_model(5, 3, seed=2), lateral, pick, outside, periodic=True)
    assert (layer >= 0).any()


@pytest.mark.parametrize("ncomp", (0, 1, 3, 4, 5))
@pytest.mark.parametrize("nb", (2, 5))
def test_components_and_interfaces(ctx, ncomp, nb):
    """0: layers only; 1, 3, 4: the unrolled forms; 5: the loop.  The count is taken once."""
    lat, lon, bounds, values = LC.regional(nb, ncomp, seed=ncomp)
    for lateral in ("cell", "bilinear"):
        _, _, _, nout = _check(ctx, LC.cloud(300, seed=ncomp), (lat, lon, bounds, values if ncomp else None), lateral, start=5)
        assert nout > 0


def test_axes_of_length_one(ctx):
    lat, lon, bounds, values = LC.regional(5, 2, seed=4)
    pts = LC.cloud(300, seed=2)
    for outside in ("fill", "clamp"):
        for lateral in ("cell", "bilinear"):
            _check(ctx, pts, (lat[3:4], lon, np.ascontiguousarray(bounds[3:4]), np.ascontiguousarray(values[3:4])), lateral, outside=outside)
            _check(ctx, pts, (lat, lon[4:5], np.ascontiguousarray(bounds[:, 4:5]), np.ascontiguousarray(values[:, 4:5])), lateral, outside=outside)
            _, layer, _, _ = _check(ctx, pts, (lat[:1], lon[:1], np.ascontiguousarray(bounds[:1, :1]), np.ascontiguousarray(values[:1, :1])),
                                    lateral, outside=outside)
            assert (layer >= 0).any()


def test_axes_in_global_memory(ctx):
    """nlat + nlon > 2048: the axes are bisected in global memory."""
    lat, lon = np.array([-6.0, 0.0, 6.0]), np.linspace(-5.5, 6.5, 2050)
    model = LC.layered_tables(lat, lon, 2, 2, seed=8)
    for lateral in ("cell", "bilinear"):
        for outside in ("fill", "clamp"):
            _, layer, _, _ = _check(ctx, LC.cloud(300, seed=3, depth=(-4000.0, 14000.0)), model, lateral, outside=outside)
            assert (layer >= 0).any()


# -------------------------------------------------------------------------------------------------------- special points
@pytest.mark.parametrize("lateral", ("cell", "bilinear"))
def test_special_points(ctx, lateral):
    r = LC.R_EARTH - 5000.0
    lat, lon, bounds, values = LC.global_model(5, 2, seed=3)
    pts = LC.sphere_cloud(80, seed=4)
    pts[:12] = [[0, 0, r], [0, 0, -r], [0, 0, 0], [r, 0, 0], [-r, 0, 0], [-r, -0.0, 0], [0, r, 0], [0, -r, 0],
                [np.nan, 1.0, r], [np.inf, 0, r], [1.0, -np.inf, 2.0], [0, 0, np.inf]]
    pts[12:15] = LC.xyz(lat[2], [lon[3], lon[4], -180.0], 10000.0)            # on map nodes
    for outside in ("fill", "clamp"):
        _, layer, _, _ = _check(ctx, pts, (lat, lon, bounds, values), lateral, outside=outside, periodic=True)
        assert layer[8] == -1 and (layer[:2] >= 0).all()
    # the regional map: on its edge, just outside it, on a map node
    lat, lon, bounds, values = LC.regional(5, 2, seed=3)
    eps = 1e-9
    edge = LC.xyz([lat[0], lat[0] - eps, lat[-1], lat[-1] + eps, 0.0, 0.0, 0.0, 0.0, lat[2]],
                  [0.0, 0.0, 0.0, 0.0, lon[0], lon[0] - eps, lon[-1], lon[-1] + eps, lon[3]], 9000.0)
    for outside in ("fill", "clamp"):
        _check(ctx, np.concatenate([edge, LC.cloud(60, seed=5)]), (lat, lon, bounds, values), lateral, outside=outside)


@pytest.mark.parametrize("lateral", ("cell", "bilinear"))
def test_depths_on_the_interfaces(ctx, lateral):
    """On a flat model depth == 6371000 - r exactly for a point on the z axis... and on any node the statement decides: the
    device's depth is what it compares.  Points are built so that their depth is EXACTLY an interface."""
    lat, lon = np.array([80.0, 90.0]), np.array([-180.0, 0.0, 180.0])
    b = np.array([-2000.0, 0.0, 5000.0, 5000.0, 20000.0])
    bounds = np.ascontiguousarray(np.broadcast_to(b, (2, 3, 5)))
    values = np.random.default_rng(1).uniform(1.0, 2.0, (2, 3, 4, 2))
    depths = np.array([-2000.5, -2000.0, -1.0, 0.0, 4999.5, 5000.0, 19999.5, 20000.0, 20000.5])
    pts = np.zeros((depths.size, 3))
    pts[:, 2] = LC.R_EARTH - depths                                       # the north pole: r = z exactly
    want = {"fill": [-1, 0, 0, 1, 1, 3, 3, 3, -1], "clamp": [0, 0, 0, 1, 1, 3, 3, 3, 3]}
    for outside in ("fill", "clamp"):
        _, layer, span, _ = _check(ctx, pts, (lat, lon, bounds, values), lateral, outside=outside, periodic=True)
        assert list(layer) == want[outside]
        assert np.array_equal(span[layer == 3], np.broadcast_to([5000.0, 20000.0], ((layer == 3).sum(), 2)))


def test_a_wave_with_every_layer_and_a_wave_wholly_outside(ctx):
    """64 consecutive nodes of one column, stepping down through all the layers (the lanes of the wave stop their scans at
    different j), then 64 nodes far outside the map, then 64 more inside."""
    lat, lon, bounds, values = LC.regional(5, 3, seed=6)
    column = LC.xyz(1.0, 1.0, np.linspace(-4000.0, 50000.0, 64))
    away = LC.xyz(40.0, 60.0, np.linspace(0.0, 30000.0, 64))
    pts = np.concatenate([column, away, LC.cloud(64, seed=1, lat=(-5.0, 5.0), lon=(-5.0, 5.0))])
    for lateral in ("cell", "bilinear"):
        _, layer, _, nout = _check(ctx, pts, (lat, lon, bounds, values), lateral)
        assert set(layer[:64]) == {-1, 0, 1, 2, 3} and (layer[64:128] == -1).all() and nout >= 64
        assert (np.diff(layer[:64][layer[:64] >= 0]) >= 0).all()


def test_pick_by_element_on_a_shared_interface(ctx):
    """Two elements share the nodes on a flat interface at 10 km: each copy takes the side of its own element, and every
    node of an element gets its centre's layer."""
    lat, lon = np.array([-5.0, 5.0]), np.array([-5.0, 5.0])
    bounds = np.ascontiguousarray(np.broadcast_to([0.0, 10000.0, 30000.0], (2, 2, 3)))
    values = np.ascontiguousarray(np.broadcast_to(np.array([[3000.0], [4500.0]]), (2, 2, 2, 1)))
    la, lo = np.meshgrid([-1.0, 0.0, 1.0], [-1.0, 0.0, 1.0], indexing="ij")
    def element(depths):
        return np.concatenate([LC.xyz(la.ravel(), lo.ravel(), d) for d in depths])
    # the shared face is at radius 6361000 exactly in both copies: the same bits
    pts = np.stack([element([2000.0, 6000.0, 10000.0]), element([10000.0, 14000.0, 18000.0])])
    assert np.array_equal(pts[0, 18:], pts[1, :9])
    want, layer, _, nout = _check(ctx, pts, (lat, lon, bounds, values), "bilinear", pick="element")
    assert nout == 0 and (layer[:27] == 0).all() and (layer[27:] == 1).all()
    assert (want[0, :27] == 3000.0).all() and (want[0, 27:] == 4500.0).all()
    _, by_node, _, _ = _check(ctx, pts, (lat, lon, bounds, values), "bilinear", pick="node")
    assert set(by_node[18:27]) <= {0, 1} and np.array_equal(by_node[18:27], by_node[27:36])   # by node the two copies agree


def test_keep_leaves_the_bits_of_outside_nodes(ctx):
    """outside = 2 with five components: out is prefilled with a pattern of NaN payloads, infinities and negative zeros, the
    count starts from a non-zero value and is taken once."""
    lat, lon, bounds, values = LC.regional(5, 5, seed=9)
    pts = LC.cloud(500, seed=9)
    pattern = np.arange(5 * 500, dtype=np.uint64).reshape(5, 500) * np.uint64(0x9E3779B97F4A7C15) | np.uint64(0x7FF0000000000000)
    pattern[:, ::3] = np.array([-0.0, np.inf, 1.5e-310]).view(np.uint64)[np.arange(167) % 3]
    out = ctx.to_device(pattern.view(np.float64))
    count = ctx.to_device(np.array([41], dtype=np.int64))
    res = LY.layered_model_apply(ctx, pts, lat, lon, bounds, values, outside="keep", out=out, want_layers=True,
                                 want_latlondepth=True, noutside=count)
    assert res["out"].ptr == out.ptr
    got, layer = out.numpy().view(np.uint64), res["layer"].numpy()
    _, want_layer, _, nout = LC.model_apply(res["latlondepth"].numpy(), None, lat, lon, bounds, values, outside=LC.KEEP,
                                            out_before=pattern.view(np.float64))
    assert np.array_equal(layer, want_layer) and 0 < nout < 500 and int(count.numpy()[0]) == 41 + nout
    assert np.array_equal(got[:, layer < 0], pattern[:, layer < 0]) and not np.array_equal(got[:, layer >= 0], pattern[:, layer >= 0])


def test_nothing_to_do_is_valid(ctx):
    lat, lon, bounds, values = LC.regional(5, 2)
    res = LY.layered_model_apply(ctx, np.zeros((0, 3)), lat, lon, bounds, values, want_layers=True)
    assert res["out"].shape == (2, 0) and res["layer"].shape == (0,)
    assert LY.layered_model_apply(ctx, np.zeros((0, 8, 3)), lat, lon, bounds, values, pick="element")["out"].shape == (2, 0, 8)
    with pytest.raises(ValueError, match="bounds must be"):
        LY.layered_model_apply(ctx, np.zeros((4, 3)), lat, lon, bounds[:, :4], values)
    with pytest.raises(ValueError, match="values must be"):
        LY.layered_model_apply(ctx, np.zeros((4, 3)), lat, lon, bounds, values[:, :, :2])
    with pytest.raises(ValueError, match="pass out"):
        LY.layered_model_apply(ctx, np.zeros((4, 3)), lat, lon, bounds, values, outside="keep")
    with pytest.raises(ValueError, match="ascending"):
        LY.layered_model_apply(ctx, np.zeros((4, 3)), lat[::-1], lon, bounds, values)


# ------------------------------------------------------------------------------- a caller's stream and caller's tensors
def test_on_a_callers_stream_with_the_callers_tensors_off_alignment(torch):
    """Late producer, early consumer, as tests/test_caller_stream_gpu.py: under a side stream the inputs hold zeros while the
    stream spins, the true values are copied in on that stream, the library is called and its outputs are cloned and
    overwritten right after, with no host synchronisation in between.  Points, tables and outputs are views that start
    8 bytes into their buffers (off 16-byte alignment), as in tests/test_caller_views_gpu.py."""
    lat, lon, bounds, values = LC.regional(5, 3, seed=12)
    pts = LC.elements(40, 27, seed=12)
    n = 40 * 27
    prefilled = _prefill(3, n)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    host = (pts, lat, lon, bounds, values, prefilled)
    staged = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in host]
    torch.cuda.synchronize()

    def view(shape, dtype, fill):
        buffer = torch.full((int(np.prod(shape)) + 1,), fill, dtype=dtype, device="cuda")
        v = buffer[1:].view(tuple(shape))
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v

    with Context(0, stream=side.cuda_stream) as ctx, torch.cuda.stream(side):
        tp, tla, tlo, tb, tv, tout = (view(x.shape, torch.float64, 0.0) for x in host)
        count = view((1,), torch.int64, 10)
        torch.cuda._sleep(30_000_000)
        for t, s in zip((tp, tla, tlo, tb, tv, tout), staged):
            t.copy_(s, non_blocking=True)
        res = LY.layered_model_apply(ctx, tp, tla, tlo, tb, tv, pick="element", outside="keep", out=tout, want_layers=True,
                                     want_span=True, want_latlondepth=True, noutside=count)
        assert res["out"].ptr == tout.data_ptr()
        got = {"out": tout.clone(), "count": count.clone()}
        extra = {k: res[k] for k in ("layer", "span", "latlondepth")}
        tout.fill_(-7.0), count.fill_(-7)
        side.synchronize()
        got = {"out": got["out"].cpu().numpy(), "count": int(got["count"].item()), **{k: a.numpy() for k, a in extra.items()}}
    _, _, _, nout = _compare(got, pts, (lat, lon, bounds, values), "bilinear", "element", "keep", np.nan, False, prefilled, 10)
    assert nout > 0


# ----------------------------------------------------------------------------------------------------- the Python layer
def _user_model(seed=20, periodic=False):
    """A :class:`LayeredModel` given north to south (the preparation flips it), three layers, two parameters."""
    lat, lon, bounds, values = (LC.global_model if periodic else LC.regional)(4, 2, seed=seed)
    if periodic:
        lon, bounds, values = lon[:-1], bounds[:, :-1], values[:, :-1]
    user_bounds = bounds.transpose(2, 0, 1)[:, ::-1]
    user_values = {p: values[..., c].transpose(2, 0, 1)[:, ::-1] for c, p in enumerate(("VSV", "VSH"))}
    return LY.LayeredModel(lat[::-1], lon, user_bounds, user_values, layer_names=["sediment", "upper", "lower"])


def _crust_chunk(order=2):
    return synth.earth_chunk(order=order, nlat=3, nlon=3, radii=(6_311_000.0, 6_351_000.0, 6_373_000.0))


def test_the_drivers_on_a_gll_mesh_a_hex_mesh_and_a_salvus_model(ctx):
    model = _user_model()
    names, bounds, values = model.packed()
    assert names == ["VSV", "VSH"] and model.flipped["latitude"]
    gp = _crust_chunk()["points"]
    E, Pn = gp.shape[:2]
    rng = np.random.default_rng(1)
    old = {p: rng.uniform(3000.0, 5000.0, (E, Pn)) for p in ("VSV", "VSH", "RHO")}
    # evaluate and layer_index: the statement on the device's coordinates
    lld = LY.layered_model_apply(ctx, gp, model.lat, model.lon, bounds, None, want_latlondepth=True)["latlondepth"].numpy()
    for lateral in ("cell", "bilinear"):
        for pick in ("node", "element"):
            dp = LC.element_depth(gp)
            want, wl, ws, nout = LC.model_apply(lld, dp, model.lat, model.lon, bounds, values, LATERALS[lateral], PICKS[pick])
            out, layer, span = LY.evaluate_layered_model(model, GllMesh(gp, 2, {}), lateral=lateral, pick=pick, return_layers=True,
                                                         context=ctx)
            assert out.shape == (2, E, Pn) and layer.shape == (E, Pn) and span.shape == (E, Pn, 2)
            assert LC.same_bits_nan(out.reshape(2, -1), want) and np.array_equal(layer.ravel(), wl) and LC.same_bits_nan(span.reshape(-1, 2), ws)
            l2, s2 = LY.layer_index(model, gp, lateral=lateral, pick=pick, context=ctx)
            assert np.array_equal(l2, layer) and LC.same_bits_nan(s2, span)
            assert 0 < nout < E * Pn
    one = LY.evaluate_layered_model(model, gp.reshape(-1, 3), params="VSH", outside="clamp", context=ctx)
    want, _, _, _ = LC.model_apply(lld, None, model.lat, model.lon, bounds, values[..., 1:], outside=LC.CLAMP)
    assert one.shape == (1, E * Pn) and LC.same_bits_nan(one, want)
    # import onto a GLL mesh: outside nodes keep the mesh's bits, RHO is untouched
    mesh = GllMesh(gp, 2, {p: v.copy() for p, v in old.items()})
    before = np.stack([old[p] for p in names]).reshape(2, -1)
    want, wl, _, nout = LC.model_apply(lld, LC.element_depth(gp), model.lat, model.lon, bounds, values, LC.BILINEAR, LC.ELEMENT,
                                       LC.KEEP, out_before=before)
    assert LY.import_layered_model(model, mesh, context=ctx) == nout and 0 < nout < E * Pn
    for p, w in zip(names, want):
        assert LC.same_bits_nan(mesh.element_nodal_fields[p], w.reshape(E, Pn)), p
    assert LC.same_bits_nan(mesh.element_nodal_fields["RHO"], old["RHO"])
    # a Salvus model in memory: only the named columns change, the return value is the count
    data = np.ascontiguousarray(np.stack([old["RHO"], old["VSH"], old["VSV"]]).transpose(1, 0, 2))
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=gp)
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=data), ["RHO", "VSH", "VSV"])
    assert LY.import_layered_model(model, f, params=["VSV", "VSH"], context=ctx) == nout
    got = np.array(f["MODEL/data"][()])
    assert LC.same_bits_nan(got[:, 2, :], want[0].reshape(E, Pn)) and LC.same_bits_nan(got[:, 1, :], want[1].reshape(E, Pn))
    assert LC.same_bits_nan(got[:, 0, :], old["RHO"])
    with pytest.raises(ValueError, match="not in MODEL/data"):
        LY.import_layered_model(LY.LayeredModel(model.lat, model.lon, model.bounds, {"VPV": model.values["VSV"]}), f, context=ctx)
    # hex8 nodes: P = 1
    points, conn = synth.hex_mesh(6, seed=1, lo=(6.32e6, -3e5, -3e5), hi=(6.372e6, 3e5, 3e5))
    oldh = rng.uniform(3000.0, 5000.0, (2, len(points)))
    hexmesh = HexMesh(points, conn, {"VSV": oldh[0].copy(), "QMU": oldh[1].copy()})
    lldh = LY.layered_model_apply(ctx, points, model.lat, model.lon, bounds, None, want_latlondepth=True)["latlondepth"].numpy()
    wanth, _, _, nouth = LC.model_apply(lldh, None, model.lat, model.lon, bounds, values[..., :1], outside=LC.KEEP, out_before=oldh[:1])
    assert LY.import_layered_model(model, hexmesh, params="VSV", context=ctx) == nouth and 0 < nouth < len(points)
    assert LC.same_bits_nan(hexmesh.nodal_fields["VSV"], wanth[0]) and LC.same_bits_nan(hexmesh.nodal_fields["QMU"], oldh[1])
    # keep needs the fields; fill creates them
    bare = GllMesh(gp, 2, {})
    with pytest.raises(ValueError, match="no field"):
        LY.import_layered_model(model, bare, context=ctx)
    assert bare.element_nodal_fields == {}
    assert LY.import_layered_model(model, bare, outside="fill", fill_value=-1.0, context=ctx) == nout
    assert sorted(bare.element_nodal_fields) == ["VSH", "VSV"] and (bare.element_nodal_fields["VSV"].ravel()[wl < 0] == -1.0).all()


def test_a_crust_over_a_harmonic_mantle(ctx):
    """import_layered_model(outside="keep") after import_harmonic_model on the same mesh: the nodes the crust did not reach
    hold the harmonic model's bits."""
    rng = np.random.default_rng(3)
    L, R = 4, HC.knots(7)
    mask = np.tril(np.ones((L + 1, L + 1), dtype=bool))
    mantle = H.SphericalHarmonicModel(L, R, {p: tuple(np.where(mask, 100.0 * rng.standard_normal((R.size, L + 1, L + 1)), 0.0)
                                                   for _ in range(2)) for p in ("VSV", "VSH")})
    crust = _user_model(seed=21, periodic=True)
    assert crust.periodic and crust.appended
    gp = synth.earth_chunk(order=2, nlat=3, nlon=3, radii=(6_251_000.0, 6_341_000.0, 6_372_000.0))["points"]
    E, Pn = gp.shape[:2]
    mesh = GllMesh(gp, 2, {})
    H.import_harmonic_model(mantle, mesh, extend=True, context=ctx)
    under = {p: mesh.element_nodal_fields[p].copy() for p in ("VSV", "VSH")}
    missed = LY.import_layered_model(crust, mesh, context=ctx)
    layer, _ = LY.layer_index(crust, mesh, pick="element", context=ctx)
    assert missed == (layer < 0).sum() and 0 < missed < E * Pn
    names, bounds, values = crust.packed()
    lld = LY.layered_model_apply(ctx, gp, crust.lat, crust.lon, bounds, None, lon_periodic=True, want_latlondepth=True)["latlondepth"].numpy()
    want, wl, _, _ = LC.model_apply(lld, LC.element_depth(gp), crust.lat, crust.lon, bounds, values, LC.BILINEAR, LC.ELEMENT, LC.KEEP,
                                    out_before=np.stack([under[p] for p in names]).reshape(2, -1))
    assert np.array_equal(layer.ravel(), wl)
    for p, w in zip(names, want):
        got = mesh.element_nodal_fields[p]
        assert LC.same_bits_nan(got, w.reshape(E, Pn)), p
        assert np.array_equal(got[layer < 0].view(np.uint64), under[p][layer < 0].view(np.uint64))
        assert not np.array_equal(got[layer >= 0], under[p][layer >= 0])
