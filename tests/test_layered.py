"""Layered column models without a GPU: the NumPy statement (tests/layered_cases.py) against an analytic model and its own
rules (zero-thickness layers, the bottom, NaN), the extension header against the module's signature table, the argument
errors that are decided before the device is touched, and the host side of :mod:`multimesh_amd.layered` (what the model
refuses, the preparation of its axes, from_thickness, fill_empty_layers, the packed layout)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import layered_cases as LC
from multimesh_amd import helpers
from multimesh_amd import layered as LY
from test_parametrisation import _c_class, _ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multimesh_layered.h")


# ----------------------------------------------------------------------------------------------- the header and the table
def _declared_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    code = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    protos = {}
    for statement in code.split(";"):
        m = re.fullmatch(r"\s*([^()]*?)\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^()]*)\)\s*", re.split(r"[{}]", statement)[-1])
        if m:
            ret, name, params = m.groups()
            protos[name] = (_c_class(ret, is_return=True), [_c_class(p) for p in params.split(",")])
    return protos


def test_the_extension_header_and_the_table_agree():
    protos = _declared_prototypes()
    assert list(protos) == list(LY.SIGNATURES) == ["mm_layered_model_apply"]
    lib = LY.bind()
    assert lib is helpers.load_lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = LY.SIGNATURES[name]
        assert len(params) == len(argtypes) == 22
        assert (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes]) == (ret, params), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert name not in helpers.SIGNATURES and name not in helpers.EXPORTED_SYMBOLS
    text = open(HEADER).read()
    assert int(re.search(r"#define MM_LAYERED_MAX_P (\d+)", text).group(1)) == LY.MAX_P
    assert int(re.search(r"#define MM_LAYERED_MAX_NB (\d+)", text).group(1)) == LY.MAX_NB
    for prefix, table in (("LATERAL", LY.LATERAL), ("PICK", LY.PICK), ("OUTSIDE", LY.OUTSIDE)):
        for name, number in table.items():
            assert int(re.search(rf"#define MM_LAYERED_{prefix}_{name.upper()} (\d+)", text).group(1)) == number
    assert (LC.CELL, LC.BILINEAR, LC.NODE, LC.ELEMENT) == (0, 1, 0, 1) and (LC.FILL, LC.CLAMP, LC.KEEP) == (0, 1, 2)


def test_the_library_exports_the_symbol():
    assert hasattr(helpers.load_lib(), "mm_layered_model_apply")


# --------------------------------------------------------------------------------------------------- argument checks
CTX = C.c_void_p(0x1000)            # a dummy: a refused call never looks at the context
PTS, LAT, LON, BND, VAL, OUT = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000))  # never read


def _call(lib, ctx=CTX, pts=PTS, ngroups=10, P_=8, lat=LAT, nlat=7, lon=LON, nlon=9, periodic=0, bnd=BND, nb=5, val=VAL,
          ncomp=2, lateral=1, pick=0, outside=0, fill=0.0, out=OUT):
    return lib.mm_layered_model_apply(ctx, pts, ngroups, P_, lat, nlat, lon, nlon, periodic, bnd, nb, val, ncomp, lateral, pick,
                                      outside, fill, out, None, None, None, None)


#: every MM_ERR_ARG case of the header; all are decided before the device is touched
REFUSED = {
    "null ctx": dict(ctx=None),
    "negative ngroups": dict(ngroups=-1),
    "ngroups at 2^48": dict(ngroups=1 << 48, P_=1, ncomp=0),
    "P zero": dict(P_=0),
    "P above 256": dict(P_=257),
    "nb one": dict(nb=1),
    "nb zero": dict(nb=0),
    "nb above 256": dict(nb=257),
    "nlat zero": dict(nlat=0),
    "nlon zero": dict(nlon=0),
    "nlon negative": dict(nlon=-3),
    "ncomp negative": dict(ncomp=-1),
    "ncomp at 65536": dict(ncomp=65536),
    "lateral two": dict(lateral=2),
    "lateral negative": dict(lateral=-1),
    "pick two": dict(pick=2),
    "pick negative": dict(pick=-1),
    "outside three": dict(outside=3),
    "outside negative": dict(outside=-1),
    "points at 2^48": dict(ngroups=1 << 39, P_=256, ncomp=0),
    "out at 2^48": dict(ngroups=1 << 44, P_=8, ncomp=2),
    "bounds at 2^48": dict(nlat=1 << 20, nlon=1 << 20, nb=256, ncomp=0),
    "values at 2^48": dict(nlat=1 << 15, nlon=1 << 15, nb=9, ncomp=1 << 15, ngroups=1),
    "null lat": dict(lat=None),
    "null lon": dict(lon=None),
    "null bounds": dict(bnd=None),
    "null values": dict(val=None),
    "null points": dict(pts=None),
    "null out": dict(out=None),
}


def test_the_extent_cases_sit_on_the_limit():
    assert 3 * (1 << 39) * 256 >= 1 << 48 and 2 * (1 << 44) * 8 == 1 << 48
    assert (1 << 20) * (1 << 20) * 256 == 1 << 48
    assert (1 << 15) * (1 << 15) * 8 * (1 << 15) == 1 << 48 and (1 << 15) < 65536 and (1 << 15) * (1 << 15) * 9 < 1 << 48


@pytest.mark.parametrize("what", list(REFUSED))
def test_refuses_without_a_gpu(what):
    lib = LY.bind()
    assert _call(lib, **REFUSED[what]) == -1, what
    message = lib.mm_last_error()
    assert b"mm_layered_model_apply" in message and len(message) > len(b"mm_layered_model_apply: "), message
    assert lib.mm_last_status() == -1


def test_nothing_to_do_is_valid_without_a_gpu():
    """ngroups == 0, and ncomp == 0 with no output asked for: MM_OK before the device is touched."""
    lib = LY.bind()
    assert _call(lib, ngroups=0, pts=None, out=None) == 0
    assert _call(lib, ncomp=0, val=None, out=None) == 0


def test_python_refuses_before_the_library_is_asked():
    class NoDevice:                      # the checks below come before anything of the context is used
        lib = None

    for kw, match in ((dict(lateral="cubic"), "lateral must be one of"), (dict(pick="corner"), "pick must be one of"),
                      (dict(outside="wrap"), "outside must be one of")):
        with pytest.raises(ValueError, match=match):
            LY.layered_model_apply(NoDevice(), np.zeros((4, 3)), [0.0, 1.0], [0.0, 1.0], np.zeros((2, 2, 2)), **kw)


# ------------------------------------------------------------------------------------------------------- the statement
def _lld(lat, lon, depth):
    lat, lon, depth = np.broadcast_arrays(np.asarray(lat, dtype=float), np.asarray(lon, dtype=float), np.asarray(depth, dtype=float))
    return np.stack([lat.ravel(), lon.ravel(), depth.ravel()], axis=1)


def test_an_analytic_moho():
    """Two interfaces over a flat top: a Moho at 30 km + 10 km sin(lat) on the map nodes, linear in latitude between them;
    crust and mantle values linear in latitude too.  Bilinear mode on nodes midway between the map nodes gives the analytic
    layer and value to 1e-9 relative."""
    lat, lon = np.linspace(-60.0, 60.0, 25), np.linspace(0.0, 40.0, 5)
    moho = 30000.0 + 10000.0 * np.sin(np.deg2rad(lat))
    bounds = np.zeros((lat.size, lon.size, 3))
    bounds[:, :, 1] = moho[:, None]
    bounds[:, :, 2] = 200000.0
    values = np.zeros((lat.size, lon.size, 2, 1))
    values[:, :, 0, 0] = (3000.0 + 10.0 * lat)[:, None]
    values[:, :, 1, 0] = (4500.0 - 5.0 * lat)[:, None]
    mid_lat, mid_lon = 0.5 * (lat[:-1] + lat[1:]), 0.5 * (lon[:-1] + lon[1:])
    la, lo, de = np.meshgrid(mid_lat, mid_lon, np.linspace(1000.0, 190000.0, 64), indexing="ij")
    lld = _lld(la, lo, de)
    out, layer, span, nout = LC.model_apply(lld, None, lat, lon, bounds, values)
    moho_mid = np.repeat(0.5 * (moho[:-1] + moho[1:]), mid_lon.size * 64)
    far = np.abs(lld[:, 2] - moho_mid) > 1e-9 * moho_mid              # (no node sits on the Moho within rounding)
    assert far.all() and nout == 0
    want_layer = (lld[:, 2] >= moho_mid).astype(np.int32)
    assert np.array_equal(layer, want_layer) and 0 < want_layer.sum() < want_layer.size
    want = np.where(want_layer == 0, 3000.0 + 10.0 * lld[:, 0], 4500.0 - 5.0 * lld[:, 0])
    assert np.abs(out[0] - want).max() <= 1e-9 * np.abs(want).max()
    assert np.abs(span[want_layer == 0, 1] - moho_mid[want_layer == 0]).max() <= 1e-9 * 40000.0
    assert np.abs(span[want_layer == 1, 0] - moho_mid[want_layer == 1]).max() <= 1e-9 * 40000.0
    assert (span[want_layer == 0, 0] == 0.0).all() and (span[want_layer == 1, 1] == 200000.0).all()


def _one_column(b, v=None):
    """A 1 x 1 map (both axes of length 1: constant) with the bounds ``b`` and the values ``v`` per layer."""
    b = np.asarray(b, dtype=float)
    v = np.arange(1.0, b.size) if v is None else np.asarray(v, dtype=float)
    return np.array([0.0]), np.array([0.0]), b.reshape(1, 1, -1), v.reshape(1, 1, -1, 1)


def _layers(depths, b, outside=LC.FILL, lateral=LC.BILINEAR):
    lat, lon, bounds, values = _one_column(b)
    out, layer, span, nout = LC.model_apply(_lld(0.0, 0.0, depths), None, lat, lon, bounds, values, lateral=lateral,
                                            outside=outside, fill=-1.0)
    assert nout == (layer < 0).sum() and np.array_equal(out[0], np.where(layer >= 0, layer + 1.0, -1.0))
    assert np.isnan(span[layer < 0]).all() and (np.isnan(b).any() or not np.isnan(span[layer >= 0]).any())
    return list(layer)


@pytest.mark.parametrize("lateral", (LC.CELL, LC.BILINEAR))
def test_zero_thickness_layers_are_skipped_and_the_bottom_belongs_to_the_model(lateral):
    b = [0.0, 10.0, 10.0, 20.0, 20.0]                    # layers 1 and 3 are empty
    depths = [-1.0, 0.0, 5.0, 10.0, 15.0, 20.0, 20.5]
    assert _layers(depths, b, lateral=lateral) == [-1, 0, 0, 2, 2, 2, -1]        # 10 is layer 2's top; 20, the bottom: the last thick one
    assert _layers(depths, b, LC.CLAMP, lateral) == [0, 0, 0, 2, 2, 2, 2]
    assert _layers(depths, [0.0, 0.0, 10.0, 20.0, 30.0], LC.CLAMP, lateral)[0] == 1    # above the top: the first thick one
    empty = [5.0, 5.0, 5.0]                              # a column without a layer: outside in every mode
    for mode in (LC.FILL, LC.CLAMP, LC.KEEP):
        lat, lon, bounds, values = _one_column(empty)
        before = np.full((1, 3), 7.0)
        out, layer, _, nout = LC.model_apply(_lld(0.0, 0.0, [0.0, 5.0, 9.0]), None, lat, lon, bounds, values, lateral=lateral,
                                             outside=mode, fill=-1.0, out_before=before)
        assert list(layer) == [-1, -1, -1] and nout == 3 and (out == (7.0 if mode == LC.KEEP else -1.0)).all()


def test_nan_nodes_and_nan_bounds():
    b = [0.0, np.nan, 20.0, 30.0]                        # a NaN bound never stops the scan
    assert _layers([5.0, 25.0, 30.0, np.nan], b) == [1, 2, 2, -1]
    assert _layers([5.0, 25.0, np.nan], b, LC.CLAMP) == [1, 2, -1]
    assert _layers([5.0], [np.nan, 10.0, 20.0]) == [-1] and _layers([5.0], [np.nan, 10.0, 20.0], LC.CLAMP) == [-1]
    lat, lon, bounds, values = LC.regional(nb=5, ncomp=2)
    lld = _lld([0.0, np.nan, 0.0, 0.0, 9.0], [0.0, 0.0, np.nan, 0.0, 0.0], [20000.0, 20000.0, 20000.0, np.nan, 20000.0])
    for mode in (LC.FILL, LC.CLAMP):
        out, layer, span, nout = LC.model_apply(lld, None, lat, lon, bounds, values, outside=mode, fill=-5.0)
        assert layer[0] >= 0 and list(layer[1:4]) == [-1, -1, -1] and (layer[4] >= 0) == (mode == LC.CLAMP)
        assert (out[:, 1:4] == -5.0).all() and np.isnan(span[1:4]).all() and nout == (4 if mode == LC.FILL else 3)


def test_pick_by_element_reads_the_centres_depth():
    lat, lon, bounds, values = _one_column([0.0, 10000.0, 20000.0])
    up = LC.xyz(0.0, 0.0, [[10000.0, 6000.0, 2000.0]])          # two elements share the node at 10 km
    down = LC.xyz(0.0, 0.0, [[10000.0, 14000.0, 18000.0]])
    pts = np.concatenate([up, down])
    dp = LC.element_depth(pts)
    assert dp.shape == (6,) and np.abs(dp - np.repeat([6000.0, 14000.0], 3)).max() < 1e-6
    lld = LC.latlondepth(pts)
    _, layer, _, _ = LC.model_apply(lld, dp, lat, lon, bounds, values, pick=LC.ELEMENT)
    assert list(layer) == [0, 0, 0, 1, 1, 1]


# ------------------------------------------------------------------------------------------------- the host side of the module
def _user_model(nb=4, seed=0, nlat=5, nlon=6):
    rng = np.random.default_rng(seed)
    lat, lon = np.linspace(-10.0, 10.0, nlat), np.linspace(20.0, 45.0, nlon)
    top = rng.uniform(-2000.0, 1000.0, (nlat, nlon))
    thickness = rng.uniform(1000.0, 9000.0, (nb - 1, nlat, nlon))
    bounds = np.concatenate([top[None], top[None] + np.cumsum(thickness, axis=0)])
    values = {"VP": rng.uniform(5000.0, 8000.0, (nb - 1, nlat, nlon)), "RHO": rng.uniform(2000.0, 3300.0, (nb - 1, nlat, nlon))}
    return lat, lon, top, thickness, bounds, values


def test_what_the_model_refuses():
    lat, lon, top, thickness, bounds, values = _user_model()
    for bad_lat, match in ((np.array([0.0, 1.0, 1.0, 2.0, 3.0]), "not strictly monotone"), (np.array([0.0, 1.0, np.nan, 3.0, 4.0]), "finite")):
        with pytest.raises(ValueError, match=match):
            LY.LayeredModel(bad_lat, lon, bounds, values)
    with pytest.raises(ValueError, match="not strictly monotone"):
        LY.LayeredModel(lat, lon[[0, 2, 1, 3, 4, 5]], bounds, values)
    nan = bounds.copy()
    nan[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="bounds must be finite"):
        LY.LayeredModel(lat, lon, nan, values)
    down = bounds.copy()
    down[2, 1, 1] = down[1, 1, 1] - 1.0
    with pytest.raises(ValueError, match="decrease downwards"):
        LY.LayeredModel(lat, lon, down, values)
    with pytest.raises(ValueError, match=r"bounds must be \[nb, 5, 6\]"):
        LY.LayeredModel(lat, lon, bounds[:, :4], values)
    with pytest.raises(ValueError, match=r"bounds must be \[nb, 5, 6\]"):
        LY.LayeredModel(lat, lon, bounds[:1], {})
    with pytest.raises(ValueError, match=r"values\['VP'\] must be \(3, 5, 6\)"):
        LY.LayeredModel(lat, lon, bounds, {"VP": values["VP"][:2]})
    with pytest.raises(ValueError, match="layer_names"):
        LY.LayeredModel(lat, lon, bounds, values, layer_names=["a", "b"])
    model = LY.LayeredModel(lat, lon, bounds, values, layer_names=["sediment", "upper", "lower"])
    assert model.parameters == ["VP", "RHO"] and model.nb == 4 and model.nlayer == 3 and not model.periodic
    with pytest.raises(ValueError, match=r"has no \['VS'\]"):
        model.packed(["VS"])
    with pytest.raises(ValueError, match="outside must be one of"):
        LY.import_layered_model(model, None, outside="wrap")
    with pytest.raises(ValueError, match="keep"):
        LY.evaluate_layered_model(model, np.zeros((3, 3)), outside="keep")
    with pytest.raises(ValueError, match="thickness is negative"):
        LY.LayeredModel.from_thickness(lat, lon, top, -thickness, values)


def test_a_flipped_latitude_and_a_global_longitude_are_prepared():
    """A model given north to south on a 0 .. 330 longitude axis is the model given south to north with its closing column."""
    rng = np.random.default_rng(4)
    lat, lon = np.linspace(-90.0, 90.0, 7), np.arange(0.0, 360.0, 30.0)
    top = rng.uniform(-2000.0, 1000.0, (7, 12))
    bounds = np.concatenate([top[None], top[None] + np.cumsum(rng.uniform(1000.0, 9000.0, (3, 7, 12)), axis=0)])
    values = {"VS": rng.uniform(3000.0, 4500.0, (3, 7, 12))}
    given = LY.LayeredModel(lat[::-1], lon, bounds[:, ::-1], {"VS": values["VS"][:, ::-1]})
    assert given.flipped == {"latitude": True, "longitude": False} and given.periodic and given.appended
    closed_lon = np.concatenate([lon, [360.0]])
    close = lambda a: np.concatenate([a, a[..., :1]], axis=-1)
    prepared = LY.LayeredModel(lat, closed_lon, close(bounds), {"VS": close(values["VS"])})
    assert prepared.periodic and not prepared.appended and prepared.flipped == {"latitude": False, "longitude": False}
    assert np.array_equal(given.lat, lat) and np.array_equal(given.lon, closed_lon) and np.array_equal(prepared.lon, closed_lon)
    assert np.array_equal(given.bounds, close(bounds)) and np.array_equal(prepared.bounds, close(bounds))
    assert np.array_equal(given.values["VS"], prepared.values["VS"])
    # ... and the statement gives the same values on both
    lld = _lld(rng.uniform(-90, 90, 200), rng.uniform(0, 360, 200), rng.uniform(-3000, 30000, 200))
    a = LC.model_apply(lld, None, given.lat, given.lon, *given.packed()[1:])
    b = LC.model_apply(lld, None, prepared.lat, prepared.lon, *prepared.packed()[1:])
    assert all(LC.same_bits_nan(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] < 200
    regional = LY.LayeredModel(lat, lon[:5], bounds[:, :, :5], {})
    assert not regional.periodic and not regional.appended and regional.lon.size == 5


def test_from_thickness():
    lat, lon, top, thickness, bounds, values = _user_model()
    model = LY.LayeredModel.from_thickness(lat, lon, top, thickness, values)
    assert np.array_equal(model.bounds, bounds) and np.array_equal(model.bounds[2], top + (thickness[0] + thickness[1]))
    zero = thickness.copy()
    zero[1, :2] = 0.0
    pinched = LY.LayeredModel.from_thickness(lat, lon, top, zero, values)
    assert np.array_equal(pinched.bounds[1, :2], pinched.bounds[2, :2])
    with pytest.raises(ValueError, match="thickness must be"):
        LY.LayeredModel.from_thickness(lat, lon, top, thickness[:, :3], values)


def test_packed_round_trips_to_the_user_layout():
    lat, lon, _, _, bounds, values = _user_model()
    model = LY.LayeredModel(lat, lon, bounds, values)
    names, b, v = model.packed()
    assert names == ["VP", "RHO"] and b.shape == (5, 6, 4) and v.shape == (5, 6, 3, 2)
    assert b.flags.c_contiguous and v.flags.c_contiguous
    assert np.array_equal(b.transpose(2, 0, 1), bounds)
    assert np.array_equal(v[..., 0].transpose(2, 0, 1), values["VP"]) and np.array_equal(v[..., 1].transpose(2, 0, 1), values["RHO"])
    names, b, v = model.packed("RHO")
    assert names == ["RHO"] and np.array_equal(v[..., 0].transpose(2, 0, 1), values["RHO"])
    names, b, v = model.packed([])
    assert names == [] and v.shape == (5, 6, 3, 0) and np.array_equal(b.transpose(2, 0, 1), bounds)


@pytest.mark.parametrize("wrapped", (False, True))
def test_fill_empty_layers(wrapped):
    """A 4 x 4 map, layer 0 pinched out in the column (1, 0) on the map's western edge: its value becomes the mean of its
    neighbours -- five of them on a plain map, eight when the longitude wraps."""
    lat = np.array([-30.0, -10.0, 10.0, 30.0])
    lon = np.array([0.0, 90.0, 180.0, 270.0]) if wrapped else np.array([0.0, 10.0, 20.0, 30.0])
    bounds = np.zeros((3, 4, 4))
    bounds[1], bounds[2] = 1000.0, 5000.0
    bounds[1, 1, 0] = 0.0
    v = np.arange(32.0).reshape(2, 4, 4)
    v[0, 1, 0] = -999.0
    model = LY.LayeredModel(lat, lon, bounds, {"VS": v})
    assert model.periodic == wrapped and model.appended == wrapped
    filled = model.fill_empty_layers()
    near = [(0, 0), (0, 1), (1, 1), (2, 0), (2, 1)] + ([(0, 3), (1, 3), (2, 3)] if wrapped else [])
    want = np.mean([v[0][j, i] for j, i in near])
    assert filled.values["VS"][0, 1, 0] == want and model.values["VS"][0, 1, 0] == -999.0
    if wrapped:
        assert filled.values["VS"].shape == (2, 4, 5) and filled.values["VS"][0, 1, 4] == want
        assert np.array_equal(filled.values["VS"][..., 0], filled.values["VS"][..., 4])
    untouched = np.ones((4, 4), dtype=bool)
    untouched[1, 0] = False
    assert np.array_equal(filled.values["VS"][0, :, :4][untouched], v[0][untouched]) and np.array_equal(filled.values["VS"][1, :, :4], v[1])
    assert np.array_equal(filled.bounds, model.bounds) and filled.periodic == model.periodic
    # two rounds: a pinched column whose neighbours are pinched too is reached through them
    bounds[1, 0, :2], bounds[1, 1, :2] = 0.0, 0.0
    twice = LY.LayeredModel(lat, lon, bounds, {"VS": v}, lon_periodic=False).fill_empty_layers().values["VS"][0]
    first = np.mean([v[0][0, 2], v[0][1, 2]])            # (0, 1) sees (0, 2) and (1, 2) in the first round
    assert twice[0, 1] == first and np.isfinite(twice[:2, :2]).all() and (twice[:2, :2] != -999.0).all()
    # a layer that is empty everywhere stays as it is
    bounds[1] = 0.0
    same = LY.LayeredModel(lat, lon, bounds, {"VS": v}).fill_empty_layers()
    assert np.array_equal(same.values["VS"][..., :4], v)
