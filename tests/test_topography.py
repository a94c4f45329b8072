"""Topography without a GPU: the extension header against the module's signature table, the argument errors that are decided
before the device is touched, the host side of :mod:`multimesh_amd.topography` (what InterfaceMap refuses, the preparation of
its axes, the three constructors), and the NumPy statement (tests/topography_cases.py) against its own properties, against
the same expressions in extended precision, and through the round trip flatten(apply(rho)); the edges the guarded cases hold
are counted here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guarded_cases as G
import topography_cases as TC
from multimesh_amd import helpers
from multimesh_amd import layered as LY
from multimesh_amd import topography as TP
from multimesh_amd.api import GllMesh
from test_parametrisation import _c_class, _ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multimesh_topography.h")
ULP = float(np.spacing(6.4e6))          # 9.3e-10 m: one unit in the last place of a radius

#: The largest error of flatten(apply(rho)) that the float64 NumPy statement makes on :func:`_round_trip_inputs` (columns whose
#: deformed layers are at least 500 m thick, (A_j - A_{j+1}) / (B_j - B_{j+1}) at most 12), measured: 3 ulps of 6.4e6.
ROUND_TRIP_MEASURED = 2.7939677238464355e-09
#: ... and what the tests allow: four times that, to cover other seeds and map shapes (the GPU drivers are held to it too).
ROUND_TRIP_BOUND = 4.0 * ROUND_TRIP_MEASURED
WORST_RATIO = 12.0                      # 6000 m of reference layer over 500 m of deformed layer


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
    assert list(protos) == list(TP.SIGNATURES) == ["mm_radial_stretch"]
    lib = TP.bind()
    assert lib is helpers.load_lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = TP.SIGNATURES[name]
        assert len(params) == len(argtypes) == 19
        assert (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes]) == (ret, params), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert name not in helpers.SIGNATURES and name not in helpers.EXPORTED_SYMBOLS
    text = open(HEADER).read()
    assert int(re.search(r"#define MM_STRETCH_MAX_NA (\d+)", text).group(1)) == TP.MAX_NA == TC.MAX_NA
    for prefix, table in (("DIRECTION", TP.DIRECTION), ("LATERAL", TP.LATERAL), ("OUTSIDE", TP.OUTSIDE)):
        for name, number in table.items():
            assert int(re.search(rf"#define MM_STRETCH_{prefix}_{name.upper()} (\d+)", text).group(1)) == number
    assert (TC.APPLY, TC.FLATTEN, TC.CELL, TC.BILINEAR, TC.KEEP, TC.CLAMP) == (0, 1, 0, 1, 0, 1)


def test_the_library_exports_the_symbol():
    assert hasattr(helpers.load_lib(), "mm_radial_stretch")


# --------------------------------------------------------------------------------------------------- argument checks
CTX = C.c_void_p(0x1000)            # a dummy: a refused call never looks at the context
PTS, REF, LAT, LON, ANC, SHF, OUT = (C.c_void_p(a) for a in (0x100000, 0x180000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000))


def _call(lib, ctx=CTX, pts=PTS, n=10, ref=None, lat=LAT, nlat=7, lon=LON, nlon=9, periodic=0, anc=ANC, na=5, shf=SHF,
          direction=0, lateral=1, outside=0, out=OUT):
    return lib.mm_radial_stretch(ctx, pts, n, ref, lat, nlat, lon, nlon, periodic, anc, na, shf, direction, lateral, outside,
                                 out, None, None, None)


#: every MM_ERR_ARG case of the header; all are decided before the device is touched
REFUSED = {
    "null ctx": dict(ctx=None),
    "negative n": dict(n=-1),
    "points at 2^48": dict(n=-(-(1 << 48) // 3)),
    "na one": dict(na=1),
    "na zero": dict(na=0),
    "na above 64": dict(na=65),
    "nlat zero": dict(nlat=0),
    "nlon zero": dict(nlon=0),
    "nlon negative": dict(nlon=-3),
    "shifts at 2^48": dict(nlat=1 << 21, nlon=1 << 21, na=64),
    "direction two": dict(direction=2),
    "direction negative": dict(direction=-1),
    "lateral two": dict(lateral=2),
    "lateral negative": dict(lateral=-1),
    "outside two": dict(outside=2),
    "outside negative": dict(outside=-1),
    "null lat": dict(lat=None),
    "null lon": dict(lon=None),
    "null anchors": dict(anc=None),
    "null shifts": dict(shf=None),
    "null points": dict(pts=None),
    "ref_radius with flatten": dict(ref=REF, direction=1),
}


def test_the_extent_cases_sit_on_the_limit():
    n = -(-(1 << 48) // 3)
    assert 3 * n >= 1 << 48 > 3 * (n - 1) and (1 << 21) * (1 << 21) * 64 == 1 << 48


@pytest.mark.parametrize("what", list(REFUSED))
def test_refuses_without_a_gpu(what):
    lib = TP.bind()
    assert _call(lib, **REFUSED[what]) == -1, what
    message = lib.mm_last_error()
    assert b"mm_radial_stretch" in message and len(message) > len(b"mm_radial_stretch: "), message
    assert lib.mm_last_status() == -1


def test_nothing_to_do_is_valid_without_a_gpu():
    """n == 0, and a call that asks for no output: MM_OK before the device is touched."""
    lib = TP.bind()
    assert _call(lib, n=0, pts=None, out=None) == 0
    assert _call(lib, out=None) == 0


def test_python_refuses_before_the_library_is_asked():
    class NoDevice:                      # the checks below come before anything of the context is used
        lib = None

    for kw, match in ((dict(direction="invert"), "direction must be one of"), (dict(lateral="cubic"), "lateral must be one of"),
                      (dict(outside="fill"), "outside must be one of")):
        with pytest.raises(ValueError, match=match):
            TP.radial_stretch(NoDevice(), np.zeros((4, 3)), [0.0, 1.0], [0.0, 1.0], [2.0, 1.0], np.zeros((2, 2, 2)), **kw)
    imap = TP.InterfaceMap.from_surface([0.0, 1.0], [0.0, 1.0], np.zeros((2, 2)))
    for call in (TP.apply_topography, TP.remove_topography, TP.reference_radius, TP.attach_z_node_1d):
        with pytest.raises(ValueError, match="lateral must be one of"):
            call(np.zeros((4, 3)), imap, lateral="cubic")
    with pytest.raises(ValueError, match="reference must be"):
        TP.apply_topography(GllMesh(np.ones((1, 8, 3)), 1, {}), imap, reference="depth")
    with pytest.raises(ValueError, match="no z_node_1D"):
        TP.apply_topography(GllMesh(np.ones((1, 8, 3)), 1, {}), imap)


# -------------------------------------------------------------------------------------------------------- InterfaceMap
def _user_map(na=3, nlat=5, nlon=6, seed=0):
    rng = np.random.default_rng(seed)
    lat, lon = np.linspace(-10.0, 10.0, nlat), np.linspace(20.0, 45.0, nlon)
    anchors = TC.anchor_radii(na, 20000.0)
    shifts = rng.uniform(-3000.0, 3000.0, (na, nlat, nlon))
    return lat, lon, anchors, shifts


def test_what_the_map_refuses():
    lat, lon, anchors, shifts = _user_map()
    for bad_lat, match in ((np.array([0.0, 1.0, 1.0, 2.0, 3.0]), "not strictly monotone"), (np.array([0.0, 1.0, np.nan, 3.0, 4.0]), "finite")):
        with pytest.raises(ValueError, match=match):
            TP.InterfaceMap(bad_lat, lon, anchors, shifts)
    for bad, match in ((anchors[::-1], "strictly descending"), ([anchors[0], anchors[0], anchors[2]], "strictly descending"),
                       ([anchors[0], np.inf, anchors[2]], "finite"), (anchors[:1], "anchors must be"),
                       (np.linspace(7e6, 6e6, 65), "anchors must be")):
        with pytest.raises(ValueError, match=match):
            TP.InterfaceMap(lat, lon, bad, shifts if len(bad) == 3 else np.zeros((len(bad), 5, 6)))
    nan = shifts.copy()
    nan[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="shifts must be finite"):
        TP.InterfaceMap(lat, lon, anchors, nan)
    with pytest.raises(ValueError, match=r"shifts must be \(3, 5, 6\)"):
        TP.InterfaceMap(lat, lon, anchors, shifts[:, :4])
    # crossing interfaces: the error names the worst column
    crossed = shifts.copy()
    crossed[1, 1, 1] = shifts[0, 1, 1] + (anchors[0] - anchors[1]) + 5.0        # B_1 five metres above B_0
    crossed[2, 3, 4] = crossed[1, 3, 4] + (anchors[1] - anchors[2]) + 70.0      # B_2 seventy metres above B_1: the worst
    with pytest.raises(ValueError, match=rf"interfaces cross: at lat {lat[3]:g}, lon {lon[4]:g} interface 2 lies 70 m above interface 1"):
        TP.InterfaceMap(lat, lon, anchors, crossed)
    touching = shifts.copy()
    touching[0, 0, 0], touching[1, 0, 0] = 0.0, anchors[0] - anchors[1]         # B_1 == B_0: a layer of no thickness cannot be inverted
    assert anchors[1] + touching[1, 0, 0] == anchors[0] + touching[0, 0, 0]
    with pytest.raises(ValueError, match="interfaces cross"):
        TP.InterfaceMap(lat, lon, anchors, touching)
    imap = TP.InterfaceMap(lat, lon, anchors, shifts)
    assert imap.na == 3 and not imap.periodic and not imap.appended and imap.packed().shape == (5, 6, 3)
    assert imap.packed().flags.c_contiguous and np.array_equal(imap.packed().transpose(2, 0, 1), shifts)


def test_a_flipped_latitude_and_a_global_longitude_are_prepared():
    """A map given north to south on a 0 .. 330 longitude axis is the map given south to north with its closing column."""
    rng = np.random.default_rng(4)
    lat, lon = np.linspace(-90.0, 90.0, 7), np.arange(0.0, 360.0, 30.0)
    anchors = TC.anchor_radii(3, 20000.0)
    shifts = rng.uniform(-3000.0, 3000.0, (3, 7, 12))
    given = TP.InterfaceMap(lat[::-1], lon, anchors, shifts[:, ::-1])
    assert given.flipped == {"latitude": True, "longitude": False} and given.periodic and given.appended
    closed_lon = np.concatenate([lon, [360.0]])
    close = lambda a: np.concatenate([a, a[..., :1]], axis=-1)
    prepared = TP.InterfaceMap(lat, closed_lon, anchors, close(shifts))
    assert prepared.periodic and not prepared.appended and prepared.flipped == {"latitude": False, "longitude": False}
    assert np.array_equal(given.lat, lat) and np.array_equal(given.lon, closed_lon) and np.array_equal(prepared.lon, closed_lon)
    assert np.array_equal(given.shifts, close(shifts)) and np.array_equal(prepared.shifts, close(shifts))
    # ... and the statement gives the same on both
    pts = TC.sphere_cloud(300, anchors, seed=1)
    lld, r = TC.device_view(pts, closed_lon, True)
    a = TC.stretch(lld, r, pts, None, given.lat, given.lon, given.anchors, given.packed())
    b = TC.stretch(lld, r, pts, None, prepared.lat, prepared.lon, prepared.anchors, prepared.packed())
    assert TC.same_bits_nan(a[0], b[0]) and TC.same_bits_nan(a[1], b[1]) and a[2] == b[2] == 0
    regional = TP.InterfaceMap(lat, lon[:5], anchors, shifts[:, :, :5])
    assert not regional.periodic and not regional.appended and regional.lon.size == 5


def test_the_constructors():
    lat, lon, anchors, shifts = _user_map()
    elevation = shifts[0]
    surface = TP.InterfaceMap.from_surface(lat, lon, elevation)
    assert list(surface.anchors) == [6371000.0, 6071000.0]
    assert np.array_equal(surface.shifts[0], elevation) and not surface.shifts[1].any()
    assert list(TP.InterfaceMap.from_surface(lat, lon, elevation, taper_radius=6_171_000.0).anchors) == [6371000.0, 6171000.0]
    with pytest.raises(ValueError, match="strictly descending"):
        TP.InterfaceMap.from_surface(lat, lon, elevation, taper_radius=6_371_000.0)
    radii = anchors[:, None, None] + shifts
    by_radii = TP.InterfaceMap.from_radii(lat, lon, anchors, radii)
    assert np.array_equal(by_radii.shifts, radii - anchors[:, None, None]) and np.abs(by_radii.shifts - shifts).max() < 1e-8
    with pytest.raises(ValueError, match="radii must be"):
        TP.InterfaceMap.from_radii(lat, lon, anchors, radii[:2])


def test_from_layered_against_a_hand_computed_map():
    """A 2 x 2 layered model with four interfaces; the surface (index 0, 1-D depth 0) and the Moho (index 3, 1-D depth
    24 400 m) are honoured.  The shift of an anchor is how far the model's interface lies ABOVE its 1-D depth."""
    lat, lon = np.array([0.0, 10.0]), np.array([20.0, 30.0])
    top = np.array([[-1000.0, 0.0], [500.0, 2000.0]])                     # depths: -1000 is 1 km ABOVE 6371 km
    moho = np.array([[30000.0, 24400.0], [20000.0, 41000.0]])
    bounds = np.stack([top, top + 3000.0, top + 9000.0, moho])
    model = LY.LayeredModel(lat, lon, bounds, {})
    imap = TP.InterfaceMap.from_layered(model, {3: 24400.0, 0: 0.0})
    assert list(imap.anchors) == [6371000.0, 6346600.0]
    assert np.array_equal(imap.shifts[0], [[1000.0, 0.0], [-500.0, -2000.0]])
    assert np.array_equal(imap.shifts[1], [[-5600.0, 0.0], [4400.0, -16600.0]])
    tapered = TP.InterfaceMap.from_layered(model, {0: 0.0, 3: 24400.0}, taper_radius=6_071_000.0)
    assert list(tapered.anchors) == [6371000.0, 6346600.0, 6071000.0] and not tapered.shifts[2].any()
    assert np.array_equal(tapered.shifts[:2], imap.shifts)
    for bad in ({}, {4: 0.0}, {-1: 0.0}):
        with pytest.raises(ValueError, match="interfaces must map"):
            TP.InterfaceMap.from_layered(model, bad)
    # a model given north to south: the map is prepared as the model was
    flipped = LY.LayeredModel(lat[::-1], lon, bounds[:, ::-1], {})
    assert np.array_equal(TP.InterfaceMap.from_layered(flipped, {0: 0.0, 3: 24400.0}).shifts, imap.shifts)


# ------------------------------------------------------------------------------------------------------- the statement
def _on_host(pts, model, periodic=False, **kw):
    lat, lon, anchors, shifts = model
    lld, r = TC.device_view(pts, lon, periodic)
    return TC.stretch(lld, r, pts, kw.pop("ref", None), lat, lon, anchors, shifts, **kw)


@pytest.mark.parametrize("lateral", (TC.CELL, TC.BILINEAR))
def test_a_zero_shift_map_leaves_the_points_bit_identical(lateral):
    lat, lon, anchors, shifts = TC.global_map(5, seed=1)
    zero = np.zeros_like(shifts)
    zero[..., 1] = -0.0
    pts = TC.sphere_cloud(4000, anchors, seed=2)
    pts[:4] = [[0.0, 0.0, 0.0], [np.nan, 1.0, 2.0], [-0.0, 0.0, anchors[1]], [anchors[0], -0.0, 0.0]]
    out, rad, nout = _on_host(pts, (lat, lon, anchors, zero), True, lateral=lateral)
    assert np.array_equal(out.view(np.uint64), pts.view(np.uint64)) and nout == 2
    assert TC.same_bits_nan(rad, TC.radius(pts))
    # flattening interpolates between the anchors, lerp(u, A_{j+1}, A_j): the radius comes back within its roundings, not its bits
    out, rad, nout = _on_host(pts, (lat, lon, anchors, zero), True, direction=TC.FLATTEN, lateral=lateral)
    assert nout == 2 and np.nanmax(np.abs(rad - TC.radius(pts))) <= 2 * ULP and np.nanmax(np.abs(out - pts)) <= 3 * ULP


def test_outside_nodes_keep_their_bits_and_are_counted():
    model = TC.regional(5, seed=3)
    pts = TC.cloud(3000, model[2], seed=4)
    pts[:3] = [[0.0, 0.0, 0.0], [np.nan, 1.0, 2.0], [1.0, np.nan, np.nan]]
    lld, r = TC.device_view(pts, model[1], False)
    off = ~((lld[:, 0] >= -6.0) & (lld[:, 0] <= 6.0) & (lld[:, 1] >= -5.5) & (lld[:, 1] <= 6.5)) | ~(r > 0)
    for direction in (TC.APPLY, TC.FLATTEN):
        out, rad, nout = _on_host(pts, model, direction=direction)
        assert nout == off.sum() and 3 < nout < len(pts)
        assert np.array_equal(out[off].view(np.uint64), pts[off].view(np.uint64)) and TC.same_bits_nan(rad[off], r[off])
        assert (out[~off] != pts[~off]).any(axis=1).all()
        out, rad, nout = _on_host(pts, model, direction=direction, outside=TC.CLAMP)
        assert nout == 3 and np.array_equal(out[:3].view(np.uint64), pts[:3].view(np.uint64))
        assert (out[3:] != pts[3:]).any(axis=1).all()


def test_apply_is_strictly_monotone_along_a_column():
    for lat, lon, anchors, shifts in (TC.regional(5, seed=5), TC.global_map(64, seed=6, spacing=3000.0)):
        for s in shifts.reshape(-1, len(anchors))[::7]:
            rho = np.sort(np.concatenate([np.linspace(anchors[-1] - 5000.0, anchors[0] + 5000.0, 4001), anchors]))
            rho = rho[np.diff(rho, prepend=0.0) > 0]
            moved = TC.displace(rho, anchors, np.broadcast_to(s, (len(rho), len(s))), TC.APPLY)
            assert (np.diff(moved) > 0).all()


def test_anchors_land_on_their_interfaces_and_the_top_moves_rigidly():
    lat, lon, anchors, shifts = TC.regional(5, seed=7)
    s = shifts.reshape(-1, 5)
    for j, a in enumerate(anchors):
        moved = TC.displace(np.full(len(s), a), anchors, s, TC.APPLY)
        assert np.array_equal(moved, a + s[:, j])                     # B_j exactly: the one rounding of A_j + s_j
        back = TC.displace(moved, anchors, s, TC.FLATTEN)               # j >= 1: u == 0 and lerp(0, A_j, A_{j-1}) is A_j; j == 0: (A_0 + s_0) - s_0
        assert np.array_equal(back, np.full(len(s), a)) if j else np.abs(back - a).max() <= ULP
    above = anchors[0] + np.linspace(0.0, 9000.0, len(s))
    assert np.array_equal(TC.displace(above, anchors, s, TC.APPLY), above + s[:, 0])
    below = anchors[-1] - np.linspace(1.0, 9000.0, len(s))
    assert np.array_equal(TC.displace(below, anchors, s, TC.APPLY), below + s[:, -1])
    nan = TC.displace(np.array([np.nan]), anchors, s[:1], TC.APPLY)
    assert np.isnan(nan).all()


def _round_trip_inputs():
    """(anchors, rho [C * 3000], s [C * 3000, na]) for every column of a regional map with 5 anchors and a global one with 9:
    deformed layers at least 500 m thick."""
    out = []
    for (lat, lon, anchors, shifts), seed in ((TC.regional(5, seed=7), 1), (TC.global_map(9, seed=8), 2)):
        s = shifts.reshape(-1, len(anchors))
        ratio = -np.diff(anchors)[None, :] / -np.diff(anchors[None, :] + s, axis=1)
        assert ratio.max() <= WORST_RATIO and -np.diff(anchors[None, :] + s, axis=1).min() >= 500.0
        out.append((anchors,) + TC.column_radii(anchors, s, 3000, seed))
    return out


def test_apply_against_extended_precision():
    """The float64 statement against the same expressions in np.longdouble: within 1 ulp of the radius."""
    for anchors, rho, s in _round_trip_inputs():
        moved = TC.displace(rho, anchors, s, TC.APPLY)
        wide = TC.displace(rho, anchors, s, TC.APPLY, dtype=np.longdouble)
        assert float(np.abs(moved - wide).max()) <= ULP


def test_the_round_trip():
    """flatten(apply(rho)) on columns whose deformed layers are at least 500 m thick.  Measured on these inputs: at most
    2.794e-09 m (3 ulps of 6.4e6); allowed: four times that, 1.118e-08 m."""
    worst = 0.0
    for anchors, rho, s in _round_trip_inputs():
        back = TC.displace(TC.displace(rho, anchors, s, TC.APPLY), anchors, s, TC.FLATTEN)
        worst = max(worst, float(np.abs(back - rho).max()))
    print(f"round trip: {worst:.4g} m = {worst / ULP:.1f} ulp")
    assert worst <= ROUND_TRIP_BOUND


def test_the_round_trip_through_a_layer_of_one_metre():
    """The error is conditioned by (A_j - A_{j+1}) / (B_j - B_{j+1}): a 3000 m layer deformed to 1 m (ratio 3000 against 12)
    gives 1.397e-06 m here, 500 times the well-conditioned figure; the bound scales with the ratio."""
    anchors = TC.anchor_radii(3, 6000.0)
    rho, s = TC.column_radii(anchors, np.array([[0.0, 0.0, 2999.0]]), 200000, 3)
    assert (anchors[1] - anchors[2]) / ((anchors[1] + 0.0) - (anchors[2] + 2999.0)) == 3000.0
    back = TC.displace(TC.displace(rho, anchors, s, TC.APPLY), anchors, s, TC.FLATTEN)
    worst = float(np.abs(back - rho).max())
    print(f"round trip through 1 m: {worst:.4g} m = {worst / ULP:.1f} ulp")
    assert ROUND_TRIP_BOUND < worst <= ROUND_TRIP_BOUND * 3000.0 / WORST_RATIO


def test_copies_of_a_shared_node_get_the_same_bits():
    model = TC.regional(5, seed=9)
    pts = TC.elements(30, 27, model[2], seed=1, lat=(-5.0, 5.0), lon=(-5.0, 5.0))
    pts[1::2, :9] = pts[0::2, 18:]                                            # every second element shares a face with the one before
    for direction in (TC.APPLY, TC.FLATTEN):
        out, _, _ = _on_host(pts.reshape(-1, 3), model, direction=direction)
        out = out.reshape(pts.shape)
        assert np.array_equal(out[1::2, :9].view(np.uint64), out[0::2, 18:].view(np.uint64)) and not np.array_equal(out, pts)


# --------------------------------------------------------------------------------------- the cases of the guarded test
def test_the_guarded_cases_span_the_byte_classes_and_hold_every_edge():
    cases = TC.guarded_cases()
    assert G.classes(cases, "points") == G.classes(cases, "lat") == G.classes(cases, "shifts") == {"pages", "granule", "neither"}
    assert G.classes(cases, "lon") == {"granule", "neither"}       # (a page of longitudes beside a page of latitudes is a map of 2 MB)
    assert G.classes(cases, "ref") == {"pages", "granule", "neither"}
    assert G.classes(cases, "anchors") == {"granule", "neither"}   # at most 64 anchors: 512 bytes, never a page
    for case in cases:
        counts = TC.guarded_edge_counts(case)
        assert all(v > 0 for v in counts.values()), (case["name"], counts)
        assert ("seam" in counts) == case["periodic"]
        for direction in (TC.APPLY, TC.FLATTEN):
            for lateral in (TC.CELL, TC.BILINEAR):
                for outside in (TC.KEEP, TC.CLAMP):
                    out, rad, nout = _on_host(case["points"], (case["lat"], case["lon"], case["anchors"], case["shifts"]),
                                              case["periodic"], direction=direction, lateral=lateral, outside=outside,
                                              ref=case["ref"] if direction == TC.APPLY else None)
                    assert np.isfinite(out).all() and np.isfinite(rad).all()
                    assert nout == 0 if (outside == TC.CLAMP or case["periodic"]) else 0 < nout < len(rad)
