"""Geographic coordinates without a GPU: the extension header against the module's signature table, the NumPy statement of
tests/geodesy_cases.py against its 12-pass ``long double`` form and against the textbook formulas, its rules for the polar
axis and the centre, :class:`Ellipsoid` on the host, and the argument errors that are decided before the device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import geodesy_cases as GC
from multimesh_amd import geodesy as G
from multimesh_amd import helpers
from multimesh_amd.api import GllMesh
from multimesh_amd.mesh import HexMesh
from test_parametrisation import _c_class, _ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multimesh_geodesy.h")
SYMBOLS = ["mm_geographic_points"]
EPS = GC.EPS
WGS84 = GC.constants()


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
    assert list(protos) == list(G.SIGNATURES) == SYMBOLS
    lib = G.bind()
    assert lib is helpers.load_lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = G.SIGNATURES[name]
        assert (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes]) == (ret, params), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert name not in helpers.SIGNATURES and name not in helpers.EXPORTED_SYMBOLS
    text = open(HEADER).read()
    assert int(re.search(r"#define MM_GEODESY_TO_GEOGRAPHIC (\d+)", text).group(1)) == G.TO_GEOGRAPHIC == GC.TO_GEOGRAPHIC == 0
    assert int(re.search(r"#define MM_GEODESY_TO_CARTESIAN (\d+)", text).group(1)) == G.TO_CARTESIAN == GC.TO_CARTESIAN == 1
    assert int(re.search(r"#define MM_GEODESY_NCONST (\d+)", text).group(1)) == G.NCONST == len(WGS84)
    assert re.search(r"THREE times", text) and GC.PASSES == 3


def test_the_library_exports_the_symbol():
    lib = helpers.load_lib()
    assert all(hasattr(lib, s) for s in SYMBOLS)


# ------------------------------------------------------------------------------------------------------- the statement
def test_three_passes_agree_with_twelve_in_long_double():
    """Seeded points with |p| in [200 km, 6500 km]: the latitude within 1e-13 rad of the 12-pass long double form (measured:
    4.3e-14 down to 200 km, 1.7e-16 from 1000 km up), the round trip within 1e-7 m (measured: 8.5e-9)."""
    pts = GC.cloud(200_000, seed=11)
    assert 200_000.0 <= np.linalg.norm(pts, axis=1).min() and np.linalg.norm(pts, axis=1).max() <= 6_500_000.0
    cphi, sphi, h, _ = GC.latitude_and_height(WGS84, pts[:, 0], pts[:, 1], pts[:, 2])
    want_lat, want_h = GC.long_double_latitude(pts)
    lat_error = np.abs(np.arctan2(sphi.astype(np.longdouble), cphi.astype(np.longdouble)) - want_lat).max()
    print(f"latitude error {float(lat_error):.3g} rad, height error {float(np.abs(h - want_h).max()):.3g} m")
    assert lat_error <= 1e-13
    shallow = np.linalg.norm(pts, axis=1) >= 1_000_000.0
    assert np.abs(np.arctan2(sphi, cphi) - want_lat)[shallow].max() <= 4 * EPS          # ... and nothing left from 1000 km up
    pseudo, _ = GC.to_geographic(WGS84, pts)
    trip = np.abs(GC.from_geographic(WGS84, pseudo) - pts).max()
    print(f"round trip {trip:.3g} m")
    assert trip <= 1e-7
    # two passes are not enough: what the third is for
    cphi2, sphi2, _, _ = GC.latitude_and_height(WGS84, pts[:, 0], pts[:, 1], pts[:, 2], passes=2)
    assert np.abs(np.arctan2(sphi2, cphi2) - want_lat).max() > 1e-12


def _known_geodetic():
    rng = np.random.default_rng(5)
    lat = np.concatenate([[90.0, -90.0, 90.0, -90.0, 0.0, 0.0, 0.0, 0.0, 45.0, -45.0, 89.999999, -89.999999, 1e-9],
                          rng.uniform(-90.0, 90.0, 2000)])
    lon = np.concatenate([[0.0, 0.0, 77.0, -180.0, 0.0, 180.0, -180.0, 90.0, 180.0, -180.0, 10.0, -20.0, 30.0],
                          rng.uniform(-180.0, 180.0, 2000)])
    h = np.concatenate([[0.0, 0.0, 8848.0, -11000.0, 0.0, 0.0, -2_891_000.0, 400_000.0, 0.0, -660_000.0, 0.0, 100.0, -5_000_000.0],
                        rng.uniform(-5_000_000.0, 500_000.0, 2000)])
    return lat, lon, h


def test_known_geodetic_coordinates_come_back():
    """Points built from (lat, lon, h) by the textbook formulas: the statement returns lat within 1e-12 degrees and h within
    1e-8 m -- at the poles, on the equator and at +-180 degrees too --, and direction 1 rebuilds the points."""
    lat, lon, h = _known_geodetic()
    pts = GC.textbook_points(lat, lon, h)
    pseudo, got_h = GC.to_geographic(WGS84, pts)
    got_lat = np.rad2deg(np.arctan2(pseudo[:, 2], np.hypot(pseudo[:, 0], pseudo[:, 1])))
    got_lon = np.rad2deg(np.arctan2(pseudo[:, 1], pseudo[:, 0]))
    print(f"lat {np.abs(got_lat - lat).max():.3g} deg, h {np.abs(got_h - h).max():.3g} m")
    assert np.abs(got_lat - lat).max() <= 1e-12
    assert np.abs(got_h - h).max() <= 1e-8
    off_axis = np.abs(lat) != 90.0
    dlon = np.abs(got_lon - lon)[off_axis]
    assert np.minimum(dlon, 360.0 - dlon).max() <= 1e-12                      # (+180 and -180 are one meridian)
    assert (got_lon[~off_axis] == 0.0).all() and (np.abs(got_lat[~off_axis]) == 90.0).all()
    assert np.abs(np.linalg.norm(pseudo, axis=1) - (GC.R_EARTH + h)).max() <= 1e-8     # the depth every sampler will read
    assert np.abs(GC.from_geographic(WGS84, pseudo) - pts).max() <= 1e-7
    # a given radius replaces R + h and nothing else
    rho = GC.radii(len(pts), seed=1)
    with_radius, same_h = GC.to_geographic(WGS84, pts, radius=rho)
    assert np.array_equal(same_h, got_h)
    assert np.abs(np.linalg.norm(with_radius, axis=1) - rho).max() <= 4 * EPS * GC.R_EARTH
    assert np.abs(with_radius / rho[:, None] - pseudo / np.linalg.norm(pseudo, axis=1, keepdims=True)).max() <= 8 * EPS


def test_the_axis_takes_longitude_zero_and_the_centre_gives_nan():
    rows = GC.special_rows()
    for direction in (GC.TO_GEOGRAPHIC, GC.TO_CARTESIAN):
        out = GC.apply(WGS84, rows, direction)
        poles = out[:4]                                                       # s = 0, with either sign of the zeros
        assert (poles[:, 0] == 0.0).all() and (poles[:, 1] == 0.0).all() and np.isfinite(poles[:, 2]).all()
        assert np.array_equal(np.sign(poles[:, 2]), [1.0, -1.0, 1.0, -1.0])
        assert np.isnan(out[4:6]).all()                                       # the centre: 0 / 0
        assert np.isnan(out[6:9]).any(axis=1).all()                           # a NaN coordinate reaches the output
        assert np.isfinite(out[13:]).all()
    pseudo, h = GC.to_geographic(WGS84, rows)
    b = WGS84[1]
    assert np.abs(h[:4] - (GC.R_EARTH - b)).max() <= 1e-8 and np.abs(np.abs(pseudo[:4, 2]) - (GC.R_EARTH + h[:4])).max() <= 1e-8
    assert np.abs(h[13:18] - (GC.R_EARTH - WGS84[0])).max() <= 1e-8           # on the equator the height is r - a
    assert np.isnan(h[4]) and np.isnan(h[6])


# ----------------------------------------------------------------------------------------------------------- Ellipsoid
def test_ellipsoid_refuses_what_it_should():
    for a, f in ((np.nan, 0.1), (np.inf, 0.1), (1.0, np.nan), (1.0, np.inf)):
        with pytest.raises(ValueError, match="finite"):
            G.Ellipsoid(a, f)
    for a in (0.0, -6378137.0):
        with pytest.raises(ValueError, match="positive"):
            G.Ellipsoid(a, 0.0)
    for f in (-1e-9, 0.5, 0.75, 1.0):
        with pytest.raises(ValueError, match="flattening"):
            G.Ellipsoid(6378137.0, f)
    with pytest.raises(ValueError, match="flattening"):
        G.Ellipsoid.from_mean_radius(f=0.5)
    with pytest.raises(ValueError, match="sphere_radius"):
        G.Ellipsoid.wgs84().constants(sphere_radius=0.0)
    G.Ellipsoid(1.0, 0.0), G.Ellipsoid(1.0, 0.499)


def test_ellipsoid_constants():
    wgs = G.Ellipsoid.wgs84()
    assert (wgs.a, wgs.f) == (6378137.0, 1.0 / 298.257223563)
    got = wgs.constants()
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), WGS84.view(np.uint64))
    a, b, e2, ome2, omf, ep2b, e2a, R = got
    assert abs(b - 6356752.314245179) < 1e-8 and abs(e2 - 6.69437999014e-3) < 1e-14 and R == 6371000.0
    assert abs(ome2 - omf * omf) <= 2 * EPS and abs(ep2b - (a * a - b * b) / b) == 0.0 and e2a == e2 * a
    assert wgs.constants(sphere_radius=6371008.8)[7] == 6371008.8
    mean = G.Ellipsoid.from_mean_radius()
    assert mean.f == wgs.f and abs(mean.a * mean.a * mean.b - 6371000.0 ** 3) <= 8 * EPS * 6371000.0 ** 3      # equal volume
    assert abs(mean.a - 6371000.0 * (1.0 + wgs.f / 3.0)) < 6371000.0 * wgs.f ** 2                               # first order in f


def test_a_sphere_of_the_packages_radius_is_the_identity():
    """f = 0, a = R: e2, ep2b and e2a are exactly 0 and both directions return the point within 4 ulp of |p|
    (``np.spacing(|p|)``).  The points have the radii of an Earth mesh, from below the core-mantle boundary to above the
    surface: the statement forms ``h = r - R`` and then ``R + h``, so its rounding is of the size of an ulp of R whatever
    |p| is, and "ulp of |p|" is a measure only where |p| is of the order of R (at 200 km an ulp of |p| is 32 times smaller
    than one of R; the figure for such points is printed, not asserted)."""
    ell = G.Ellipsoid(GC.R_EARTH, 0.0).constants()
    assert np.array_equal(ell, [GC.R_EARTH, GC.R_EARTH, 0.0, 1.0, 1.0, 0.0, 0.0, GC.R_EARTH])
    pts = GC.cloud(20_000, seed=3, rmin=3_400_000.0)
    norm = np.linalg.norm(pts, axis=1, keepdims=True)
    ulp = np.spacing(norm)
    there, h = GC.to_geographic(ell, pts)
    back = GC.from_geographic(ell, pts)
    deep = GC.cloud(20_000, seed=4, rmax=3_400_000.0)
    print(f"identity: {(np.abs(there - pts) / ulp).max():.1f} ulp of |p| there, {(np.abs(back - pts) / ulp).max():.1f} back; "
          f"at 200 km to 3400 km: {(np.abs(GC.to_geographic(ell, deep)[0] - deep) / np.spacing(np.linalg.norm(deep, axis=1, keepdims=True))).max():.1f}")
    assert (np.abs(there - pts) <= 4 * ulp).all()
    assert (np.abs(back - pts) <= 4 * ulp).all()
    assert (np.abs(h - (norm[:, 0] - GC.R_EARTH)) <= 4 * ulp[:, 0]).all()


# --------------------------------------------------------------------------------------------------- argument checks
CTX = C.c_void_p(0x1000)            # a dummy: a refused call never looks at the context
A, B, RAD, HGT = 0x100000, 0x900000, 0x2000000, 0x3000000          # never read
N = 10


def _ell(**changed):
    e = list(WGS84)
    for k, v in changed.items():
        e[int(k[1:])] = v
    return (C.c_double * 8)(*e)


def _call(lib, ctx=CTX, n=N, a=A, b=B, ell=_ell(), direction=0, radius=None, height=None):
    return lib.mm_geographic_points(ctx, n, a, b, ell, direction, radius, height)


REFUSED = {
    "null ctx": dict(ctx=None),
    "negative n": dict(n=-1),
    "3 n at 2^48": dict(n=-(-(1 << 48) // 3)),
    "null in": dict(a=None),
    "null out": dict(b=None),
    "null ell": dict(ell=None),
    "NaN in ell": dict(ell=_ell(e2=np.nan)),
    "inf in ell": dict(ell=_ell(e7=np.inf)),
    "-inf in ell": dict(ell=_ell(e5=-np.inf)),
    "a zero": dict(ell=_ell(e0=0.0)),
    "a negative": dict(ell=_ell(e0=-6378137.0)),
    "b zero": dict(ell=_ell(e1=0.0)),
    "b negative": dict(ell=_ell(e1=-1.0)),
    "direction 2": dict(direction=2),
    "direction -1": dict(direction=-1),
    "radius with direction 1": dict(direction=1, radius=RAD),
    "height with direction 1": dict(direction=1, height=HGT),
    "out starts inside in": dict(b=A + 8),
    "out one point into in": dict(b=A + 24),
    "out ends inside in": dict(b=A - 24 * (N - 1)),
    "radius inside out": dict(radius=B + 8),
    "radius over the end of out": dict(radius=B + 24 * N - 8),
    "radius ends inside out": dict(radius=B - 8 * (N - 1)),
    "height inside out": dict(height=B + 16),
    "height ends inside out": dict(height=B - 8 * (N - 1)),
    "height inside in": dict(height=A + 8),
    "height inside radius": dict(radius=RAD, height=RAD + 8),
    "height inside out, in place": dict(b=A, height=A + 24),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_geographic_points_refuses_without_a_gpu(what):
    lib = G.bind()
    assert _call(lib, **REFUSED[what]) == -1, what
    message = lib.mm_last_error()
    assert b"mm_geographic_points" in message and len(message) > len(b"mm_geographic_points: "), message
    assert lib.mm_last_status() == -1


def test_nothing_to_do_is_valid_without_a_gpu():
    """n == 0: MM_OK before the device is touched, null arrays allowed -- but what is wrong whatever n is, is still refused."""
    lib = G.bind()
    assert _call(lib, n=0, a=None, b=None) == 0
    assert _call(lib, n=0, a=None, b=None, direction=1) == 0
    assert _call(lib, n=0, a=None, b=None, direction=2) == -1
    assert _call(lib, n=0, a=None, b=None, ell=None) == -1


def test_python_refuses_before_the_library_is_asked():
    wgs = G.Ellipsoid.wgs84()
    with pytest.raises(ValueError, match="GllMesh or a HexMesh"):
        G.as_geographic(np.zeros((4, 3)), wgs)
    with pytest.raises(ValueError, match="3-D meshes only"):
        G.as_geographic(GllMesh(np.zeros((2, 9, 2)), 2, {}), wgs)
    with pytest.raises(ValueError, match="3-D meshes only"):
        G.as_geographic(HexMesh(np.zeros((4, 2)), np.zeros((1, 4), dtype=np.int64)), wgs)
    with pytest.raises(ValueError, match="depth must be"):
        G.as_geographic(GllMesh(np.zeros((2, 27, 3)), 2, {}), wgs, depth="geoid")
    with pytest.raises(ValueError, match="z_node_1D"):
        G.as_geographic(GllMesh(np.ones((2, 27, 3)), 2, {"VS": np.ones((2, 27))}), wgs, depth="z_node_1D")
    with pytest.raises(ValueError, match="its 8 constants"):
        G._constants(np.zeros(7))
    with pytest.raises(ValueError, match="takes a GllMesh"):
        G.extract_geographic_grid(np.zeros((4, 3)), ["VS"], [0.0], [0.0], [0.0])
    with pytest.raises(ValueError, match="no field"):
        G.extract_geographic_grid(GllMesh(np.ones((2, 27, 3)), 2, {}), ["VS"], [0.0], [0.0], [0.0])
    with pytest.raises(ValueError, match="latitude axis"):
        G.extract_geographic_grid(GllMesh(np.ones((2, 27, 3)), 2, {"VS": np.ones((2, 27))}), ["VS"], [np.nan], [0.0], [0.0])
