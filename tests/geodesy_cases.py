"""The NumPy statement of include/multimesh_geodesy.h (``mm_geographic_points``), operation by operation -- every product,
quotient, sum and square root a separate IEEE binary64 operation, sums left to right --, its 12-pass ``long double`` form, the
textbook formulas, and the case builders of tests/test_geodesy.py, tests/test_geodesy_gpu.py and
tests/test_geodesy_guarded_gpu.py."""
import numpy as np

R_EARTH = 6371000.0
EPS = np.finfo(np.float64).eps
TO_GEOGRAPHIC, TO_CARTESIAN = 0, 1      # MM_GEODESY_TO_*
PASSES = 3
WGS84_A, WGS84_F = 6378137.0, 1.0 / 298.257223563


def constants(a=WGS84_A, f=WGS84_F, R=R_EARTH, dtype=np.float64):
    """(a, b, e2, 1 - e2, 1 - f, ep2b, e2a, R) formed as multimesh_amd.geodesy.Ellipsoid.constants forms them, in ``dtype``."""
    a, f, R = dtype(a), dtype(f), dtype(R)
    one, two = dtype(1.0), dtype(2.0)
    b = a * (one - f)
    e2 = f * (two - f)
    return np.array([a, b, e2, one - e2, one - f, (a * a - b * b) / b, e2 * a, R], dtype=dtype)


# ------------------------------------------------------------------------------------------------------- the statement
def _longitude(x, y, s):
    off_axis = s > 0.0
    safe = np.where(off_axis, s, 1.0)
    return np.where(off_axis, x / safe, 1.0), np.where(off_axis, y / safe, 0.0)


def latitude_and_height(ell, x, y, z, passes=PASSES):
    """(cphi, sphi, h, s) of the header's DIRECTION 0 for arrays x, y, z, in the dtype of the arrays."""
    a, b, e2, _, omf, ep2b, e2a, _ = ell
    with np.errstate(all="ignore"):
        s = np.sqrt(x * x + y * y)
        u, v = b * s, a * z
        for _ in range(passes):
            nb = np.sqrt(u * u + v * v)
            cb, sb = u / nb, v / nb
            zn = z + ep2b * ((sb * sb) * sb)
            sn = s - e2a * ((cb * cb) * cb)
            u, v = sn, omf * zn
        nn = np.sqrt(sn * sn + zn * zn)
        cphi, sphi = sn / nn, zn / nn
        h = (s * cphi + z * sphi) - a * np.sqrt(1.0 - e2 * (sphi * sphi))
    return cphi, sphi, h, s


def to_geographic(ell, points, radius=None, passes=PASSES):
    """mm_geographic_points, direction 0: (pseudo-points f64[..., 3], heights f64[...])."""
    ell = np.asarray(ell, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    cphi, sphi, h, s = latitude_and_height(ell, x, y, z, passes)
    with np.errstate(all="ignore"):
        cl, sl = _longitude(x, y, s)
        rho = ell[7] + h if radius is None else np.asarray(radius, dtype=np.float64)
        return np.stack([(rho * cphi) * cl, (rho * cphi) * sl, rho * sphi], axis=-1), h


def from_geographic(ell, points):
    """mm_geographic_points, direction 1: f64[..., 3] -> f64[..., 3]."""
    a, _, e2, ome2, _, _, _, R = np.asarray(ell, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) + z * z)
        s = np.sqrt(x * x + y * y)
        cl, sl = _longitude(x, y, s)
        sphi, cphi, h = z / r, s / r, r - R
        N = a / np.sqrt(1.0 - e2 * (sphi * sphi))
        return np.stack([((N + h) * cphi) * cl, ((N + h) * cphi) * sl, (N * ome2 + h) * sphi], axis=-1)


def apply(ell, points, direction, radius=None):
    return to_geographic(ell, points, radius)[0] if direction == TO_GEOGRAPHIC else from_geographic(ell, points)


# ------------------------------------------------------------------------------------------ what the statement is held to
def long_double_latitude(points, a=WGS84_A, f=WGS84_F, passes=12):
    """(geodetic latitude in radians, height) of the same iteration run ``passes`` times in ``long double``."""
    ld = np.longdouble
    p = np.asarray(points, dtype=np.float64).astype(ld)
    cphi, sphi, h, _ = latitude_and_height(constants(a, f, dtype=ld), p[..., 0], p[..., 1], p[..., 2], passes)
    return np.arctan2(sphi, cphi), h


def textbook_points(lat_deg, lon_deg, h, a=WGS84_A, f=WGS84_F):
    """Cartesian f64[..., 3] of geodetic (lat, lon, h) by the textbook formulas, ``(N + h) cos(lat) cos(lon)`` ..., evaluated in
    ``long double`` and rounded once."""
    ld = np.longdouble
    lat, lon, h = np.deg2rad(np.asarray(lat_deg, dtype=ld)), np.deg2rad(np.asarray(lon_deg, dtype=ld)), np.asarray(h, dtype=ld)
    a, f = ld(a), ld(f)
    e2 = f * (2 - f)
    N = a / np.sqrt(1 - e2 * np.sin(lat) ** 2)
    # the cosine of +-90 degrees is exactly 0: a pole lies on the axis
    clat = np.where(np.abs(np.asarray(lat_deg, dtype=ld)) == 90, ld(0), np.cos(lat))
    out = np.stack([(N + h) * clat * np.cos(lon), (N + h) * clat * np.sin(lon), (N * (1 - e2) + h) * np.sin(lat)], axis=-1)
    return out.astype(np.float64)


def same_bits_nan(a, b):
    """Equal bit for bit where neither is a NaN, and NaN in the same places (a NaN's payload and sign are the processor's)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


# ------------------------------------------------------------------------------------------------------------ the cases
def cloud(n, seed=0, rmin=200_000.0, rmax=6_500_000.0):
    """n points in random directions with |p| uniform in [rmin, rmax], f64[n, 3]."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    return d * rng.uniform(rmin, rmax, (n, 1))


def special_rows():
    """Rows with +-0.0, +-inf and NaN coordinates, both poles (s = 0, with either sign of zero), the centre, the axes of the
    equator and a point a denormal away from the axis."""
    r = R_EARTH
    return np.array([[0.0, 0.0, r], [0.0, 0.0, -r], [-0.0, 0.0, r], [-0.0, -0.0, -r], [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0],
                     [np.nan, 1.0, r], [1.0, np.nan, 2.0], [1.0, 2.0, np.nan], [np.inf, 1.0, 1.0], [1.0, -np.inf, 1.0],
                     [1.0, 1.0, np.inf], [-np.inf, np.inf, -np.inf], [r, 0.0, 0.0], [-r, 0.0, -0.0], [0.0, r, 0.0],
                     [0.0, -r, 0.0], [-r, -0.0, 0.0], [5e-324, 0.0, r], [1e-200, -1e-200, -r]])


def points_with_specials(n, seed=0):
    """:func:`cloud` with :func:`special_rows` at its head (as many as fit)."""
    pts = cloud(n, seed=seed)
    special = special_rows()
    k = min(n, len(special))
    pts[:k] = special[:k]
    return pts


def radii(n, seed=0):
    """One radius per point, as ``z_node_1D * 6371000`` would give them."""
    return np.random.default_rng(300 + seed).uniform(0.5, 1.0, n) * R_EARTH


GUARDED_SIZES = (1, 2, 101, 512)


def guarded_cases():
    """The inputs of tests/test_geodesy_guarded_gpu.py: ordinary points (a few special rows at the head of the larger ones) at
    sizes whose 3 n doubles end on no allocation granule (1, 101) and on one (2, 512), with a radius per point."""
    return [{"name": f"n={n}", "points": points_with_specials(n, seed=40 + n) if n > 100 else cloud(n, seed=40 + n),
             "radius": radii(n, seed=n)} for n in GUARDED_SIZES]
