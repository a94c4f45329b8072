"""The NumPy statement of mm_sample_grid (include/multimesh_hip.h) and the inputs the grid-import tests share.  Nothing
here imports the code under test.

Per point p = (x, y, z), every operation an array operation of its own (no fused multiply-add):

  r = sqrt((x*x + y*y) + z*z)        depth = 6371000.0 - r        c = z / r where r > 0, else 0.0
  lat = 90.0 - arccos(c) * (180.0 / pi)        lon = arctan2(y, x) * (180.0 / pi)             (np.rad2deg's product)
  periodic: lon += 360.0 where lon < lon_a[0], then lon -= 360.0 where lon >= lon_a[0] + 360.0

Per axis a[0..n-1] and value v: inside = (v >= a[0]) & (v <= a[n-1]); clamp mode sets v = minimum(maximum(v, a[0]), a[n-1])
and inside = True; i = clip(searchsorted(a, v, side="right") - 1, 0, n - 2), t = (v - a[i]) / (a[i+1] - a[i]), i1 = i + 1.  An
axis of length 1: i = i1 = 0, t = 0, inside.

Per component, lerp(t, p, q) = (1.0 - t) * p + t * q: four along longitude, two along latitude, one along depth.
"""
import numpy as np

R_EARTH = 6371000.0
RAD2DEG = 180.0 / np.pi
MODES = ("fill", "clamp", "keep")

AXIS_POINTS = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0],
                        [0.0, -1.0, 0.0], [0.0, 0.0, 0.0]])
# (lat, lon) of the six axis directions and of the origin, exact in the statement above
AXIS_LATLON = np.array([[90.0, 0.0], [-90.0, 0.0], [0.0, 0.0], [0.0, 180.0], [0.0, 90.0], [0.0, -90.0], [0.0, 0.0]])


def latlondepth(points):
    """f64[..., 3] -> f64[N, 3] = (lat, lon, depth)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = np.sqrt((x * x + y * y) + z * z)
    depth = R_EARTH - r
    c = np.zeros_like(r)
    pos = r > 0
    c[pos] = z[pos] / r[pos]
    lat = 90.0 - np.arccos(c) * RAD2DEG
    lon = np.arctan2(y, x) * RAD2DEG
    return np.stack([lat, lon, depth], axis=1)


def wrap(lon, lon0):
    lon = np.where(lon < lon0, lon + 360.0, lon)
    return np.where(lon >= lon0 + 360.0, lon - 360.0, lon)


def cell(axis, v, clamp):
    """-> (i, i1, t, inside)"""
    a = np.asarray(axis, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    n = len(a)
    if n == 1:
        z = np.zeros(v.shape, dtype=np.int64)
        return z, z, np.zeros(v.shape), np.ones(v.shape, dtype=bool)
    inside = (v >= a[0]) & (v <= a[-1])
    if clamp:
        v = np.minimum(np.maximum(v, a[0]), a[-1])
        inside = np.ones(v.shape, dtype=bool)
    i = np.clip(np.searchsorted(a, v, side="right") - 1, 0, n - 2)
    with np.errstate(invalid="ignore"):
        t = (v - a[i]) / (a[i + 1] - a[i])
    return i, i + 1, t, inside


def lerp(t, p, q):
    return (1.0 - t) * p + t * q


def sample(grid, depth, lat, lon, D, LA, LO, mode="fill", fill=np.nan, periodic=False, out=None):
    """grid f64[C, nd, nla, nlo] at the points' (D, LA, LO) -> (values f64[C, N], nmissing, inside bool[N]).
    ``out`` f64[C, N]: what "keep" starts from (not modified)."""
    grid = np.asarray(grid, dtype=np.float64)
    D, LA, LO = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (D, LA, LO))
    if periodic:
        LO = wrap(LO, lon[0])
    clamp = mode == "clamp"
    k, k1, tz, in_d = cell(depth, D, clamp)
    j, j1, ty, in_la = cell(lat, LA, clamp)
    i, i1, tx, in_lo = cell(lon, LO, clamp)
    inside = in_d & in_la & in_lo
    C, N = grid.shape[0], len(D)
    if mode == "keep":
        res = np.array(out, dtype=np.float64).reshape(C, N)
    else:
        res = np.full((C, N), fill, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for c in range(C):
            g = grid[c]
            a00 = lerp(tx, g[k, j, i], g[k, j, i1])
            a01 = lerp(tx, g[k, j1, i], g[k, j1, i1])
            a10 = lerp(tx, g[k1, j, i], g[k1, j, i1])
            a11 = lerp(tx, g[k1, j1, i], g[k1, j1, i1])
            v = lerp(tz, lerp(ty, a00, a01), lerp(ty, a10, a11))
            res[c, inside] = v[inside]
    return res, int((~inside).sum()), inside


def same_bits(a, b):
    """Equal shapes, NaN in the same places, and every other value equal bit for bit (IEEE-754 leaves the sign and the
    payload of a NaN that an operation produces to the implementation; its place it does not)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


# ------------------------------------------------------------------------------------------------ shared inputs
DEPTH = np.array([-5_000.0, 0.0, 12_000.0, 40_000.0, 95_000.0, 180_000.0, 300_000.0])      # non-uniform
LAT = np.linspace(-6.0, 6.0, 9)
LON = np.linspace(-5.5, 6.5, 11)


def grid_values(ncomp, shape=(7, 9, 11), seed=5):
    """A smooth part plus noise, of order 1"""
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(*(np.linspace(0.0, 1.0, n) for n in shape), indexing="ij")
    base = np.sin(3.0 * k) + np.cos(2.0 * j) * (1.0 + i)
    return np.ascontiguousarray(np.stack([base * (c + 1.0) + rng.normal(size=shape) for c in range(ncomp)])
                                if ncomp else np.zeros((0,) + shape))


def chunk_points(n, seed=11, order=4, **deform):
    """n nodes of the +-8 degree, 400 km chunk of synth.earth_chunk in a seeded random order: some inside the grid above,
    some outside it on every axis."""
    from multimesh_amd import synth

    pts = synth.earth_chunk(order, nlat=4, nlon=4, **deform)["points"].reshape(-1, 3)
    pick = np.random.default_rng(seed).permutation(len(pts))[:n]
    return np.ascontiguousarray(pts[pick])


def sphere_points(n=4099, seed=3, rmin=3.5e6, rmax=6.4e6):
    """n random directions over the whole sphere at radii rmin..rmax"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return np.ascontiguousarray(v * rng.uniform(rmin, rmax, size=(n, 1)))


def periodic_field(lat, lon, depth):
    """A function of (lat, lon mod 360, depth) on the nodes: f64[D, LA, LO]"""
    lo = np.deg2rad(np.mod(lon, 360.0))[None, None, :]
    la = np.deg2rad(lat)[None, :, None]
    d = (np.asarray(depth) / 1.0e6)[:, None, None]
    return np.cos(la) * np.sin(2.0 * lo) + 0.3 * np.sin(la) + 0.1 * np.cos(lo) + 0.2 * d
