"""The NumPy statement of mm_layered_model_apply (include/multimesh_layered.h), written from the header and not from the
kernel, and the small models and point sets the layered-model tests share.  Nothing here imports the code under test.

The device's acos and atan2 are the only part that cannot be bit for bit, so the statement starts from the (lat, lon, depth)
the device handed back (``lld``); everything after them is one NumPy float64 operation per operation of the header.

  element_depth  6371000 - |centre| of every element: the picking depth of pick = 1 (no libm: bit for bit)
  columns        b_j (or the values of a layer) at the nodes' columns: bilinear, or the nearest map node's
  model_apply    the whole statement: (out, layer, span, noutside)
"""
import numpy as np

from grid_import_cases import cell, latlondepth, lerp, wrap  # noqa: F401  (latlondepth, wrap: re-exported for the tests)
from radial_cases import same_bits_nan  # noqa: F401  (re-exported for the tests)

R_EARTH = 6371000.0
FILL, CLAMP, KEEP = 0, 1, 2
CELL, BILINEAR = 0, 1
NODE, ELEMENT = 0, 1


def element_depth(points):
    """points f64[G, P, 3] -> dp f64[G * P]: 6371000 - rc of the node's element, c = (((X[0] + X[1]) + ...) + X[P-1]) / P."""
    X = np.asarray(points, dtype=np.float64)
    G, P = X.shape[:2]
    c = X[:, 0, :].copy()
    with np.errstate(all="ignore"):
        for p in range(1, P):
            c = c + X[:, p, :]
        c = c / np.float64(P)
        rc = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        return np.repeat(R_EARTH - rc, P)


def columns(table, ca, co, lateral):
    """table f64[nlat, nlon, ...] at the nodes' columns -> f64[N, ...].  ca, co: (i, i1, t, inside) per axis."""
    ja, ja1, ta, _ = ca
    io, io1, to, _ = co
    if lateral == CELL:
        with np.errstate(invalid="ignore"):
            return table[np.where(ta < 0.5, ja, ja1), np.where(to < 0.5, io, io1)]
    shape = (-1,) + (1,) * (table.ndim - 2)
    ta, to = ta.reshape(shape), to.reshape(shape)
    with np.errstate(all="ignore"):
        return lerp(ta, lerp(to, table[ja, io], table[ja, io1]), lerp(to, table[ja1, io], table[ja1, io1]))


def model_apply(lld, dp, lat, lon, bounds, values, lateral=BILINEAR, pick=NODE, outside=FILL, fill=np.nan, out_before=None):
    """lld f64[N, 3] = the device's (lat, lon, depth); dp f64[N]: the picking depth of pick = 1 (:func:`element_depth`;
    ignored with pick = 0); bounds f64[nlat, nlon, nb], values f64[nlat, nlon, nlayer, ncomp] (or None: no components);
    out_before f64[ncomp, N]: what outside = 2 starts from (not modified).
    -> (out f64[ncomp, N], layer int32[N], span f64[N, 2], noutside)."""
    lld = np.asarray(lld, dtype=np.float64).reshape(-1, 3)
    LA, LO = lld[:, 0], lld[:, 1]
    dp = lld[:, 2] if pick == NODE else np.asarray(dp, dtype=np.float64).reshape(-1)
    bounds = np.asarray(bounds, dtype=np.float64)
    nb = bounds.shape[2]
    nlayer, N = nb - 1, len(LA)
    values = np.zeros(bounds.shape[:2] + (nlayer, 0)) if values is None else np.asarray(values, dtype=np.float64)
    ncomp = values.shape[3]
    clamp = outside == CLAMP
    with np.errstate(invalid="ignore"):
        ca, co = cell(lat, LA, clamp), cell(lon, LO, clamp)
        valid = ~np.isnan(LA) & ~np.isnan(LO) & ~np.isnan(dp) & ca[3] & co[3]
        b = columns(bounds, ca, co, lateral)                      # [N, nb]
        below = dp[:, None] < b[:, 1:]                            # dp < b_{j+1}
        from_top = dp >= b[:, 0]
        thick = b[:, :-1] < b[:, 1:]                              # layers of positive thickness
        first_thick = np.argmax(thick, axis=1)
        last_thick = nlayer - 1 - np.argmax(thick[:, ::-1], axis=1)
        layer = np.full(N, -1, dtype=np.int64)
        found = from_top & below.any(axis=1)
        layer[found] = np.argmax(below, axis=1)[found]
        rest = from_top & ~found & thick.any(axis=1)
        take_last = rest if clamp else rest & (dp == b[:, -1])
        layer[take_last] = last_thick[take_last]
        if clamp:
            take_first = (dp < b[:, 0]) & thick.any(axis=1)
            layer[take_first] = first_thick[take_first]
    layer[~valid] = -1
    inside = layer >= 0
    at = np.where(inside, layer, 0)
    rows = np.arange(N)
    span = np.full((N, 2), np.nan)
    span[inside, 0] = b[rows, at][inside]
    span[inside, 1] = b[rows, at + 1][inside]
    if outside == KEEP:
        out = np.array(out_before, dtype=np.float64).reshape(ncomp, N)
    else:
        out = np.full((ncomp, N), fill, dtype=np.float64)
    if ncomp:
        ja, ja1, ta, _ = ca
        io, io1, to, _ = co
        if lateral == CELL:
            with np.errstate(invalid="ignore"):
                v = values[np.where(ta < 0.5, ja, ja1), np.where(to < 0.5, io, io1), at]
        else:
            with np.errstate(all="ignore"):
                ta, to = ta[:, None], to[:, None]
                v = lerp(ta, lerp(to, values[ja, io, at], values[ja, io1, at]), lerp(to, values[ja1, io, at], values[ja1, io1, at]))
        out[:, inside] = v.T[:, inside]
    return out, layer.astype(np.int32), span, int((~inside).sum())


# ------------------------------------------------------------------------------------------------------- shared inputs
REGIONAL_LAT = np.array([-6.0, -4.5, -2.0, 0.0, 1.5, 4.0, 6.0])                       # 7, non-uniform
REGIONAL_LON = np.array([-5.5, -4.0, -3.0, -1.0, 0.0, 1.5, 3.0, 5.0, 6.5])           # 9
GLOBAL_LAT = np.linspace(-90.0, 90.0, 6)
GLOBAL_LON = np.arange(-180.0, 180.0, 30.0)                                           # 12: the closing column is appended


def layered_tables(lat, lon, nb, ncomp, seed=0, periodic=False):
    """(lat, lon, bounds f64[nlat, nlon, nb], values f64[nlat, nlon, nb - 1, ncomp]) as the device reads them: a top that
    undulates about 0 m (so some depths are negative), layers some 8 km thick; with nb = 5, layer 1 pinched to zero
    thickness over the southern part of the map; one column whose layers are all empty.  ``periodic``: ``lon`` goes once
    round without its closing column, which is appended here (lon[0] + 360, the tables of column 0)."""
    rng = np.random.default_rng(seed)
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    nlat, nlon, nlayer = len(lat), len(lon), nb - 1
    top = rng.uniform(-3000.0, 2000.0, (nlat, nlon))
    thickness = rng.uniform(4000.0, 12000.0, (nlat, nlon, nlayer))
    if nlayer >= 2:
        thickness[: max(nlat // 2, 1), :, 1] = 0.0
    thickness[nlat // 2, nlon // 3, :] = 0.0
    bounds = np.concatenate([top[..., None], top[..., None] + np.cumsum(thickness, axis=2)], axis=2)
    values = rng.uniform(2000.0, 8000.0, (nlat, nlon, nlayer, ncomp))
    if periodic:
        lon = np.concatenate([lon, [lon[0] + 360.0]])
        bounds = np.concatenate([bounds, bounds[:, :1]], axis=1)
        values = np.concatenate([values, values[:, :1]], axis=1)
    return lat, lon, np.ascontiguousarray(bounds), np.ascontiguousarray(values)


def regional(nb=5, ncomp=3, seed=0):
    return layered_tables(REGIONAL_LAT, REGIONAL_LON, nb, ncomp, seed)


def global_model(nb=5, ncomp=3, seed=0):
    return layered_tables(GLOBAL_LAT, GLOBAL_LON, nb, ncomp, seed, periodic=True)


def xyz(lat, lon, depth):
    """Points f64[..., 3] at geocentric latitude, longitude (degrees) and depth (m)."""
    lat, lon, depth = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (lat, lon, depth)))
    r, colat, lo = R_EARTH - depth, np.deg2rad(90.0 - lat), np.deg2rad(lon)
    return np.ascontiguousarray(np.stack([r * np.sin(colat) * np.cos(lo), r * np.sin(colat) * np.sin(lo), r * np.cos(colat)], axis=-1))


def cloud(n, seed=0, lat=(-8.0, 8.0), lon=(-8.0, 8.0), depth=(-6000.0, 60000.0)):
    """n points: most within the regional model, some outside it on every side."""
    rng = np.random.default_rng(seed)
    return xyz(rng.uniform(*lat, n), rng.uniform(*lon, n), rng.uniform(*depth, n)).reshape(n, 3)


def sphere_cloud(n, seed=0, depth=(-6000.0, 60000.0)):
    rng = np.random.default_rng(seed)
    return xyz(np.rad2deg(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n), rng.uniform(*depth, n)).reshape(n, 3)


def elements(G, P, seed=0, size=0.5, height=6000.0, lat=(-8.0, 8.0), lon=(-8.0, 8.0), depth=(-6000.0, 60000.0)):
    """G elements of P nodes f64[G, P, 3]: nodes scattered within ``size`` degrees and ``height`` metres of a centre."""
    rng = np.random.default_rng(seed)
    la, lo, de = rng.uniform(*lat, (G, 1)), rng.uniform(*lon, (G, 1)), rng.uniform(*depth, (G, 1))
    return xyz(la + rng.uniform(-size, size, (G, P)), lo + rng.uniform(-size, size, (G, P)), de + rng.uniform(-height, height, (G, P)))
