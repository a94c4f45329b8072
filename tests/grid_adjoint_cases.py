"""The NumPy statement of mm_grid_operator (include/multimesh_hip.h), of its transpose, of the fold back to the caller's
layout and of the chunk rule, and the inputs the grid-adjoint tests share.  Built on tests/grid_import_cases.py; nothing
here imports the code under test.

Per point, with (lat, lon, depth), the periodic wrap and per axis (i, i1, t, inside) exactly as grid_import_cases states
them for mm_sample_grid -- depth gives (k, k1, tz), latitude (j, j1, ty), longitude (i, i1, tx):

  corner c = 4 a + 2 b + e, a, b, e in {0, 1} selecting K = k|k1, J = j|j1, I = i|i1
  ids[n][c] = (K * nlat + J) * nlon + I             u(t, 0) = 1.0 - t, u(t, 1) = t
  w[n][c]   = (u(tz, a) * u(ty, b)) * u(tx, e)       every operation an array operation of its own
  a point outside the grid (clamp off; NaN is outside): ids 0 and w +0.0 in all eight slots, and it is counted

The transpose is np.add.at on zeros (tests/transpose_cases.py); the chunk rule adds the transposes of consecutive chunks
of points in ascending order, ((c0 + c1) + c2) + ...; the fold adds an appended closing longitude column onto column 0,
drops it, and flips flipped axes back.
"""
import numpy as np

import grid_import_cases as G

EPS = np.finfo(np.float64).eps


def cell(axis, v, clamp):
    """grid_import_cases.cell with the clamp written as the header writes it for the weights' sake: v = a[0] where
    v < a[0], then v = a[n-1] where v > a[n-1].  np.maximum(-0.0, +0.0) may return either zero; the comparisons leave a
    -0.0 on an axis that starts at +0.0 as it is, so that t = (-0.0 - 0.0) / h = -0.0 and the weights it multiplies keep
    that sign (mm_sample_grid's values cannot tell: t * q is added to a term)."""
    if not clamp or len(axis) == 1:
        return G.cell(axis, v, clamp)
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        v = np.where(v < axis[0], axis[0], v)
        v = np.where(v > axis[-1], axis[-1], v)
    i, i1, t, _ = G.cell(axis, v, False)
    return i, i1, t, np.ones(v.shape, dtype=bool)


def operator(depth, lat, lon, D, LA, LO, clamp=False, periodic=False):
    """-> (ids int64[N, 8], w f64[N, 8], noutside, inside bool[N]) at the points' (D, LA, LO)"""
    D, LA, LO = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (D, LA, LO))
    if periodic:
        LO = G.wrap(LO, lon[0])
    k, k1, tz, in_d = cell(depth, D, clamp)
    j, j1, ty, in_la = cell(lat, LA, clamp)
    i, i1, tx, in_lo = cell(lon, LO, clamp)
    inside = in_d & in_la & in_lo
    nla, nlo = len(lat), len(lon)
    ids = np.zeros((len(D), 8), dtype=np.int64)
    w = np.zeros((len(D), 8))
    uz, uy, ux = (1.0 - tz, tz), (1.0 - ty, ty), (1.0 - tx, tx)
    with np.errstate(invalid="ignore"):
        for c in range(8):
            a, b, e = c >> 2, (c >> 1) & 1, c & 1
            ids[:, c] = ((k1 if a else k) * nla + (j1 if b else j)) * nlo + (i1 if e else i)
            w[:, c] = (uz[a] * uy[b]) * ux[e]
    ids[~inside] = 0
    w[~inside] = 0.0
    return ids, w, int((~inside).sum()), inside


def transpose(ids, w, values, nsrc):
    """values f64[C, N] -> f64[C, nsrc]: np.add.at on zeros, component by component"""
    values = np.asarray(values, dtype=np.float64).reshape(-1, len(ids))
    out = np.zeros((values.shape[0], nsrc))
    with np.errstate(invalid="ignore"):
        for c in range(values.shape[0]):
            np.add.at(out[c], ids, w * values[c][:, None])
    return out


def chunked_transpose(ids, w, values, nsrc, chunk):
    """The chunk rule: transposes of consecutive chunks of ``chunk`` points, added in ascending order"""
    values = np.asarray(values, dtype=np.float64).reshape(-1, len(ids))
    total = np.zeros((values.shape[0], nsrc))
    for n, start in enumerate(range(0, len(ids), chunk)):
        stop = min(start + chunk, len(ids))
        part = transpose(ids[start:stop], w[start:stop], values[:, start:stop], nsrc)
        total = part if n == 0 else total + part
    return total


def gather(cube, ids, w):
    """cube f64[C, nsrc] -> f64[C, N]: np.sum(cube[c][ids] * w, axis=1), what mm_gather computes"""
    with np.errstate(invalid="ignore"):
        return np.stack([np.sum(g[ids] * w, axis=1) for g in cube]) if len(cube) else np.zeros((0, len(ids)))


def dense(ids, w, nsrc):
    """The operator as a matrix f64[N, nsrc] (ids repeated in a row add up)"""
    A = np.zeros((len(ids), nsrc))
    np.add.at(A, (np.arange(len(ids))[:, None], ids), w)
    return A


def to_prepared(values, flipped, appended):
    """f64[..., D, LA, LO] in the caller's layout -> the prepared layout: flipped axes reversed, column 0 repeated last"""
    v = np.asarray(values)
    for ax, f in zip((-3, -2, -1), flipped):
        if f:
            v = v[(Ellipsis, slice(None, None, -1)) + (slice(None),) * (-ax - 1)]
    if appended:
        v = np.concatenate([v, v[..., :1]], axis=-1)
    return np.ascontiguousarray(v)


def fold(values, flipped, appended):
    """The transpose of to_prepared: the closing column is added onto column 0 and dropped, flipped axes flipped back"""
    v = np.array(values, dtype=np.float64)
    if appended:
        v[..., 0] = v[..., 0] + v[..., -1]
        v = v[..., :-1]
    for ax, f in zip((-3, -2, -1), flipped):
        if f:
            v = v[(Ellipsis, slice(None, None, -1)) + (slice(None),) * (-ax - 1)]
    return np.ascontiguousarray(v)


# ------------------------------------------------------------------------------------------------ shared inputs
def xyz(lat, lon, depth):
    """(lat, lon, depth) -> f64[N, 3], the expressions of latlondepth_to_xyz"""
    lat, lon, depth = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (lat, lon, depth)))
    r = G.R_EARTH - depth.reshape(-1)
    colat, lo = np.deg2rad(90.0 - lat.reshape(-1)), np.deg2rad(lon.reshape(-1))
    return np.ascontiguousarray(np.stack([r * np.sin(colat) * np.cos(lo), r * np.sin(colat) * np.sin(lo), r * np.cos(colat)], axis=1))


def random_points(n, depth, lat, lon, margin, seed):
    """n points uniform in the box of the axes widened by ``margin`` of its span on every side of every axis that has one
    (0.075: about a third of the points fall outside a 3-D grid)"""
    rng = np.random.default_rng(seed)

    def draw(a):
        span = a[-1] - a[0]
        return rng.uniform(a[0] - margin * span, a[-1] + margin * span, n) if len(a) > 1 else np.full(n, a[0])

    return xyz(draw(lat), draw(lon), draw(depth))


def mixed_points(depth=G.DEPTH, lat=G.LAT, lon=G.LON, nrandom=1000, nface=300, seed=23):
    """About 2000 points: the seven axis points, the grid's own nodes, points on cell faces (one coordinate a node's, the
    others random inside), random points of which about a third fall outside, and one NaN row"""
    rng = np.random.default_rng(seed)
    d, la, lo = np.meshgrid(depth, lat, lon, indexing="ij")
    nodes = xyz(la, lo, d)
    faces = []
    for axis in range(3):
        coords = [rng.uniform(a[0], a[-1], nface // 3) if len(a) > 1 else np.full(nface // 3, a[0]) for a in (depth, lat, lon)]
        coords[axis] = rng.choice((depth, lat, lon)[axis], nface // 3)
        faces.append(xyz(coords[1], coords[2], coords[0]))
    rand = random_points(nrandom, depth, lat, lon, 0.075, seed + 1)
    nan_row = np.array([[6.0e6, np.nan, 1.0e5]])
    return np.ascontiguousarray(np.concatenate([G.AXIS_POINTS * 6.3e6, nodes] + faces + [rand, nan_row]))


def angle_difference(got, ref):
    """|got - ref| in degrees, a whole turn apart counting as equal (a longitude within rounding of the seam)"""
    d = np.abs(np.asarray(got) - np.asarray(ref))
    return np.minimum(d, np.abs(d - 360.0))
