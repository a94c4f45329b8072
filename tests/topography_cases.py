"""The NumPy statement of mm_radial_stretch (include/multimesh_topography.h), written from the header and not from the kernel,
and the small maps and point sets the topography tests share.  Nothing here imports the code under test.

The device's acos and atan2 are the only part that cannot be bit for bit, so the statement starts from the (lat, lon) the
device handed back (``lld``) and from r = |p|, which has no libm in it; everything after them is one NumPy operation per
operation of the header, in float64 -- or, with ``dtype=np.longdouble``, the same expressions in extended precision, the
reference the CPU tests hold the float64 statement to.

  radius     r = sqrt((x*x + y*y) + z*z)
  stretch    the whole statement: (points_out, radius_out, noutside)
  displace   steps 3 and 4 alone, on given columns: the new radius of every node
"""
import numpy as np

from layered_cases import R_EARTH, cell, columns, latlondepth, lerp, same_bits_nan, wrap, xyz  # noqa: F401  (re-exported)

APPLY, FLATTEN = 0, 1
CELL, BILINEAR = 0, 1
KEEP, CLAMP = 0, 1
MAX_NA = 64


def radius(points):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def displace(radii, anchors, s, direction, dtype=np.float64):
    """Steps 3 and 4: ``radii`` [N] (apply: rho; flatten: r), ``anchors`` [na], ``s`` [N, na] the shifts of every node's
    column -> the new radius [N] (apply: r' = rho + d; flatten: rho)."""
    x = np.asarray(radii, dtype=dtype).reshape(-1)
    A = np.asarray(anchors, dtype=dtype)
    s = np.asarray(s, dtype=dtype)
    rows = np.arange(len(x))
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        levels = np.broadcast_to(A, s.shape) if direction == APPLY else A[None, :] + s       # A_j, or B_j = A_j + s_j
        ge = x[:, None] >= levels
        above, found = ge[:, 0], ge[:, 1:].any(axis=1)
        j = np.argmax(ge[:, 1:], axis=1)                                                     # the first j with x >= level_{j+1}
        u = (x - levels[rows, j + 1]) / (levels[rows, j] - levels[rows, j + 1])
        if direction == APPLY:
            mid = x + ((one - u) * s[rows, j + 1] + u * s[rows, j])
            return np.where(above, x + s[:, 0], np.where(found, mid, x + s[:, -1]))
        mid = (one - u) * A[j + 1] + u * A[j]
        return np.where(above, x - s[:, 0], np.where(found, mid, x - s[:, -1]))


def stretch(lld, r, points, ref_radius, lat, lon, anchors, shifts, direction=APPLY, lateral=BILINEAR, outside=KEEP):
    """lld f64[N, 3] = the device's (lat, lon, depth) (the depth is not read); r f64[N] = |p|; points f64[N, 3]; ref_radius
    f64[N] or None; shifts f64[nlat, nlon, na].  -> (points_out f64[N, 3], radius_out f64[N], noutside)."""
    lld = np.asarray(lld, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    LA, LO = lld[:, 0], lld[:, 1]
    clamp = outside == CLAMP
    with np.errstate(all="ignore"):
        ca, co = cell(lat, LA, clamp), cell(lon, LO, clamp)
        valid = ~np.isnan(LA) & ~np.isnan(LO) & (r > 0.0) & ca[3] & co[3]
        s = columns(np.asarray(shifts, dtype=np.float64), ca, co, lateral)                   # [N, na]
        start = r if (direction == FLATTEN or ref_radius is None) else np.asarray(ref_radius, dtype=np.float64).reshape(-1)
        new = displace(start, anchors, s, direction)
        scale = new / r
        moved = p * scale[:, None]
    out = np.where(valid[:, None], moved, p)
    return out, np.where(valid, new, r), int((~valid).sum())


def device_view(points, lon, periodic):
    """NumPy's own (lld, r) of the points: what the statement starts from when no device is at hand."""
    with np.errstate(all="ignore"):
        lld = latlondepth(points)
        if periodic:
            lld[:, 1] = wrap(lld[:, 1], lon[0])
    return lld, radius(points)


# ------------------------------------------------------------------------------------------------------- shared inputs
REGIONAL_LAT = np.array([-6.0, -4.5, -2.0, 0.0, 1.5, 4.0, 6.0])                       # 7, non-uniform
REGIONAL_LON = np.array([-5.5, -4.0, -3.0, -1.0, 0.0, 1.5, 3.0, 5.0, 6.5])           # 9
GLOBAL_LAT = np.linspace(-90.0, 90.0, 6)
GLOBAL_LON = np.arange(-180.0, 180.0, 30.0)                                           # 12: the closing column is appended


def anchor_radii(na, spacing=6000.0):
    """na anchors from 6371000 m down, ``spacing`` apart but for a thin second interval (half of it)."""
    gaps = np.full(na - 1, spacing)
    if na > 2:
        gaps[1] = 0.5 * spacing
    return R_EARTH - np.concatenate([[0.0], np.cumsum(gaps)])


def interface_tables(lat, lon, na, seed=0, periodic=False, spacing=6000.0, thinnest=500.0):
    """(lat, lon, anchors f64[na], shifts f64[nlat, nlon, na]) as the device reads them: random shifts of either sign, small
    enough that the deformed layers of every column stay at least ``thinnest`` thick (so do their bilinear blends, which are
    convex combinations).  ``periodic``: ``lon`` goes once round without its closing column, which is appended here."""
    rng = np.random.default_rng(seed)
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    anchors = anchor_radii(na, spacing)
    amp = 0.5 * (np.min(-np.diff(anchors)) - thinnest)
    shifts = rng.uniform(-amp, amp, (len(lat), len(lon), na))
    if periodic:
        lon = np.concatenate([lon, [lon[0] + 360.0]])
        shifts = np.concatenate([shifts, shifts[:, :1]], axis=1)
    assert (np.diff(anchors[None, None, :] + shifts, axis=2) <= -thinnest).all()
    return lat, lon, anchors, np.ascontiguousarray(shifts)


def regional(na=5, seed=0, **kw):
    return interface_tables(REGIONAL_LAT, REGIONAL_LON, na, seed, **kw)


def global_map(na=5, seed=0, **kw):
    return interface_tables(GLOBAL_LAT, GLOBAL_LON, na, seed, periodic=True, **kw)


def depth_span(anchors, margin=8000.0):
    """Depths from above the top anchor to below the bottom one."""
    return (R_EARTH - anchors[0] - margin, R_EARTH - anchors[-1] + margin)


def cloud(n, anchors, seed=0, lat=(-8.0, 8.0), lon=(-8.0, 8.0)):
    """n points f64[n, 3]: most within the regional map, some outside it on every side; radii from above the top anchor to
    below the bottom one."""
    rng = np.random.default_rng(seed)
    return xyz(rng.uniform(*lat, n), rng.uniform(*lon, n), rng.uniform(*depth_span(anchors), n)).reshape(n, 3)


def sphere_cloud(n, anchors, seed=0):
    rng = np.random.default_rng(seed)
    return xyz(np.rad2deg(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n),
               rng.uniform(*depth_span(anchors), n)).reshape(n, 3)


def elements(G, P, anchors, seed=0, size=0.5, height=6000.0, lat=(-8.0, 8.0), lon=(-8.0, 8.0)):
    """G elements of P nodes f64[G, P, 3]: nodes scattered within ``size`` degrees and ``height`` metres of a centre."""
    rng = np.random.default_rng(seed)
    la, lo = rng.uniform(*lat, (G, 1)), rng.uniform(*lon, (G, 1))
    de = rng.uniform(*depth_span(anchors), (G, 1))
    return xyz(la + rng.uniform(-size, size, (G, P)), lo + rng.uniform(-size, size, (G, P)), de + rng.uniform(-height, height, (G, P)))


def column_radii(anchors, s, n, seed=0, margin=4000.0):
    """n reference radii per column of ``s`` [C, na], from ``margin`` below the bottom anchor to ``margin`` above the top: [C * n]
    radii and the matching rows of s [C * n, na]."""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(anchors[-1] - margin, anchors[0] + margin, (len(s), n))
    return rho.reshape(-1), np.repeat(s, n, axis=0)


# ------------------------------------------------------------------------------------- under guarded allocations
def guarded_model(kind):
    """(lat, lon, anchors, shifts, periodic): ``regional`` with even axes (6 and 8 values: granules) and na = 4 (anchors a
    granule), ``odd`` (7 and 9 values, na = 5: neither), ``global`` (6 latitudes, 12 + 1 longitudes once round, na = 5),
    ``pages`` (a latitude axis of 512 values, one page; 2 longitudes; na = 4: shifts of 512 * 2 * 4 doubles, eight pages)."""
    if kind == "global":
        return global_map(5, seed=2) + (True,)
    if kind == "regional":
        return interface_tables(REGIONAL_LAT[:6], REGIONAL_LON[:8], 4, seed=1) + (False,)
    if kind == "pages":
        return interface_tables(np.linspace(-6.0, 6.0, 512), np.array([-5.5, 6.5]), 4, seed=4) + (False,)
    return regional(5, seed=3) + (False,)


def guarded_points(kind, n, anchors, seed):
    """f64[n, 3]: past every edge of a regional map, all round a global one.  The first nodes: below the bottom anchor and
    above the top one in (or, past the edge, clamped onto) the LAST row and column -- on a global map in the cell that closes
    the round --, and one on the x axis exactly on the bottom anchor."""
    pts = sphere_cloud(n, anchors, seed) if kind == "global" else cloud(n, anchors, seed)
    low, high = R_EARTH - anchors[-1] + 5000.0, R_EARTH - anchors[0] - 3000.0
    corner = (80.0, 179.0) if kind == "global" else (5.99, 6.4)
    pts[0] = xyz(*corner, low)
    pts[1] = xyz(*corner, high)
    pts[2] = [anchors[-1], 0.0, 0.0]
    if kind != "global":
        pts[3] = xyz(7.5, 7.5, low)                      # past both edges: clamped onto the last row and column
    return np.ascontiguousarray(pts)


def guarded_cases():
    """mm_radial_stretch under guarded allocations; the test runs every case in both directions, both lateral modes and both
    outside modes.  Points of 8, 101 and 1024 nodes: 24 n bytes = a granule, neither, six pages."""
    out = []
    for kind, n in (("regional", 8), ("odd", 101), ("global", 1024), ("global", 101), ("pages", 8), ("odd", 1024)):
        lat, lon, anchors, shifts, periodic = guarded_model(kind)
        pts = guarded_points(kind, n, anchors, seed=n + len(kind))
        ref = radius(pts) + 10.0
        out.append(dict(name=f"{kind} n={n}", points=pts, ref=ref, lat=lat, lon=lon, anchors=anchors, shifts=shifts,
                        periodic=periodic, arrays=dict(points=pts, ref=ref, lat=lat, lon=lon, anchors=anchors, shifts=shifts)))
    return out


def guarded_edge_counts(case):
    """By the statement's own cells on NumPy's coordinates (the device's differ from them by a rounding of acos / atan2)."""
    lat, lon, A = case["lat"], case["lon"], case["anchors"]
    lld, r = device_view(case["points"], lon, case["periodic"])
    ca, co = cell(lat, lld[:, 0], True), cell(lon, lld[:, 1], True)
    last = (ca[1] == len(lat) - 1) & (co[1] == len(lon) - 1)
    off = (lld[:, 0] > lat[-1]) & (lld[:, 1] > lon[-1])
    counts = {"last row": int((ca[1] == len(lat) - 1).sum()), "last column": int((co[1] == len(lon) - 1).sum()),
              "last anchor of the last column": int((last & (r < A[-1])).sum()), "above the top there": int((last & (r >= A[0])).sum()),
              "on the bottom anchor": int((r == A[-1]).sum())}
    if case["periodic"]:
        counts["seam"] = int((co[0] == len(lon) - 2).sum())          # the cell that closes the round
    else:
        counts["clamped onto the corner"] = int(off.sum())
    return counts
