"""Regions: outlines drawn on a map -- a continent, the area with ray coverage, the footprint of a regional model -- given as
rings of (lat, lon) vertices, and what the model tools do with them on the GPU: the inside flag and the signed distance to
the outline for every node (include/multimesh_regions.h: ``mm_region_distance``; the header holds the statement, operation by
operation, which the device reproduces bit for bit), masks, tapers and blends through ``mm_distance_taper``.  Imported
explicitly (``from multimesh_amd import regions``); the reference has no counterpart.

Geometry.  Vertices become unit vectors by :func:`multimesh_amd.api.latlondepth_to_xyz`'s expressions: latitude is geocentric,
``z`` is the pole, longitude runs from ``x`` towards ``y``, as in ``mm_sample_grid``.  Consecutive vertices are joined by the
shorter great-circle arc; rings, holes and several polygons are all just edges and inside is even-odd.  Only a node's
direction counts, so a region is a cone through all depths.

Distances.  The device measures CHORDS on the unit sphere and scales them by ``radius``.  Every length a caller gives here
(``cutoff_m``, ``taper_m``) is an ARC length on the sphere of ``radius`` and is converted with ``2 R sin(w / 2R)``; what comes
back is the chord in metres.  A smoothstep over the chord differs from one over the arc by ``theta**2 / 24`` relative
(``theta`` the taper width as an angle): 1.e-4 for a taper of 300 km on the Earth.

Rotated frames.  Every function here takes ``frames.in_frame(mesh, R)`` for an outline given in a rotated frame: the view's
points are the rotated ones and its field store is the mesh's own.

The symbol is an extension of the library's C ABI with a header of its own: this module keeps its signature table and applies
it to the handle of :func:`multimesh_amd.helpers.load_lib` on first use; the call itself goes through
:func:`multimesh_amd.device._call` and the :class:`Context` checks like every other call of the package."""
from __future__ import annotations

import numpy as np

from . import device as _device
from .api._common import R_EARTH, named_fields, points_of
from .device import default_context
from .helpers import f64, i32, i64, load_lib, vp

__all__ = ["Region", "region_distance_call", "region_distance", "contains", "region_mask", "taper_to_region", "blend_into",
           "statement", "MIN_RADIUS", "MAX_EDGES", "EDGE_CHUNK", "MIN_ANCHOR_CHORD", "MIN_EDGE_CHORD"]

MAX_EDGES = 1 << 20          # MM_REGION_MAX_EDGES
EDGE_CHUNK = 32              # MM_REGION_EDGE_CHUNK: the edges that share a bounding ball on the device
MIN_EDGE_CHORD = 2.0 ** -20  # consecutive vertices closer than this chord (6 m on the Earth), or that close to antipodal, are refused
MIN_ANCHOR_CHORD = 1e-3      # the anchor keeps this chord (6.4 km on the Earth) from the outline, or the region is refused
WGS84_FLATTENING = 1.0 / 298.257223563

#: name -> (restype, argtypes) of the function include/multimesh_regions.h declares (tests/test_regions.py compares it with
#: the header); it is not part of helpers.SIGNATURES, the table of include/multimesh_hip.h
SIGNATURES = {
    "mm_region_distance": (i64, (vp, vp, i64, i64, vp, i64, vp, i32, f64, f64, vp, vp, vp)),
}

#: (lat, lon) of the anchor candidates: generic directions -- no pole, no round-number parallel or meridian --, so that meshes
#: and boxes on whole degrees do not put nodes and vertices on one great circle through the anchor
ANCHOR_CANDIDATES = tuple((lat, lon + 7.3 * i) for i, lat in enumerate((17.318, -23.457, 41.713, -47.291, 68.937, -71.153))
                          for lon in (23.7131, 113.3719, -156.4687, -66.8113))


def bind(lib=None):
    """The library handle with :data:`SIGNATURES` applied (once)."""
    lib = lib or load_lib()
    if getattr(lib, "_regions_bound", False) is not True:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        lib._regions_bound = True
    return lib


# ------------------------------------------------------------------------------------------------- the statement in NumPy
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def edge_normals(U, V):
    """The N of the header for edges U -> V f64[E, 3]: ``c = cross(U, V); N = c / sqrt(dot(c, c))``."""
    c = _cross(U, V)
    return c / np.sqrt(_dot(c, c))[..., None]


MIN_RADIUS = 2.0 ** -500     # a node nearer the centre than this is invalid: its squares would leave the normal range


def statement(points, edges, anchor, anchor_inside, cutoff, scale, block=None):
    """The statement of include/multimesh_regions.h on the host, operation by operation: ``(signed f64[n], inside int32[n],
    ninside, nhit, ninvalid)`` for points f64[n, 3].  What :class:`Region` measures its anchor with.  The edges are taken in
    blocks of ``block`` (None: as many as keep a block near 2^18 edge-node pairs) as arrays [block, n]; q is a minimum and the
    crossings a sum, so the blocks change no bit (``block=1`` is the header's loop, edge by edge in ascending order)."""
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1, 9)
    a = np.asarray(anchor, dtype=np.float64)
    n = len(x)
    block = int(block) if block else max(1, (1 << 18) // max(n, 1))
    with np.errstate(all="ignore"):
        r = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        valid = np.isfinite(r) & (r >= MIN_RADIUS)
        p = np.where(valid[:, None], x / r[:, None], 0.0)
        m = _cross(p, a[None, :])
        q = np.full(n, cutoff * cutoff)
        hit = np.zeros(n, dtype=bool)
        ncross = np.zeros(n, dtype=np.int64)
        pb, mb = p[None], m[None]
        for first in range(0, len(edges), block):
            rows = edges[first:first + block]
            U, V, N = rows[:, None, 0:3], rows[:, None, 3:6], rows[:, None, 6:9]
            su, sv, tp, ta = _dot(mb, U), _dot(mb, V), _dot(N, pb), _dot(N, a[None, None, :])
            ncross += (((su >= 0) != (sv >= 0)) & ((tp >= 0) != (ta >= 0)) & ((ta >= 0) == (su >= 0))).sum(axis=0)
            w1, w2 = _dot(_cross(U, pb), N), _dot(_cross(pb, V), N)
            g = 1.0 - tp * tp
            g = np.where(g < 0.0, 0.0, g)
            circle = (2.0 * (tp * tp)) / (1.0 + np.sqrt(g))
            du, dv = pb - U, pb - V
            qe = np.where((w1 >= 0) & (w2 >= 0), circle, np.minimum(_dot(du, du), _dot(dv, dv))).min(axis=0)
            less = qe < q
            q = np.where(less, qe, q)
            hit |= less
        inside = np.where(valid, int(anchor_inside) ^ (ncross & 1), 0).astype(np.int32)
        d = np.where(hit, scale * np.sqrt(q), scale * cutoff)
        s = np.where(valid, np.where(inside == 1, d, -d), -(scale * cutoff))
    hit &= valid
    return s, inside, int(inside.sum()), int(hit.sum()), int((~valid).sum())


# ---------------------------------------------------------------------------------------------------------------- Region
def unit_vectors(latlon):
    """(lat, lon) in degrees f64[n, 2] -> unit vectors f64[n, 3], by ``latlondepth_to_xyz``'s expressions at radius 1."""
    latlon = np.asarray(latlon, dtype=np.float64)
    colat, lon = np.deg2rad(90.0 - latlon[:, 0]), np.deg2rad(latlon[:, 1])
    return np.array([np.sin(colat) * np.cos(lon), np.sin(colat) * np.sin(lon), np.cos(colat)]).T


def geocentric_latitude(lat_deg):
    """Geographic (geodetic) latitude -> geocentric, on the WGS84 ellipsoid: ``atan((1 - f)**2 tan(lat))``; the poles stay."""
    lat = np.asarray(lat_deg, dtype=np.float64)
    out = np.rad2deg(np.arctan((1.0 - WGS84_FLATTENING) ** 2 * np.tan(np.deg2rad(lat))))
    return np.where(np.abs(lat) == 90.0, lat, out)


def _ring_list(rings):
    if isinstance(rings, np.ndarray) and rings.ndim == 2:
        return [rings]
    rings = list(rings)
    if rings and np.ndim(rings[0]) == 1:
        return [np.asarray(rings)]
    return rings


class Region:
    """A region on the sphere bounded by rings of (lat, lon) vertices in degrees.

    ``rings``: one f64[n, 2] or a list of them; a closed ring (first vertex repeated at the end) is accepted.  Consecutive
    vertices are joined by the shorter great-circle arc (:meth:`densify` first for outlines meant as straight lines on a
    lat/lon map, such as parallels).  Several rings combine even-odd: a ring inside another is a hole.  ``geodetic=True``
    converts geographic to geocentric latitude with the WGS84 flattening first -- for the nodes of a mesh as it is, whose
    latitudes are geocentric.  On :func:`multimesh_amd.geodesy.as_geographic`'s view of a mesh the node latitudes ARE geodetic:
    there the outline keeps its geographic vertices, ``geodetic=False``.

    ``interior`` says which side is the region: "left" -- to the left of the FIRST ring walked in order, seen from outside the
    sphere (GeoJSON's counter-clockwise exterior rings and clockwise holes all agree on it); "smaller" -- each ring encloses
    its smaller side, whatever its orientation; ``(lat, lon)`` -- a point declared inside.  All three reduce to one boolean,
    ``anchor_inside``, computed once on the host.

    ``edges`` f64[E, 9] is the table the device reads (U, V, N per edge; both rows that share a vertex hold the same three
    doubles), ``anchor`` f64[3] the unit vector crossings are counted from: the one of :data:`ANCHOR_CANDIDATES` farthest from
    the outline, measured with :func:`statement`.  ``ValueError`` for a ring with fewer than 3 distinct vertices, values that
    are not finite, ``|lat| > 90``, consecutive vertices closer than :data:`MIN_EDGE_CHORD` or that close to antipodal, more than
    2^20 edges, or an outline that comes within :data:`MIN_ANCHOR_CHORD` of every candidate."""

    def __init__(self, rings, interior="left", geodetic=False):
        self.rings, self.interior, self.geodetic = [], interior, bool(geodetic)
        tables = []
        for ring in _ring_list(rings):
            ring = np.array(ring, dtype=np.float64)
            if ring.ndim != 2 or ring.shape[1] != 2:
                raise ValueError(f"a ring must be f64[n, 2] of (lat, lon), got {ring.shape}")
            if not np.isfinite(ring).all() or (np.abs(ring[:, 0]) > 90.0).any():
                raise ValueError("the vertices of a ring must be finite with |lat| <= 90")
            if len(ring) > 1 and np.array_equal(ring[0], ring[-1]):
                ring = ring[:-1]
            if len(np.unique(ring, axis=0)) < 3:
                raise ValueError("a ring needs at least 3 distinct vertices")
            self.rings.append(ring)
            latlon = ring if not geodetic else np.stack([geocentric_latitude(ring[:, 0]), ring[:, 1]], axis=1)
            U = unit_vectors(latlon)
            V = np.roll(U, -1, axis=0)
            d, s = U - V, U + V
            short = np.minimum(_dot(d, d), _dot(s, s)) < MIN_EDGE_CHORD ** 2
            if short.any():
                i = int(np.argmax(short))
                raise ValueError(f"vertices {i} and {(i + 1) % len(ring)} of a ring are equal or antipodal (closer than a chord of 2^-20)")
            tables.append(np.concatenate([U, V, edge_normals(U, V)], axis=1))
        if not tables:
            raise ValueError("a region needs at least one ring")
        self.edges = np.ascontiguousarray(np.concatenate(tables))
        self._ring_edges = np.cumsum([0] + [len(t) for t in tables])
        if len(self.edges) > MAX_EDGES:
            raise ValueError(f"a region holds at most 2^20 edges, got {len(self.edges)}")
        candidates = unit_vectors(np.array(ANCHOR_CANDIDATES))
        far = np.abs(statement(candidates, self.edges, candidates[0], 0, 2.0, 1.0)[0])   # (the distance does not depend on the anchor)
        best = int(np.argmax(far))
        self.anchor_distance = float(far[best])
        if not self.anchor_distance >= MIN_ANCHOR_CHORD:
            raise ValueError(f"the outline comes within a chord of {MIN_ANCHOR_CHORD} of every anchor candidate")
        self.anchor = np.ascontiguousarray(candidates[best])
        self.anchor_inside = self._anchor_status(interior)

    # ---- which side
    def _parity(self, point, edges):
        """Whether the arc anchor -> ``point`` crosses ``edges`` an odd number of times (the statement's count)."""
        return int(statement(point[None], edges, self.anchor, 0, 2.0, 1.0)[1][0])

    def _left_point(self, edges):
        """A point immediately to the left of one edge of a ring: off the edge's midpoint towards N by a thousandth of the
        edge, and verified to be nearer to that edge than to any other of the ring."""
        for row in edges:
            U, V, N = row[0:3], row[3:6], row[6:9]
            mid = U + V
            mid = mid / np.sqrt(_dot(mid, mid))
            step = 1e-3 * np.sqrt(_dot(U - V, U - V))
            L = mid + step * N
            L = L / np.sqrt(_dot(L, L))
            own = statement(L[None], row[None], self.anchor, 0, 2.0, 1.0)[0][0]
            if abs(own) > 0.0 and own == statement(L[None], edges, self.anchor, 0, 2.0, 1.0)[0][0]:
                return L
        raise ValueError("no edge of the ring has free space to its left: the ring is degenerate")

    @staticmethod
    def _left_area(edges):
        """The area to the left of a ring on the unit sphere: 2 pi minus the sum of its turning angles (Gauss-Bonnet)."""
        U, N = edges[:, 0:3], edges[:, 6:9]
        t_out = _cross(N, U)                                   # the direction of travel leaving U
        t_in = _cross(np.roll(N, 1, axis=0), U)                # ... and arriving at it along the previous edge
        turn = np.arctan2(_dot(U, _cross(t_in, t_out)), _dot(t_in, t_out))
        return 2.0 * np.pi - float(turn.sum())

    def _anchor_status(self, interior):
        if isinstance(interior, str) and interior == "left":
            first = self.edges[self._ring_edges[0]:self._ring_edges[1]]
            return 1 ^ self._parity(self._left_point(first), self.edges)
        if isinstance(interior, str) and interior == "smaller":
            status = 0
            for b, e in zip(self._ring_edges[:-1], self._ring_edges[1:]):
                ring = self.edges[b:e]
                in_left = 1 ^ self._parity(self._left_point(ring), ring)
                status ^= in_left if self._left_area(ring) < 2.0 * np.pi else 1 ^ in_left
            return status
        point = np.zeros(0) if isinstance(interior, str) else np.asarray(interior, dtype=np.float64)
        if point.shape != (2,) or not np.isfinite(point).all() or abs(point[0]) > 90.0:
            raise ValueError(f'interior must be "left", "smaller" or a (lat, lon) inside the region, got {interior!r}')
        if self.geodetic:
            point = np.array([geocentric_latitude(point[0]), point[1]])
        return 1 ^ self._parity(unit_vectors(point[None])[0], self.edges)

    # ---- builders
    def complement(self):
        """The same edges with the flag flipped: everything outside this region."""
        other = object.__new__(Region)
        other.__dict__.update(self.__dict__)
        other.anchor_inside = 1 ^ self.anchor_inside
        other.interior = None
        return other

    def densify(self, max_step_deg):
        """A region whose rings carry extra vertices along straight lines in (lat, lon), at most ``max_step_deg`` apart in either
        coordinate, so that outlines meant as lines on a lat/lon map (parallels) are followed.  Longitudes are taken as given:
        a side from 170 to 190 runs across the antimeridian.  Not for a region made by :meth:`complement`."""
        step = float(max_step_deg)
        if not step > 0.0 or self.interior is None:
            raise ValueError("densify needs a positive step and a region that was built from rings")
        return Region([self._densified(ring, step) for ring in self.rings], interior=self.interior, geodetic=self.geodetic)

    @staticmethod
    def _densified(ring, step):
        parts = []
        for a, b in zip(ring, np.roll(ring, -1, axis=0)):
            k = max(1, int(np.ceil(np.abs(b - a).max() / step)))
            t = np.arange(k)[:, None] / k
            parts.append(a[None] * (1.0 - t) + b[None] * t)
        return np.concatenate(parts)

    @classmethod
    def from_box(cls, lat0, lat1, lon0, lon1, step=1.0):
        """The lat/lon box ``[lat0, lat1] x [lon0, lon1]``, its sides densified to ``step`` degrees.  ``lon1 < lon0`` spans the
        antimeridian (170 to -170 is twenty degrees wide).  A side on a pole is a point and is refused."""
        lat0, lat1, lon0, lon1 = float(lat0), float(lat1), float(lon0), float(lon1)
        if not lat0 < lat1:
            raise ValueError("from_box needs lat0 < lat1")
        if lon1 <= lon0:
            lon1 += 360.0
        if lon1 - lon0 >= 360.0:
            raise ValueError("a box spans less than 360 degrees of longitude")
        ring = np.array([[lat0, lon0], [lat0, lon1], [lat1, lon1], [lat1, lon0]])     # counter-clockwise: the box is on the left
        if not float(step) > 0.0:
            raise ValueError("from_box needs a positive step")
        return cls(cls._densified(ring, float(step)), interior="left")

    @classmethod
    def circle(cls, lat, lon, radius_m, n=360, radius=R_EARTH):
        """The small circle of arc radius ``radius_m`` about (lat, lon) as ``n`` vertices, the centre's side inside."""
        delta = float(radius_m) / float(radius)
        if not 0.0 < delta < np.pi or int(n) < 3:
            raise ValueError("circle needs 0 < radius_m < pi * radius and n >= 3")
        c = unit_vectors(np.array([[lat, lon]], dtype=np.float64))[0]
        e1 = _cross(np.array([0.0, 0.0, 1.0]) if abs(c[2]) < 0.9 else np.array([1.0, 0.0, 0.0]), c)
        e1 = e1 / np.sqrt(_dot(e1, e1))
        e2 = _cross(c, e1)
        phi = 2.0 * np.pi * np.arange(int(n)) / int(n)
        v = np.cos(delta) * c[None] + np.sin(delta) * (np.cos(phi)[:, None] * e1[None] + np.sin(phi)[:, None] * e2[None])
        ring = np.stack([90.0 - np.rad2deg(np.arccos(np.clip(v[:, 2], -1.0, 1.0))), np.rad2deg(np.arctan2(v[:, 1], v[:, 0]))], axis=1)
        return cls(ring, interior=(float(lat), float(lon)))


# -------------------------------------------------------------------------------------------------------------- the call
def region_distance_call(ctx, points, edges, anchor, anchor_inside, cutoff, scale, want_signed=True, want_inside=False,
                         want_info=False, signed_out=None, inside_out=None):
    """``mm_region_distance`` on the context ``ctx``: ``points`` f64[G, P, 3] (P <= 256) or f64[N, 3]; ``edges`` f64[E, 9] and
    ``anchor`` f64[3] as :class:`Region` holds them; ``cutoff`` a chord on the unit sphere in (0, 2]; ``scale`` metres per
    unit chord.  Every array may be a host array, a :class:`DeviceArray` or a torch-like tensor on the GPU.  Returns
    ``(result, ninside)`` with result a dict of device arrays: "signed" f64 and "inside" int32 in the points' leading shape,
    "info" int64[2] = (nodes with hit, invalid nodes), as asked for (``signed_out`` / ``inside_out``: the caller's arrays).
    ``ValueError`` with the library's message for what it refuses; nothing is written then.  Synchronises."""
    lib = bind(ctx.lib)
    pts, ngroups, P = ctx._node_groups(points)
    e = ctx.asdevice(edges, np.float64)
    if len(e.shape) != 2 or e.shape[1] != 9:
        raise ValueError(f"edges must be f64[E, 9], got {e.shape}")
    a = ctx.asdevice(anchor, np.float64)
    if a.size != 3:
        raise ValueError("anchor must be f64[3]")
    lead = pts.shape[:-1]
    res = {"signed": signed_out if signed_out is not None else ctx._wanted(want_signed, lead),
           "inside": inside_out if inside_out is not None else ctx._wanted(want_inside, lead, np.int32),
           "info": ctx._wanted(want_info, (2,), np.int64)}
    for key, dtype in (("signed", np.float64), ("inside", np.int32)):
        if res[key] is not None:
            res[key] = ctx.asdevice(res[key], dtype)
            if res[key].size != ngroups * P:
                raise ValueError(f"{key}_out must hold one value per node")
    rc = _device._call(lib, "mm_region_distance", ctx.handle, pts, ngroups, P, e, e.shape[0], a, int(anchor_inside), float(cutoff),
                       float(scale), res["signed"], res["inside"], res["info"], arg_error=True)
    return {k: v for k, v in res.items() if v is not None}, int(rc)


def arc_to_chord(arc_m, radius=R_EARTH):
    """The chord in metres of an arc length on the sphere of ``radius``: ``2 R sin(w / 2R)``."""
    return 2.0 * radius * np.sin(float(arc_m) / (2.0 * radius))


def _nodes(mesh_or_points):
    """(host points f64[G, P, 3] or [N, 3] as the call takes them, the leading shape of the caller's points)."""
    pts = points_of(mesh_or_points)
    if pts.ndim < 2 or pts.shape[-1] != 3:
        raise ValueError(f"regions need 3-D points [..., 3], got {pts.shape}")
    lead = pts.shape[:-1]
    if pts.ndim != 3 or pts.shape[1] > 256:
        pts = pts.reshape(-1, 3)
    return pts, lead


def _unit_cutoff(length_m, radius):
    length_m, radius = float(length_m), float(radius)
    if not (np.isfinite(radius) and radius > 0.0):
        raise ValueError("radius must be positive and finite")
    if not (np.isfinite(length_m) and 0.0 <= length_m <= np.pi * radius):
        raise ValueError("a length must lie in [0, pi * radius] and be finite")
    return arc_to_chord(length_m, radius) / radius


def _signed(ctx, pts, lead, region, unit_cutoff, radius, want_inside=False):
    out = ctx.empty(lead, np.float64)
    flags = ctx.empty(lead, np.int32) if want_inside else None
    _, ninside = region_distance_call(ctx, pts, region.edges, region.anchor, region.anchor_inside, unit_cutoff, float(radius),
                                      signed_out=out, inside_out=flags, want_signed=False)
    return out, flags, ninside


def region_distance(mesh_or_points, region, cutoff_m, radius=R_EARTH, context=None):
    """The signed distance of every node of a mesh (a :class:`GllMesh`, :class:`HexMesh`, Salvus mesh object) or of points
    f64[..., 3] to the outline of ``region``, on the device in the node shape: positive inside, negative outside,
    ``+-chord(cutoff_m)`` where the outline is farther than ``cutoff_m``.  ``cutoff_m`` is an arc length in metres on the sphere
    of ``radius`` and is converted with ``2 R sin(w / 2R)``; the value is the CHORD in metres on that sphere, bit for bit the
    statement of include/multimesh_regions.h.  Nodes at the centre or with coordinates that are not finite get
    ``-chord(cutoff_m)``."""
    unit = _unit_cutoff(cutoff_m, radius)
    if not unit > 0.0:
        raise ValueError("cutoff_m must be positive")
    pts, lead = _nodes(mesh_or_points)
    return _signed(context or default_context(), pts, lead, region, unit, radius)[0]


def contains(mesh_or_points, region, context=None):
    """Whether every node lies inside ``region``: int32 (0 / 1) on the device in the node shape."""
    pts, lead = _nodes(mesh_or_points)
    ctx = context or default_context()
    res, _ = region_distance_call(ctx, pts, region.edges, region.anchor, region.anchor_inside, 2.0 ** -20, 1.0, want_signed=False,
                                  inside_out=ctx.empty(lead, np.int32))
    return res["inside"]


_HARD_CUT = 2.0 ** -20    # the cutoff of a call that only needs the sign of the distance


def _weight_distance(ctx, mesh_or_points, region, taper_m, radius):
    """(signed distance on the device, outer): the distance up to the taper's width, and that width as the chord in metres
    the device itself reports for a node beyond it (``scale * cutoff``), so that such a node has weight exactly 1."""
    unit = _unit_cutoff(taper_m, radius)
    pts, lead = _nodes(mesh_or_points)
    dist, _, _ = _signed(ctx, pts, lead, region, unit if unit > 0.0 else _HARD_CUT, radius)
    return dist, float(radius) * unit


def region_mask(mesh_or_points, region, taper_m=0.0, radius=R_EARTH, context=None):
    """The weight of ``region`` on every node, f64 on the device in the node shape: 1 deeper than ``taper_m`` (an arc length)
    inside, 0 on the outline and outside, ``mm_distance_taper``'s smoothstep of the chord distance between.  ``taper_m = 0`` is
    a hard cut."""
    ctx = context or default_context()
    dist, outer = _weight_distance(ctx, mesh_or_points, region, taper_m, radius)
    return ctx.distance_taper(dist, 0.0, outer, None, want_weight=True)[2]


def taper_to_region(mesh, params, region, taper_m, radius=R_EARTH, context=None):
    """The fields ``params`` of ``mesh`` restricted to ``region``: ``(values, ntapered)`` as
    :func:`multimesh_amd.boundary.taper_to_boundary` gives them -- new host arrays f64[C, E, P] (a :class:`HexMesh`: [C, N]), the
    mesh's fields are untouched -- times :func:`region_mask`'s weight; ``ntapered`` counts the nodes whose weight is below 1.
    Nodes at weight 1 keep their bits."""
    ctx = context or default_context()
    _, fields = named_fields(mesh, params)
    dist, outer = _weight_distance(ctx, mesh, region, taper_m, radius)
    out, ntapered = ctx.distance_taper(dist, 0.0, outer, fields.reshape(fields.shape[0], -1))
    return out.numpy().reshape(fields.shape), ntapered


def blend_into(host_mesh, params, values, region, taper_m, located=None, radius=R_EARTH, context=None):
    """A regional model blended into the fields ``params`` of ``host_mesh`` along the outline of ``region``: ``(values, info)``
    with, for :func:`region_mask`'s weight ``w``::

        out = host where w == 0,  values where w == 1,  (w * values) + ((1 - w) * host)  between

    through ``mm_distance_taper``'s blend, so host nodes outside keep their bits and nodes deeper than ``taper_m`` carry
    ``values``.  ``values``: f64[C, ...] on the host's nodes, e.g. what ``import_regular_grid``, ``import_point_cloud`` or
    ``import_harmonic_model`` wrote into a copy of the mesh.  ``located``: an ``elem``-like integer array over the nodes or None;
    a negative entry means weight 0 (the regional model has no value there).  ``info = {"nblended", "nreplaced"}``: the nodes
    with 0 < w < 1 and with w == 1.  This is :func:`multimesh_amd.boundary.blend_models` for regional models that are not
    meshes.  New host arrays; the mesh's fields are untouched."""
    ctx = context or default_context()
    _, f_h = named_fields(host_mesh, params)
    a = np.ascontiguousarray(values, dtype=np.float64)
    if a.size != f_h.size:
        raise ValueError(f"values must hold one value per field and node of the host ({f_h.shape}), got {a.shape}")
    dist, outer = _weight_distance(ctx, host_mesh, region, taper_m, radius)
    elem = None
    if located is not None:
        elem = np.ascontiguousarray(located, dtype=np.int64)
        if elem.size != dist.size:
            raise ValueError("located must hold one entry per node")
    out, _, w = ctx.distance_taper(dist, 0.0, outer, a.reshape(f_h.shape[0], -1), b=f_h.reshape(f_h.shape[0], -1), elem=elem,
                                   want_weight=True)
    w = w.numpy()
    info = {"nblended": int(((w > 0.0) & (w < 1.0)).sum()), "nreplaced": int((w == 1.0).sum())}
    return out.numpy().reshape(f_h.shape), info
