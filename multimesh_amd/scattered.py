"""Scattered point models: a model that is only points with values -- another code's element-nodal dump without its
connectivity, a tomography model on irregular nodes, borehole or profile picks, a sediment-thickness cloud -- onto arbitrary
points or onto the nodes of a mesh, on the GPU: the exact k nearest samples (``mm_knn_build`` / ``mm_knn_query``), then
inverse-distance weights relative to the nearest one (``mm_idw_gather``, where include/multimesh_hip.h states the arithmetic
bit for bit).  Imported explicitly (``from multimesh_amd import scattered``); the reference has no counterpart (its users go
through ``scipy.spatial.cKDTree`` and NumPy on the host).

A target's value depends on its own kNN row alone: neither the chunk size nor the copies of a node shared by several
elements can change a bit of it."""
from __future__ import annotations

import numpy as np

from .api._common import ImportTarget, latlondepth_to_xyz, name_list
from .device import default_context
from .helpers import MM_KNN_MAX_K

__all__ = ["PointCloud", "chunk_size", "interpolate_scattered", "import_point_cloud"]

#: bytes of idx + dist scratch (16 * k per target) one chunk of targets may take
SCRATCH_BYTES = 1 << 30


class PointCloud:
    """Points with values: ``points`` f64[n, ndim], ndim 1..3, and the named columns ``values`` -- a dict name -> f64[n], or
    an array f64[n, C] (or f64[n]) whose columns ``names`` names.  ``geocentric=True``: the rows of ``points`` are
    (geocentric latitude, longitude in degrees, depth in m below 6371 km) and go through
    :func:`multimesh_amd.api.latlondepth_to_xyz`.  Coordinates need not be finite: a sample with a NaN coordinate is never
    anybody's neighbour (``mm_knn_query``)."""

    def __init__(self, points, values, names=None, geocentric=False):
        pts = np.array(points, dtype=np.float64)
        if pts.ndim == 1:
            pts = pts[:, None]
        if pts.ndim != 2 or not 1 <= pts.shape[1] <= 3 or pts.shape[0] < 1:
            raise ValueError(f"points must be [n, ndim] with n >= 1 and ndim in 1..3, got {pts.shape}")
        if geocentric:
            if pts.shape[1] != 3:
                raise ValueError("geocentric points are rows of (latitude, longitude, depth)")
            pts = latlondepth_to_xyz(pts)
        self.points = np.ascontiguousarray(pts)
        if isinstance(values, dict):
            if names is not None and list(names) != list(values):
                raise ValueError("names with a dict of values must be its keys in order (or None)")
            names, columns = list(values), [np.asarray(v, dtype=np.float64) for v in values.values()]
        else:
            v = np.asarray(values, dtype=np.float64)
            if v.ndim == 1:
                v = v[:, None]
            if v.ndim != 2:
                raise ValueError(f"values must be [n, C], [n] or a dict of [n] columns, got {v.shape}")
            if names is None:
                raise ValueError("an array of values needs names for its columns")
            names = name_list(names, ())
            if len(names) != v.shape[1]:
                raise ValueError(f"{len(names)} names for {v.shape[1]} columns of values")
            columns = [v[:, c] for c in range(v.shape[1])]
        if not all(isinstance(p, str) for p in names) or len(set(names)) != len(names):
            raise ValueError("the names must be distinct strings")
        for p, col in zip(names, columns):
            if col.shape != (len(self.points),):
                raise ValueError(f"{p}: shape {col.shape}, the cloud has {len(self.points)} points")
        self.values = {p: np.ascontiguousarray(col, dtype=np.float64) for p, col in zip(names, columns)}
        self._index = None

    def __len__(self):
        return len(self.points)

    @property
    def ndim(self):
        return self.points.shape[1]

    @property
    def names(self):
        return list(self.values)

    def pick(self, params=None):
        """The names ``params`` asks for (None: all, a string: that one), checked against the cloud's."""
        names = name_list(params, self.names)
        unknown = [p for p in names if p not in self.values]
        if unknown:
            raise ValueError(f"parameters {unknown} are not in the cloud (it holds {self.names})")
        return names

    def fields(self, params=None):
        """f64[C, n]: one contiguous row per parameter, the layout ``mm_idw_gather`` reads."""
        names = self.pick(params)
        return np.ascontiguousarray(np.stack([self.values[p] for p in names])) if names else np.zeros((0, len(self)))

    def index(self, context=None):
        """The :class:`multimesh_amd.device.KnnIndex` over the points on ``context``, built once and kept (another context
        builds another)."""
        ctx = context or default_context()
        if self._index is None or self._index.ctx is not ctx or not self._index.handle:
            self._index = ctx.knn_build(self.points)
        return self._index


def chunk_size(npoints, k, scratch_bytes=SCRATCH_BYTES):
    """The targets of one chunk: as many as keep ``idx`` + ``dist`` (16 * k bytes per target) within ``scratch_bytes``, at
    least one, at most ``npoints`` (and one for no targets at all)."""
    if k < 1 or scratch_bytes < 1:
        raise ValueError("k and scratch_bytes must be positive")
    return int(max(1, min(int(npoints), int(scratch_bytes) // (16 * int(k)))))


def _settings(cloud, k, power, max_distance, outside, modes):
    """The checked (k, power, max_distance) of a call; ``ValueError`` before any device work."""
    if not isinstance(cloud, PointCloud):
        raise ValueError("cloud must be a PointCloud")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MM_KNN_MAX_K:
        raise ValueError(f"k must be an integer in 1..{MM_KNN_MAX_K}, got {k!r}")
    if isinstance(power, bool) or not isinstance(power, (int, np.integer)) or not 1 <= power <= 8:
        raise ValueError(f"power must be an integer in 1..8, got {power!r}")
    max_distance = np.inf if max_distance is None else float(max_distance)
    if not max_distance >= 0.0:
        raise ValueError("max_distance must not be negative or a NaN (None: no limit)")
    if outside not in modes:
        raise ValueError(f"outside must be one of {sorted(modes)}, got {outside!r}")
    return int(k), int(power), max_distance


def _targets(cloud, points):
    """(f64[N, ndim] contiguous, the leading shape) of target points [..., ndim] of the cloud's dimension."""
    pts = np.asarray(points, dtype=np.float64)
    if cloud.ndim == 1 and (pts.ndim == 0 or pts.shape[-1] != 1):
        pts = pts[..., None]
    if pts.ndim < 2 or pts.shape[-1] != cloud.ndim:
        raise ValueError(f"points must be [..., {cloud.ndim}] like the cloud's, got {pts.shape}")
    return np.ascontiguousarray(pts.reshape(-1, cloud.ndim)), pts.shape[:-1]


def _run(cloud, ctx, pts, names, k, power, max_distance, outside, fill_value, prior, point_major, chunk_points):
    """The chunks of one call: (values f64[N, C] or [C, N] on the host, nearest f64[N], the number of outside targets).
    prior: the host array "keep" starts from, in the layout of the values."""
    n, ncomp = len(pts), len(names)
    chunk = chunk_size(n, k) if chunk_points is None else int(chunk_points)
    if chunk < 1:
        raise ValueError("chunk_points must be positive")
    index = cloud.index(ctx)
    fields = ctx.to_device(cloud.fields(names))
    values = np.empty((n, ncomp) if point_major else (ncomp, n))
    nearest = np.empty(n)
    noutside = 0
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        idx, dist = index.query(pts[a:b], k, want_dist=True)
        out = None
        if outside == "keep":
            out = ctx.to_device(prior[a:b] if point_major else prior[:, a:b])
        out, miss, near = ctx.idw_gather(fields, idx, dist, power=power, max_distance=max_distance, outside=outside,
                                         fill_value=fill_value, out=out, point_major=point_major, want_nearest=True)
        noutside += miss
        if point_major:
            values[a:b] = out.numpy()
        else:
            values[:, a:b] = out.numpy()
        nearest[a:b] = near.numpy()
        for d in (idx, dist, out, near):
            d.free()
    fields.free()
    return values, nearest, noutside


def interpolate_scattered(cloud, points, params=None, k=8, power=2, max_distance=None, outside="fill", fill_value=np.nan,
                          context=None, chunk_points=None):
    """The cloud's columns ``params`` (None: all) at ``points`` f64[..., ndim]: ``(values f64[N, C], noutside)``.  Per
    target, the ``k`` nearest samples (exact, ties by index) weighted by ``(d0 / d) ** power`` with ``d0`` the nearest
    distance -- ``k=1`` is nearest neighbour, a target that is a sample gets that sample's bits --; samples farther than
    ``max_distance`` (None: no limit) do not take part, and a target without any is outside and holds ``fill_value``
    (``outside`` is "fill" here: :func:`import_point_cloud` has values to keep).  ``power`` is an integer in 1..8.  Targets
    go through in chunks of ``chunk_points`` (None: :func:`chunk_size`); the chunk size cannot change a bit."""
    k, power, max_distance = _settings(cloud, k, power, max_distance, outside, ("fill",))
    names = cloud.pick(params)
    pts, _ = _targets(cloud, points)
    if chunk_points is not None and int(chunk_points) < 1:
        raise ValueError("chunk_points must be positive")
    ctx = context or default_context()
    values, _, noutside = _run(cloud, ctx, pts, names, k, power, max_distance, "fill", fill_value, None, True, chunk_points)
    return values, noutside


def import_point_cloud(cloud, mesh, params=None, k=8, power=2, max_distance=None, outside="keep", blend=None, context=None,
                       *, fill_value=np.nan, chunk_points=None):
    """A scattered model onto a mesh: every node of ``mesh`` gets the cloud's value there, as
    :func:`interpolate_scattered` gives it.  ``mesh``:

    * a :class:`GllMesh`: ``element_nodal_fields[p]`` becomes a new f64[E, P] array;
    * a :class:`HexMesh`: nodal fields through ``attach_field``;
    * a writable Salvus model -- an h5py-like object (:class:`multimesh_amd.io.MemoryH5`) or, with h5py, a path: the columns
      of ``MODEL/data`` that ``DIMENSION_LABELS`` names are overwritten in place, every other column stays as it is.

    ``outside``: "keep" (default: nodes without a sample within ``max_distance`` keep the mesh's value; the field must
    exist, else ``ValueError``) or "fill" (``fill_value``).  ``blend=(inner, outer)`` softens the cloud's edge: the mesh
    takes the imported value within ``inner`` of the nearest sample, keeps its own beyond ``outer`` and the smoothstep of
    ``Context.distance_taper`` between (``a`` the mesh's values, ``b`` the imported ones); outside nodes have a nearest
    distance of +inf and keep the mesh's bits, whatever ``outside`` says.  Element-nodal nodes are not deduplicated: the
    copies of a shared node have equal coordinates, hence equal kNN rows, hence equal bits.  Returns the number of outside
    nodes."""
    k, power, max_distance = _settings(cloud, k, power, max_distance, outside, ("keep", "fill"))
    names = cloud.pick(params)
    if blend is not None:
        inner, outer = (float(r) for r in blend)
        if not (np.isfinite(inner) and np.isfinite(outer) and 0.0 <= inner <= outer):
            raise ValueError("blend = (inner, outer) needs 0 <= inner <= outer, both finite")
    needs_mesh_values = outside == "keep" or blend is not None

    with ImportTarget(mesh) as target:
        if target.points.shape[-1] != cloud.ndim:
            raise ValueError(f"the mesh is {target.points.shape[-1]}-D, the cloud {cloud.ndim}-D")
        target.require(names, values=needs_mesh_values)
        pts, _ = _targets(cloud, target.points)
        prior = target.existing(names).reshape(len(names), -1) if needs_mesh_values else None
        ctx = context or default_context()
        values, nearest, noutside = _run(cloud, ctx, pts, names, k, power, max_distance, outside, fill_value, prior, False,
                                         chunk_points)
        if blend is not None and names:
            values = ctx.distance_taper(nearest, inner, outer, prior, b=values)[0].numpy()
        target.write(names, values.reshape((len(names),) + target.lead))
    return noutside
