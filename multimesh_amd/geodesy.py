"""Geographic (geodetic) coordinates: meshes and points seen on an ellipsoid of revolution, on the GPU
(include/multimesh_geodesy.h: ``mm_geographic_points``; the header holds the statement, operation by operation -- only
``+ - * / sqrt`` --, which the device reproduces bit for bit).  Imported explicitly (``from multimesh_amd import geodesy``).

Every model tool of the package reads a model at a node's GEOCENTRIC latitude and at the depth ``6371000 - |p|``.  The
models those tools serve -- crustal columns, regional tomographies on lat/lon/depth cubes, coastlines -- are published in
GEOGRAPHIC coordinates: geodetic latitude, depth below the reference ellipsoid.  On an elliptical mesh (a Salvus mesh,
``synth.earth_chunk(ellipticity=...)``) the two differ by up to 0.19 degrees and by -7 km (equator) to +14 km (poles).

The GEOGRAPHIC VIEW of a point ``p`` is the pseudo-point ``p'`` whose geocentric latitude is the geodetic latitude of ``p``,
whose longitude is that of ``p`` and whose radius is ``6371000 + h``, ``h`` the height of ``p`` above the ellipsoid.  A tool
that reads ``p'`` reads (geodetic latitude, longitude, depth below the ellipsoid) of ``p`` with no change of its own:
:func:`as_geographic` hands any import a mesh whose points are the pseudo-points and whose field store is the original's, as
:func:`multimesh_amd.frames.in_frame` does for rotated frames.  :func:`geographic_points` and
:func:`extract_geographic_grid` go the other way: geodetic rows to Cartesian points, and a model onto geodetic axes.

The symbol is an extension of the library's C ABI with a header of its own: this module keeps its signature table and
applies it to the handle of :func:`multimesh_amd.helpers.load_lib` on first use; the call goes through
:func:`multimesh_amd.device._call` and the :class:`Context` checks like every other call of the package."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np

from . import device as _device
from .api._common import R_EARTH, GllMesh, _mesh_points, is_mesh, latlondepth_to_xyz
from .api.earth import _sphere_layout
from .api.gll import interpolate_gll_to_points
from .api.grids import RegularGrid
from .device import default_context
from .helpers import i32, i64, load_lib, vp
from .mesh import HexMesh

__all__ = ["Ellipsoid", "to_geographic", "from_geographic", "geodetic_coordinates", "as_geographic", "geographic_points",
           "extract_geographic_grid", "geographic_points_on_device", "WGS84_A", "WGS84_F", "TO_GEOGRAPHIC", "TO_CARTESIAN"]

WGS84_A = 6378137.0
WGS84_F = 1.0 / 298.257223563
TO_GEOGRAPHIC, TO_CARTESIAN = 0, 1      # MM_GEODESY_TO_*
NCONST = 8                              # MM_GEODESY_NCONST
#: the grid points :func:`extract_geographic_grid` interpolates at a time unless told otherwise
CHUNK_POINTS = 4_000_000

#: name -> (restype, argtypes) of the function include/multimesh_geodesy.h declares (tests/test_geodesy.py compares it with
#: the header); it is not part of helpers.SIGNATURES, the table of include/multimesh_hip.h
SIGNATURES = {
    "mm_geographic_points": (i32, (vp, i64, vp, vp, vp, i32, vp, vp)),
}


def bind(lib=None):
    """The library handle with :data:`SIGNATURES` applied (once)."""
    lib = lib or load_lib()
    if getattr(lib, "_geodesy_bound", False) is not True:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        lib._geodesy_bound = True
    return lib


# -------------------------------------------------------------------------------------------------------- the ellipsoid
class Ellipsoid:
    """An ellipsoid of revolution about ``z``: semi-major axis ``a`` (m) and flattening ``f`` (``b = a (1 - f)``).
    ``ValueError`` for values that are not finite, ``a <= 0`` and ``f`` outside ``[0, 0.5)``."""

    def __init__(self, a, f):
        a, f = np.float64(a), np.float64(f)
        if not (np.isfinite(a) and np.isfinite(f)):
            raise ValueError(f"an ellipsoid needs a finite a and f, got ({a}, {f})")
        if not a > 0.0:
            raise ValueError(f"the semi-major axis must be positive, got {a}")
        if not 0.0 <= f < 0.5:
            raise ValueError(f"the flattening must lie in [0, 0.5), got {f}")
        self.a, self.f = a, f

    @classmethod
    def wgs84(cls):
        return cls(WGS84_A, WGS84_F)

    @classmethod
    def from_mean_radius(cls, radius=R_EARTH, f=WGS84_F):
        """The sphere of ``radius`` flattened at equal volume: ``a = radius / (1 - f)^(1/3)``.  With the package's
        6371000 m this is the shape of ``synth.earth_chunk(ellipticity=f)`` to first order in ``f``."""
        radius, f = np.float64(radius), np.float64(f)
        if not (np.isfinite(f) and 0.0 <= f < 0.5):
            raise ValueError(f"the flattening must lie in [0, 0.5), got {f}")
        return cls(radius / np.cbrt(1.0 - f), f)

    @property
    def b(self):
        return self.a * (1.0 - self.f)

    @property
    def e2(self):
        return self.f * (2.0 - self.f)

    def constants(self, sphere_radius=R_EARTH):
        """The eight doubles ``mm_geographic_points`` reads, formed here in NumPy scalars (the kernel derives nothing):
        ``a, b, e2, 1 - e2, 1 - f, ep2b = (a*a - b*b) / b, e2a = e2 * a, R = sphere_radius``."""
        R = np.float64(sphere_radius)
        if not (np.isfinite(R) and R > 0.0):
            raise ValueError(f"sphere_radius must be finite and positive, got {sphere_radius}")
        a, b, e2 = self.a, self.b, self.e2
        return np.array([a, b, e2, 1.0 - e2, 1.0 - self.f, (a * a - b * b) / b, e2 * a, R], dtype=np.float64)

    def __repr__(self):
        return f"Ellipsoid(a={float(self.a)!r}, f={float(self.f)!r})"


def _constants(ellipsoid):
    """f64[8] of an :class:`Ellipsoid`, or eight doubles given as they are (what they hold is the library's to refuse)."""
    if isinstance(ellipsoid, Ellipsoid):
        return ellipsoid.constants()
    ell = np.ascontiguousarray(ellipsoid, dtype=np.float64)
    if ell.shape != (NCONST,):
        raise ValueError(f"an ellipsoid is an Ellipsoid or its {NCONST} constants, got {ell.shape}")
    return ell


# ------------------------------------------------------------------------------------------------------------- the call
def _is_device(ctx, x):
    return isinstance(x, _device.DeviceArray) or (hasattr(x, "data_ptr") and hasattr(x, "shape") and not ctx._on_host(x))


def geographic_points_on_device(ctx, points, ellipsoid, direction=TO_GEOGRAPHIC, out=None, radius=None, height_out=None):
    """``mm_geographic_points`` on the context ``ctx``: ``points`` f64[..., 3] (a host array, a :class:`DeviceArray` or a
    torch-like tensor on the GPU) to their geographic view (``direction`` 0) or back (1), into ``out`` -- a device array of
    as many values, which may be ``points`` itself, or None: a new one.  Direction 0 only: ``radius`` f64[...], one per
    point, replaces ``R + height`` as the pseudo-point's radius; ``height_out``, a device array of one value per point,
    receives the heights.  Returns the device array.  Runs on the context's stream and does not synchronise;
    ``ValueError`` with the library's message for what it refuses."""
    lib = bind(ctx.lib)
    pts, n = ctx._points3(points)
    ell = _constants(ellipsoid)
    out = ctx._out(out, pts.shape, "out must hold as many values as points", size_only=True)
    if radius is not None:
        radius = ctx.asdevice(radius, np.float64)
        if radius.size != n:
            raise ValueError(f"radius needs one value per point ({n}), got {radius.shape}")
    if height_out is not None:
        height_out = ctx._out(height_out, pts.shape[:-1], "height_out needs one value per point", size_only=True)
    _device._call(lib, "mm_geographic_points", ctx.handle, n, pts, out, (C.c_double * NCONST)(*ell), int(direction), radius,
                  height_out, arg_error=True)
    return out


def _apply(points, ellipsoid, direction, radius, out, height_out, context):
    """The contract of :meth:`multimesh_amd.frames.Rotation.apply` for both directions."""
    ctx = context or default_context()
    if _is_device(ctx, points):
        return geographic_points_on_device(ctx, points, ellipsoid, direction, out=out, radius=radius, height_out=height_out)
    host = np.ascontiguousarray(points, dtype=np.float64)
    if host.ndim < 2 or host.shape[-1] != 3:
        raise ValueError(f"points must be [..., 3] (3-D only), got {host.shape}")

    def writable(a, shape, name):
        if a is not None and not (isinstance(a, np.ndarray) and a.shape == shape and a.dtype == np.float64
                                  and a.flags.c_contiguous and a.flags.writeable):
            raise ValueError(f"{name} must be a writable C-contiguous f64 array of shape {shape}")

    writable(out, host.shape, "out")
    writable(height_out, host.shape[:-1], "height_out")
    if radius is not None:
        radius = np.ascontiguousarray(radius, dtype=np.float64)
        if radius.shape != host.shape[:-1]:
            raise ValueError(f"radius must have the leading shape of points {host.shape[:-1]}, got {radius.shape}")
    pts = ctx.to_device(host)
    heights = ctx.empty(host.shape[:-1], np.float64) if height_out is not None else None
    res = geographic_points_on_device(ctx, pts, ellipsoid, direction, out=pts, radius=radius, height_out=heights).numpy()
    if height_out is not None:
        height_out[...] = heights.numpy()
    if out is None:
        return res
    out[...] = res
    return out


def to_geographic(points, ellipsoid, radius=None, out=None, height_out=None, context=None):
    """The geographic view of ``points`` f64[..., 3] on the GPU (``mm_geographic_points``, direction 0: Bowring's iteration,
    three passes, every operation rounded on its own): pseudo-points whose geocentric latitude is the geodetic latitude,
    whose longitude is the point's and whose radius is ``6371000 + height`` -- or ``radius`` f64[...], one per point.
    ``height_out`` f64[...] receives the heights above the ellipsoid (m).

    A NumPy array gives a new NumPy array, or fills ``out`` -- a C-contiguous f64 array of the same shape, which may be
    ``points`` itself; ``height_out`` is then a NumPy array too.  A :class:`DeviceArray` or a device tensor gives a device
    array: a new one, or ``out``, which may be ``points`` itself (in place); ``radius`` and ``height_out`` are then device
    arrays that share no byte with ``out``; the call runs on the context's stream and does not synchronise.

    A point on the polar axis takes longitude 0; the centre gives NaN.  Within about 50 km of the centre (inside the
    evolute of the meridian ellipse) the geodetic latitude is not unique and the result is whatever the statement gives."""
    return _apply(points, ellipsoid, TO_GEOGRAPHIC, radius, out, height_out, context)


def from_geographic(points, ellipsoid, out=None, context=None):
    """The way back (``mm_geographic_points``, direction 1): pseudo-points f64[..., 3] -- geocentric latitude = the geodetic
    latitude meant, radius = ``6371000 + height`` -- to the Cartesian points they stand for.  Arrays as
    :func:`to_geographic`.  After :func:`to_geographic` the round trip closes to 1e-8 m at ``|p| >= 200 km``."""
    return _apply(points, ellipsoid, TO_CARTESIAN, None, out, None, context)


def geodetic_coordinates(mesh_or_points, ellipsoid, context=None):
    """``(lat_deg, lon_deg, height_m)`` of a mesh's nodes or of points f64[..., 3], each over the points' leading shape:
    geodetic latitude, longitude in (-180, 180] and height above the ellipsoid.  The kernel runs on the device; the two
    angles are then NumPy's ``arctan2`` of the pseudo-points on the host."""
    ctx = context or default_context()
    pts = _mesh_points(mesh_or_points) if is_mesh(mesh_or_points) else mesh_or_points
    on_device = _is_device(ctx, pts)
    if not on_device:
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        if pts.ndim < 2 or pts.shape[-1] != 3:
            raise ValueError(f"points must be [..., 3] (3-D only), got {pts.shape}")
    src = ctx.asdevice(pts, np.float64)
    heights = ctx.empty(tuple(src.shape[:-1]), np.float64)
    pseudo = geographic_points_on_device(ctx, src, ellipsoid, out=None if on_device else src, height_out=heights).numpy()
    lat = np.rad2deg(np.arctan2(pseudo[..., 2], np.sqrt(pseudo[..., 0] * pseudo[..., 0] + pseudo[..., 1] * pseudo[..., 1])))
    lon = np.rad2deg(np.arctan2(pseudo[..., 1], pseudo[..., 0]))
    return lat, lon, heights.numpy()


# --------------------------------------------------------------------------------------------------------------- meshes
def _model_radius(mesh, context):
    """``z_node_1D * 6371000`` per point of the mesh: the radius :func:`multimesh_amd.api.map_to_sphere` reads, through its
    own helpers (a node layout takes the value of a node's first occurrence in the connectivity).  ``ValueError`` without
    the field, before a device is asked for."""
    pts, z, connectivity = _sphere_layout(mesh)
    if connectivity is not None:
        ctx = context or default_context()
        z = z.reshape(-1)[ctx.first_occurrence(connectivity, pts.shape[0]).numpy()]
    return np.ascontiguousarray(z * R_EARTH).reshape(pts.shape[:-1])


def as_geographic(mesh, ellipsoid=None, depth="ellipsoid", context=None):
    """``mesh`` seen in geographic coordinates: a mesh of the same class (:class:`GllMesh` or :class:`HexMesh`) whose
    points are the pseudo-points of :func:`to_geographic`, computed on the device into a NEW array, and whose field store
    IS the original's -- built exactly like :func:`multimesh_amd.frames.in_frame`.  The caller's coordinates never change.

    Every sampler reads a node's geocentric latitude, longitude and ``6371000 - |p|``; of the view these are the node's
    GEODETIC latitude, its longitude and its depth below the ellipsoid.  So
    ``api.import_regular_grid(grid, geodesy.as_geographic(mesh), ...)`` imports a cube published on geodetic axes, and
    :func:`multimesh_amd.layered.import_layered_model`, :func:`multimesh_amd.harmonics.import_harmonic_model`,
    :func:`multimesh_amd.topography.apply_topography` and the tools of :mod:`multimesh_amd.regions` read it likewise, with
    no change of their own; the fields they write land in ``mesh``.

    ``ellipsoid``: None is :meth:`Ellipsoid.wgs84`.  ``depth``:

    * ``"ellipsoid"``: ``|p'| = 6371000 + height``: depth below the ellipsoid's surface.
    * ``"z_node_1D"``: ``|p'| = z_node_1D * 6371000``, the radius :func:`multimesh_amd.api.map_to_sphere` reads: a node
      keeps the depth of the 1-D model the mesh was stretched from and takes only its direction from the ellipsoid.
      ``ValueError`` when the mesh has no such field.

    The view composes with :func:`multimesh_amd.frames.in_frame`: ``in_frame(as_geographic(mesh), R)`` is the geographic
    view seen from a rotated frame.  A :class:`multimesh_amd.regions.Region` used on the view wants ``geodetic=False``
    vertices: the view's latitudes ARE geodetic already, and ``geodetic=True`` would convert the outline a second time."""
    if not isinstance(mesh, (GllMesh, HexMesh)):
        raise ValueError("as_geographic takes a GllMesh or a HexMesh")
    if depth not in ("ellipsoid", "z_node_1D"):
        raise ValueError(f'depth must be "ellipsoid" or "z_node_1D", got {depth!r}')
    pts = np.asarray(_mesh_points(mesh))
    if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
        raise ValueError(f"as_geographic takes 3-D meshes only (points of shape {pts.shape})")
    radius = _model_radius(mesh, context) if depth == "z_node_1D" else None
    view = copy.copy(mesh)              # (shallow: the same field store, the same connectivity)
    pseudo = to_geographic(np.ascontiguousarray(pts, dtype=np.float64), ellipsoid or Ellipsoid.wgs84(), radius=radius,
                           context=context)
    if isinstance(mesh, GllMesh):
        view.gll_points = pseudo
    else:
        view.points = pseudo
    return view


def geographic_points(lat, lon, depth, ellipsoid, context=None):
    """Cartesian points f64[..., 3] of geodetic rows: ``lat`` and ``lon`` in degrees and ``depth`` in metres below the
    ellipsoid, broadcast against one another.  The pseudo-points are formed on the host with the expressions of
    :func:`multimesh_amd.api.latlondepth_to_xyz` (that function itself); direction 1 then runs on the device."""
    lat, lon, depth = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (lat, lon, depth)))
    rows = np.stack([lat.reshape(-1), lon.reshape(-1), depth.reshape(-1)], axis=1)
    pseudo = np.ascontiguousarray(latlondepth_to_xyz(rows)) if len(rows) else np.zeros((0, 3))
    return from_geographic(pseudo, ellipsoid, context=context).reshape(lat.shape + (3,))


def _axis(values, name):
    a = np.atleast_1d(np.asarray(values, dtype=np.float64))
    if a.ndim != 1 or a.size < 1 or not np.isfinite(a).all():
        raise ValueError(f"the {name} axis must be 1-D, finite and not empty")
    return a


def extract_geographic_grid(mesh, parameters, lat, lon, depth, ellipsoid=None, *, nelem_to_search=25, tolerance=1.05,
                            fill_value=np.nan, chunk_points=None, context=None):
    """A GLL model on a regular grid over GEODETIC axes: ``lat`` and ``lon`` (degrees) and ``depth`` (metres below the
    ellipsoid) are 1-D axes, the result a :class:`multimesh_amd.api.RegularGrid` with dims (depth, latitude, longitude)
    -- the inverse of an import through :func:`as_geographic`.  ``ellipsoid``: None is :meth:`Ellipsoid.wgs84`.

    The grid points come from :func:`geographic_points` and are interpolated by
    :func:`multimesh_amd.api.interpolate_gll_to_points`, in chunks of whole depth levels of at most ``chunk_points`` points
    (None: 4 M; a single level is never split).  Points outside the mesh hold ``fill_value`` and are counted in
    ``nmissing``: the constant field 1 is interpolated beside the parameters and is exactly 0 at a point without an
    element.  ``mesh`` is a :class:`GllMesh`.  ``mm_sample_columns_gll``, which generates geocentric columns on the device
    for :func:`multimesh_amd.api.extract_regular_grid`, is not used: the geographic points are not columns of one table."""
    if not isinstance(mesh, GllMesh):
        raise ValueError("extract_geographic_grid takes a GllMesh")
    parameters = [parameters] if isinstance(parameters, str) else list(parameters)
    missing = [p for p in parameters if p not in mesh.element_nodal_fields]
    if missing:
        raise ValueError(f"the mesh has no field {missing}")
    lat, lon, depth = _axis(lat, "latitude"), _axis(lon, "longitude"), _axis(depth, "depth")
    per_level = len(lat) * len(lon)
    budget = CHUNK_POINTS if chunk_points is None else int(chunk_points)
    if budget < 1:
        raise ValueError("chunk_points must be >= 1 (or None)")
    levels = max(1, budget // per_level)
    ellipsoid = ellipsoid or Ellipsoid.wgs84()
    found = "__found__"
    while found in mesh.element_nodal_fields:
        found += "_"
    fields = {p: mesh.element_nodal_fields[p] for p in parameters}
    fields[found] = np.ones(mesh.gll_points.shape[:2])
    probe = GllMesh(mesh.gll_points, mesh.shape_order, fields)
    values = np.empty((len(parameters), len(depth), len(lat), len(lon)))
    nmissing = 0
    for start in range(0, len(depth), levels):
        stop = min(start + levels, len(depth))
        pts = geographic_points(lat[None, :, None], lon[None, None, :], depth[start:stop, None, None], ellipsoid, context=context)
        vals = interpolate_gll_to_points(probe, pts.reshape(-1, 3), parameters + [found], nelem_to_search=nelem_to_search,
                                         tolerance=tolerance, context=context)
        outside = vals[:, -1] == 0.0
        nmissing += int(outside.sum())
        vals[outside, :-1] = fill_value
        values[:, start:stop] = vals[:, :-1].T.reshape(len(parameters), stop - start, len(lat), len(lon))
    return RegularGrid(depth, lat, lon, {p: values[c] for c, p in enumerate(parameters)}, nmissing, fill_value)
