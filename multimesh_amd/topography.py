"""Topography: the nodes of a mesh stretched radially between anchor radii by a latitude x longitude map of interface
positions -- surface elevation, Moho, any honoured discontinuity -- and the flattening that undoes it and returns every node's
1-D reference radius, on the GPU (include/multimesh_topography.h: ``mm_radial_stretch``; the header holds the statement,
operation by operation, which the device reproduces bit for bit).  Imported explicitly
(``from multimesh_amd import topography``); the reference has no counterpart beyond ``map_to_ellipse``.

What it is for.  :func:`multimesh_amd.layered.import_layered_model` lays a crust with a Moho map over a mesh whose element
faces stay at the 1-D Moho radius: :func:`apply_topography` with :meth:`InterfaceMap.from_layered` moves the faces onto the
map first.  :func:`multimesh_amd.api.radial_profile` and ``evaluate_radial_model`` want a mesh on its 1-D sphere, and
:func:`multimesh_amd.api.map_to_sphere` wants ``z_node_1D``: :func:`attach_z_node_1d` computes that field for a mesh that
arrives with its topography applied and the field missing.  Geometry is ``mm_sample_grid``'s: ``z`` is the pole, latitude is
geocentric, longitude runs from ``x`` towards ``y``.  No analytic ellipticity, no repair of element quality after large shifts
(:func:`multimesh_amd.resolution.check_model` reports the result), no Exodus coordinate writer
(:class:`multimesh_amd.io.Exodus` has none, as :mod:`multimesh_amd.frames` notes).

The symbol is an extension of the library's C ABI with a header of its own: this module keeps its signature table and
applies it to the handle of :func:`multimesh_amd.helpers.load_lib` on first use; the call itself goes through
:func:`multimesh_amd.device._call` and the :class:`Context` checks like every other call of the package."""
from __future__ import annotations

import contextlib

import numpy as np

from . import device as _device
from . import io as mio
from .api._common import R_EARTH, GllMesh, ImportTarget, _mesh_points, is_mesh
from .api.earth import _set_points, _z_node_1d
from .api.grids import RegularGrid, prepare_regular_grid
from .device import default_context
from .helpers import i32, i64, load_lib, vp
from .mesh import HexMesh

__all__ = ["InterfaceMap", "radial_stretch", "stretch_points", "apply_topography", "remove_topography", "reference_radius",
           "attach_z_node_1d", "DIRECTION", "LATERAL", "OUTSIDE"]

MAX_NA = 64     # MM_STRETCH_MAX_NA
#: names -> their numbers in the C ABI (MM_STRETCH_DIRECTION_*, _LATERAL_*, _OUTSIDE_*)
DIRECTION = {"apply": 0, "flatten": 1}
LATERAL = {"cell": 0, "bilinear": 1}
OUTSIDE = {"keep": 0, "clamp": 1}

#: name -> (restype, argtypes) of the function include/multimesh_topography.h declares (tests/test_topography.py compares it
#: with the header); it is not part of helpers.SIGNATURES, the table of include/multimesh_hip.h
SIGNATURES = {
    "mm_radial_stretch": (i32, (vp, vp, i64, vp, vp, i32, vp, i32, i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp)),
}


def bind(lib=None):
    """The library handle with :data:`SIGNATURES` applied (once)."""
    lib = lib or load_lib()
    if getattr(lib, "_topography_bound", False) is not True:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        lib._topography_bound = True
    return lib


def _number(table, key, what):
    if key not in table:
        raise ValueError(f"{what} must be one of {list(table)}, got {key!r}")
    return table[key]


_SHIFTS = "\0shifts"     # the name the shifts travel under through prepare_regular_grid


class InterfaceMap:
    """Where a stack of interfaces lies on a latitude x longitude map, as shifts of their 1-D reference radii.

    ``lat`` f64[nlat], ``lon`` f64[nlon]: degrees, finite and strictly monotone (either way).  ``anchors`` f64[na]: the
    reference radii ``A_0 > A_1 > ...`` in metres, top first, finite and strictly descending, ``2 <= na <= 64``.  ``shifts``
    f64[na, nlat, nlon]: the radial displacement of every anchor at every map node in metres, positive up, finite.  At every
    map node the deformed anchors ``B_j = A_j + shifts[j]`` must descend strictly -- interfaces that cross are refused, and
    the error names the worst column --, which makes the stretching invertible.  ``lon_periodic``: None detects a global
    longitude axis as :func:`multimesh_amd.api.prepare_regular_grid` does.

    The axes are prepared by that function -- descending axes are flipped with their data, a global longitude axis is
    closed by the column ``lon[0] + 360`` -- so this is stated once; ``lat``, ``lon`` and ``shifts`` hold the prepared map,
    ``flipped`` (axis name -> bool), ``appended`` (whether a closing column was added) and ``periodic`` what was done.
    ``ValueError`` for what is refused.

    Between two anchors a node moves by the linear blend of their shifts, above the top anchor by the top shift (rigidly),
    below the bottom anchor by the bottom shift: end the stack with an anchor of zero shift (``taper_radius`` of the
    constructors) and everything below it stays where it is."""

    def __init__(self, lat, lon, anchors, shifts, lon_periodic=None):
        anchors = np.array(anchors, dtype=np.float64)
        if anchors.ndim != 1 or not 2 <= anchors.size <= MAX_NA:
            raise ValueError(f"anchors must be f64[na] with 2 <= na <= {MAX_NA}, got {anchors.shape}")
        if not np.isfinite(anchors).all() or not (np.diff(anchors) < 0).all():
            raise ValueError("the anchors must be finite and strictly descending (radii, top first)")
        shifts = np.asarray(shifts, dtype=np.float64)
        if shifts.shape != (anchors.size, np.size(lat), np.size(lon)):
            raise ValueError(f"shifts must be {(anchors.size, np.size(lat), np.size(lon))} ([anchor][lat][lon]), got {shifts.shape}")
        if not np.isfinite(shifts).all():
            raise ValueError("the shifts must be finite")
        lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        gap = np.diff(anchors[:, None, None] + shifts, axis=0)                # B_{j+1} - B_j: negative where all is well
        if (gap >= 0).any():
            j, ja, io = np.unravel_index(np.argmax(gap), gap.shape)
            raise ValueError(f"interfaces cross: at lat {lat[ja]:g}, lon {lon[io]:g} interface {j + 1} lies {gap[j, ja, io]:g} m "
                             f"above interface {j} (every deformed anchor must lie below the one above it)")
        grid = RegularGrid(np.arange(anchors.size, dtype=np.float64), lat, lon, {_SHIFTS: shifts})
        _, self.lat, self.lon, data, _, self.periodic = prepare_regular_grid(grid, lon_periodic=lon_periodic)
        self.flipped = {"latitude": bool(lat.size > 1 and lat[0] > lat[-1]), "longitude": bool(lon.size > 1 and lon[0] > lon[-1])}
        self.appended = data.shape[-1] != lon.size
        self.anchors = anchors
        self.shifts = np.ascontiguousarray(data[0])

    @classmethod
    def from_surface(cls, lat, lon, elevation, taper_radius=6_071_000.0, lon_periodic=None):
        """Surface topography: ``elevation`` f64[nlat, nlon] in metres above 6 371 000 m.  Anchors ``[6371000, taper_radius]``,
        shifts ``[elevation, 0]``: the surface follows the map, the displacement fades linearly to nothing at
        ``taper_radius`` (default: 300 km down) and everything below stays."""
        elevation = np.asarray(elevation, dtype=np.float64)
        return cls(lat, lon, [R_EARTH, taper_radius], np.stack([elevation, np.zeros_like(elevation)]), lon_periodic)

    @classmethod
    def from_radii(cls, lat, lon, anchors, radii, lon_periodic=None):
        """From the actual radius of every interface: ``radii`` f64[na, nlat, nlon]; ``shifts[j] = radii[j] - anchors[j]``."""
        anchors, radii = np.asarray(anchors, dtype=np.float64), np.asarray(radii, dtype=np.float64)
        if anchors.ndim != 1 or radii.ndim != 3 or radii.shape[0] != anchors.size:
            raise ValueError(f"radii must be [na, nlat, nlon] over anchors [na], got {radii.shape} over {anchors.shape}")
        return cls(lat, lon, anchors, radii - anchors[:, None, None], lon_periodic)

    @classmethod
    def from_layered(cls, model, interfaces, taper_radius=None):
        """From the interfaces of a :class:`multimesh_amd.layered.LayeredModel`.  ``interfaces``: interface index of the model
        -> its depth in the mesh's 1-D model, in metres below 6 371 000 m, e.g. ``{0: 0.0, 3: 24400.0}`` for the surface and a
        Moho the mesh honours at 24.4 km.  The anchor is ``6371000 - depth`` and its shift
        ``(6371000 - bounds[i]) - (6371000 - depth)``.  ``taper_radius``: a bottom anchor of zero shift is appended."""
        items = sorted(((float(depth), int(i)) for i, depth in dict(interfaces).items()))
        if not items or any(not 0 <= i < model.nb for _, i in items):
            raise ValueError(f"interfaces must map interface indices in [0, {model.nb}) to their 1-D depths, got {interfaces}")
        anchors = [R_EARTH - depth for depth, _ in items]
        shifts = [(R_EARTH - model.bounds[i]) - (R_EARTH - depth) for depth, i in items]
        if taper_radius is not None:
            anchors.append(float(taper_radius))
            shifts.append(np.zeros_like(shifts[0]))
        return cls(model.lat, model.lon, anchors, np.stack(shifts), lon_periodic=model.periodic)

    @property
    def na(self):
        return self.anchors.size

    def packed(self):
        """shifts f64[nlat, nlon, na]: the column-major table the device reads -- the column of a map node is one run."""
        return np.ascontiguousarray(self.shifts.transpose(1, 2, 0))

    def on_device(self, ctx):
        """The map resident on ``ctx``: what :func:`stretch_points` takes in place of the map itself, to upload it once."""
        return _ResidentMap(ctx.to_device(self.lat), ctx.to_device(self.lon), ctx.to_device(self.anchors),
                            ctx.to_device(self.packed()), self.periodic)


class _ResidentMap:
    def __init__(self, lat, lon, anchors, shifts, periodic):
        self.lat, self.lon, self.anchors, self.shifts, self.periodic = lat, lon, anchors, shifts, periodic


# ------------------------------------------------------------------------------------------------------------- the call
def radial_stretch(ctx, points, lat, lon, anchors, shifts, lon_periodic=False, direction="apply", ref_radius=None,
                   lateral="bilinear", outside="keep", out=None, want_points=True, want_radius=False, want_latlondepth=False,
                   noutside=None):
    """``mm_radial_stretch`` on the context ``ctx``: ``points`` f64[..., 3]; ``lat`` f64[nlat], ``lon`` f64[nlon] strictly
    ascending (a periodic ``lon`` closed at ``lon[0] + 360``: host axes are checked as :meth:`Context.sample_grid` checks
    them, device axes are the caller's word); ``anchors`` f64[na] and ``shifts`` f64[nlat, nlon, na], the column-major table of
    :meth:`InterfaceMap.packed`, both the caller's word.  ``direction`` "apply" or "flatten", ``lateral`` "bilinear" or "cell",
    ``outside`` "keep" or "clamp": include/multimesh_topography.h states each.  ``ref_radius``: f64 of the points' leading
    shape, with "apply" only.  ``out``: a device array of as many values as ``points``, which may be ``points`` itself (in
    place), or None: a new one (``want_points=False``: the points are not written).  ``noutside``: int64[1] on the device,
    added to (not zeroed), or None.  Every array may be a host array, a :class:`DeviceArray` or a torch-like tensor on the
    GPU.  Returns a dict of device arrays: "points" f64[..., 3] and, as asked for, "radius" f64[...] and "latlondepth"
    f64[..., 3].  Runs on the context's stream and does not synchronise.  ``ValueError`` with the library's message for what
    it refuses.

    Copies of a shared node that hold the same bits get the same bits: a node's result depends on its own coordinates (and
    its own ``ref_radius``) alone, by one fixed sequence of operations."""
    ndirection, nlateral, noutmode = (_number(DIRECTION, direction, "direction"), _number(LATERAL, lateral, "lateral"),
                                      _number(OUTSIDE, outside, "outside"))
    lib = bind(ctx.lib)
    pts, n = ctx._points3(points)
    _, la, lo = ctx._grid_axes(np.zeros(1), lat, lon, lon_periodic)
    a = ctx.asdevice(anchors, np.float64)
    if len(a.shape) != 1 or not 2 <= a.shape[0] <= MAX_NA:
        raise ValueError(f"anchors must be f64[na] with 2 <= na <= {MAX_NA}, got {a.shape}")
    s = ctx.asdevice(shifts, np.float64)
    if s.shape != (la.shape[0], lo.shape[0], a.shape[0]):
        raise ValueError(f"shifts must be [{la.shape[0]}, {lo.shape[0]}, {a.shape[0]}] over the axes and the anchors, got {s.shape}")
    lead = pts.shape[:-1]
    ref = None
    if ref_radius is not None:
        if direction != "apply":
            raise ValueError('ref_radius goes with direction="apply": flattening computes it')
        ref = ctx.asdevice(ref_radius, np.float64)
        if ref.size != n:
            raise ValueError("ref_radius needs one value per point")
    if noutside is not None:
        noutside = ctx.asdevice(noutside, np.int64)
        if noutside.size != 1:
            raise ValueError("noutside must be int64[1]")
    if out is not None or want_points:
        out = ctx._out(out, pts.shape, "out must hold as many values as points", size_only=True)
    res = {"points": out, "radius": ctx._wanted(want_radius, lead), "latlondepth": ctx._wanted(want_latlondepth, lead + (3,))}
    _device._call(lib, "mm_radial_stretch", ctx.handle, pts, n, ref, la, la.shape[0], lo, lo.shape[0], int(bool(lon_periodic)),
                  a, a.shape[0], s, ndirection, nlateral, noutmode, res["points"], res["radius"], res["latlondepth"], noutside,
                  arg_error=True)
    return {k: v for k, v in res.items() if v is not None}


def stretch_points(ctx, points, imap, direction="apply", ref_radius=None, lateral="bilinear", outside="keep", out=None,
                   want_radius=False, want_latlondepth=False, noutside=None, want_points=True):
    """:func:`radial_stretch` with an :class:`InterfaceMap` (uploaded for the call) or what its ``on_device(ctx)`` returned
    (resident): the call for resident or host points.  Returns the dict of device arrays of :func:`radial_stretch`."""
    shifts = imap.packed() if isinstance(imap, InterfaceMap) else imap.shifts
    return radial_stretch(ctx, points, imap.lat, imap.lon, imap.anchors, shifts, lon_periodic=imap.periodic, direction=direction,
                          ref_radius=ref_radius, lateral=lateral, outside=outside, out=out, want_points=want_points,
                          want_radius=want_radius, want_latlondepth=want_latlondepth, noutside=noutside)


# --------------------------------------------------------------------------------------------------------------- meshes
class _Geometry:
    """The points of a mesh, open for the length of a ``with`` block: a :class:`GllMesh`, a :class:`HexMesh` or a Salvus mesh
    object (``points``), read and written as :func:`multimesh_amd.frames.rotate_mesh` does, or a writable Salvus file -- an
    h5py-like object (:class:`multimesh_amd.io.MemoryH5`) or, with h5py, a path --, whose ``MODEL/coordinates`` are assigned."""

    def __init__(self, mesh, who):
        self.mesh, self.who = mesh, who

    def __enter__(self):
        with contextlib.ExitStack() as stack:
            self._coordinates = None
            if is_mesh(self.mesh):
                pts = np.asarray(_mesh_points(self.mesh))
            else:
                self._coordinates = stack.enter_context(mio.open_h5(self.mesh, "r+"))["MODEL/coordinates"]
                pts = np.array(self._coordinates[()])
            if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
                raise ValueError(f"{self.who} moves 3-D meshes only (points of shape {pts.shape})")
            self.points = np.ascontiguousarray(pts, dtype=np.float64)
            self._close = stack.pop_all().close
        return self

    def __exit__(self, *exc):
        self._close()

    def write(self, moved):
        if self._coordinates is None:
            _set_points(self.mesh, moved)
        else:
            self._coordinates[...] = moved


def _reference_of(mesh, pts, reference):
    if reference == "radius":
        return None
    if reference != "z_node_1D":
        raise ValueError(f'reference must be "z_node_1D" or "radius", got {reference!r}')
    if not is_mesh(mesh):
        with ImportTarget(mesh) as target:
            target.require(["z_node_1D"])
            z = target.existing(["z_node_1D"])[0]
    else:
        z = _z_node_1d(mesh)
    if z.shape != pts.shape[:-1]:
        raise ValueError(f"z_node_1D of shape {z.shape} does not fit the points {pts.shape}: one value per point is needed")
    return z * R_EARTH


def _move(mesh, imap, direction, ref, lateral, outside, context, who, reference="radius"):
    _number(LATERAL, lateral, "lateral"), _number(OUTSIDE, outside, "outside")
    with _Geometry(mesh, who) as geometry:
        pts = geometry.points
        if ref is None:
            ref = _reference_of(mesh, pts, reference)
        ctx = context or default_context()
        count = ctx.zeros((1,), np.int64)
        dev = ctx.to_device(pts)
        stretch_points(ctx, dev, imap, direction=direction, ref_radius=ref, lateral=lateral, outside=outside, out=dev, noutside=count)
        geometry.write(dev.numpy().reshape(pts.shape))
        return int(count.numpy()[0])


def apply_topography(mesh, imap, reference="z_node_1D", lateral="bilinear", outside="keep", context=None):
    """Stretches the points of ``mesh`` onto the interfaces of ``imap``, IN PLACE, on the GPU.  ``mesh``: a :class:`GllMesh`,
    a :class:`HexMesh` or a Salvus mesh object (``points``), read and written as :func:`multimesh_amd.frames.rotate_mesh`
    does, or a writable Salvus file (an h5py-like object or a path: ``MODEL/coordinates``).  ``reference``: "z_node_1D" takes
    every node's reference radius from the mesh's field, ``z_node_1D * 6371000`` as :func:`multimesh_amd.api.map_to_sphere`
    reads it (one value per point), and moves the node to the stretched image of THAT radius along its own direction;
    "radius" takes the node's own radius -- right for a mesh that is on its 1-D sphere.  ``lateral`` "bilinear" or "cell",
    ``outside`` "keep" (nodes off the map stay where they are) or "clamp" (the map's edge extends).  The fields of the mesh
    are untouched.  Copies of a shared node that hold the same bits (and the same ``z_node_1D``) get the same bits.  Returns
    the number of nodes outside the map."""
    return _move(mesh, imap, "apply", None, lateral, outside, context, "apply_topography", reference)


def remove_topography(mesh, imap, lateral="bilinear", outside="keep", context=None):
    """The flattening, IN PLACE: every node of ``mesh`` goes back to its 1-D reference radius along its own direction -- the
    inverse of :func:`apply_topography` with ``reference="radius"``, exact to a few roundings times the largest ratio of an
    undeformed to a deformed layer thickness.  That holds for ``lateral="bilinear"``, where the map is continuous; with "cell"
    it is piecewise constant, and a node within rounding of the border between the cells of two map nodes may read the other
    column on the way back.  Arguments and return value as :func:`apply_topography`."""
    return _move(mesh, imap, "flatten", None, lateral, outside, context, "remove_topography")


def reference_radius(mesh_or_points, imap, lateral="bilinear", outside="keep", context=None):
    """The 1-D reference radius ``rho`` of every node of a mesh (or of points f64[..., 3]) that carries the topography of
    ``imap``: host f64 in the leading shape of the points.  Nothing is moved.  Nodes outside the map get their own radius."""
    _number(LATERAL, lateral, "lateral"), _number(OUTSIDE, outside, "outside")
    if is_mesh(mesh_or_points) or isinstance(mesh_or_points, np.ndarray) or isinstance(mesh_or_points, (list, tuple)):
        pts = np.ascontiguousarray(_mesh_points(mesh_or_points) if is_mesh(mesh_or_points) else mesh_or_points, dtype=np.float64)
        if pts.ndim < 2 or pts.shape[-1] != 3:
            raise ValueError(f"reference_radius needs 3-D points [..., 3], got {pts.shape}")
        return _radius_of(pts, imap, lateral, outside, context)
    with _Geometry(mesh_or_points, "reference_radius") as geometry:
        return _radius_of(geometry.points, imap, lateral, outside, context)


def _radius_of(pts, imap, lateral, outside, context):
    ctx = context or default_context()
    res = stretch_points(ctx, pts, imap, direction="flatten", lateral=lateral, outside=outside, want_points=False, want_radius=True)
    return res["radius"].numpy().reshape(pts.shape[:-1])


def attach_z_node_1d(mesh, imap, lateral="bilinear", outside="keep", context=None):
    """Stores ``reference_radius / 6371000`` as the ``z_node_1D`` field of ``mesh`` -- ``element_nodal_fields`` of a
    :class:`GllMesh` or a Salvus mesh object, a nodal field of a :class:`HexMesh`, the ``z_node_1D`` column of a Salvus
    file's ``MODEL/data`` (which must exist) --, so that :func:`multimesh_amd.api.map_to_sphere`, and with it the advice of
    :func:`multimesh_amd.api.radial_profile`, works on a mesh that came with its topography applied and without the field.
    Returns the mesh."""
    z = reference_radius(mesh, imap, lateral=lateral, outside=outside, context=context) / R_EARTH
    if isinstance(mesh, (GllMesh, HexMesh)) or not is_mesh(mesh):
        with ImportTarget(mesh) as target:
            target.require(["z_node_1D"])
            target.write(["z_node_1D"], z[None])
    else:
        fields = getattr(mesh, "element_nodal_fields", None)
        if fields is None or z.ndim != 2:
            raise ValueError("the mesh has no element_nodal_fields to hold an element-nodal z_node_1D")
        fields["z_node_1D"] = np.ascontiguousarray(z)
    return mesh
