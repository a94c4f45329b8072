"""The boundary of a mesh as a SURFACE: its faces as triangles through their GLL nodes, the exact distance of every node or
point to them -- with a cutoff of any size or with none --, the depth of a mesh's nodes below its own free surface, and the
taper and blend of :mod:`multimesh_amd.boundary` driven by that distance, on the GPU (include/multimesh_surface.h:
``mm_boundary_triangles``, ``mm_surface_distance``; the header holds the statements, which the device reproduces bit for
bit).  Imported explicitly (``from multimesh_amd import surface``); the reference has no counterpart.

:mod:`multimesh_amd.boundary` measures the distance to the nearest boundary NODE, whose resolution is the node spacing and
whose cost grows with the cube of the cutoff; here the distance is to the faces between the nodes -- the piecewise-linear
surface through them: 2 order^2 flat facets per face -- and the cost follows the distance found, not the cutoff.

The two symbols are an extension of the library's C ABI with a header of their own: this module keeps their signature
table and applies it to the handle of :func:`multimesh_amd.helpers.load_lib` on first use; the calls themselves go through
:func:`multimesh_amd.device._call` like every other call of the package.  3-D meshes only."""
from __future__ import annotations

import numpy as np

from . import boundary as _boundary
from . import device as _device
from .api._common import is_mesh, points_of
from .boundary import mesh_boundary
from .device import default_context
from .helpers import f64, i32, i64, load_lib, vp

__all__ = ["boundary_triangles", "distance_to_triangles", "distance_to_surface", "depth_below_surface", "taper_to_surface",
           "blend_models"]

#: name -> (restype, argtypes) of the functions include/multimesh_surface.h declares (tests/test_surface.py compares it
#: with the header); they are not part of helpers.SIGNATURES, the table of include/multimesh_hip.h
SIGNATURES = {
    "mm_boundary_triangles": (i64, (vp, vp, i64, i32, vp, vp, i64, i32, vp)),
    "mm_surface_distance": (i64, (vp, vp, i64, vp, i64, f64, vp)),
}


def bind(lib=None):
    """The library handle with :data:`SIGNATURES` applied (once)."""
    lib = lib or load_lib()
    if getattr(lib, "_surface_bound", False) is not True:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        lib._surface_bound = True
    return lib


def _cutoff(cutoff):
    """``None`` is no cutoff, +inf to the library."""
    cutoff = np.inf if cutoff is None else float(cutoff)
    if not cutoff > 0.0:
        raise ValueError("cutoff must be positive (None or inf: unbounded)")
    return cutoff


def _triangles(boundary, mask):
    """The triangles of the faces whose side is in ``mask``, f64[T, 3, 3] on the boundary's own context."""
    ctx, order = boundary._ctx, boundary._order
    nb = boundary._faces.shape[0]
    out = ctx.empty((nb * 2 * order * order, 3, 3), np.float64)
    T = _device._call(bind(ctx.lib), "mm_boundary_triangles", ctx.handle, boundary._points, boundary._points.shape[0], order,
                      boundary._faces, boundary._side, nb, int(mask), out, arg_error=True)
    return out.rows(0, int(T))


def boundary_triangles(boundary, sides=("side", "bottom")):
    """The faces of ``sides`` of a :class:`multimesh_amd.boundary.Boundary` as triangles through their nodes: a device array
    f64[T, 3, 3] (triangle, vertex, coordinate) on the boundary's own context, 2 order^2 per face, face by face: each
    sub-quad of a face's node grid ``q[j][i]`` gives ``(q[j][i], q[j][i+1], q[j+1][i+1])`` and ``(q[j][i], q[j+1][i+1],
    q[j+1][i])``.  The surface is the piecewise-linear one through the nodes (order 1: the corner quad split along a diagonal;
    a curved order-4 face: 32 flat facets).  The default leaves the free surface ("top") out."""
    return _triangles(_boundary._boundary_of(boundary), _boundary._side_mask(sides))


def _distance(ctx, points, triangles, cutoff):
    """(distance on the device over the points' leading shape, the number below the cutoff)"""
    pts, n = ctx._points3(points)
    tri = ctx.asdevice(triangles, np.float64)
    if len(tri.shape) != 3 or tri.shape[1:] != (3, 3):
        raise ValueError("triangles must be [T, 3, 3]")
    dist = ctx.empty(pts.shape[:-1], np.float64)
    count = _device._call(bind(ctx.lib), "mm_surface_distance", ctx.handle, pts, n, tri, tri.shape[0], cutoff, dist,
                          arg_error=True)
    return dist, int(count)


def distance_to_triangles(points, triangles, cutoff=None, context=None):
    """The distance of points f64[..., 3] to the nearest point of any of ``triangles`` f64[T, 3, 3], or ``cutoff`` where
    none lies within it (``None``: unbounded, +inf without triangles): ``(distance f64[...] on the device, the number of
    points below the cutoff)``, bit for bit the brute-force minimum over every triangle of the header's closest-point walk.
    Both arrays may be host arrays, :class:`DeviceArray` objects or torch-like tensors on the GPU.  A point with a
    coordinate that is not finite keeps the cutoff; a triangle with one raises ``ValueError``."""
    return _distance(context or default_context(), points, triangles, _cutoff(cutoff))


def _surface_distance(ctx, bnd, points, mask, cutoff):
    """The distance step of this module, as :func:`multimesh_amd.boundary._blend` calls it."""
    return _distance(ctx, points, _triangles(bnd, mask), max(cutoff, _boundary._MIN_CUTOFF))[0]


def distance_to_surface(mesh_or_points, boundary, cutoff=None, sides=("side", "bottom"), context=None):
    """The distance of every node of a mesh (f64[E, P]; a :class:`HexMesh`: f64[N]) or of points f64[..., 3] to the faces of
    ``sides`` of ``boundary`` -- to the triangles of :func:`boundary_triangles`, not to their nodes --, or ``cutoff`` where
    the surface is farther (``None``: unbounded).  A node of those faces gets exactly 0.0.  The call runs on the boundary's own
    context: ``context`` is that one or ``None`` (``ValueError`` otherwise)."""
    bnd = _boundary._boundary_of(boundary)
    cutoff, mask = _cutoff(cutoff), _boundary._side_mask(sides)
    pts = points_of(mesh_or_points) if is_mesh(mesh_or_points) else mesh_or_points
    ctx = bnd._context(context)
    return _distance(ctx, pts, _triangles(bnd, mask), cutoff)[0].numpy()


def depth_below_surface(mesh, boundary=None, context=None):
    """The depth of every node of ``mesh`` below the mesh's own free surface: its unbounded distance to the "top" faces
    (f64[E, P]; a :class:`HexMesh`: f64[N]), whatever that surface is -- topography and ellipticity included, where
    ``6371000 - |p|`` is wrong by kilometres.  ``boundary``: what :func:`mesh_boundary` returned for this mesh (``None``:
    computed here, with radial up)."""
    if boundary is None:
        boundary = mesh_boundary(mesh, context=context)
    return distance_to_surface(mesh, boundary, None, sides=("top",), context=context)


def taper_to_surface(mesh, params, inner, outer, sides=("side", "bottom"), boundary=None, context=None):
    """:func:`multimesh_amd.boundary.taper_to_boundary` with the distance to the faces: ``(values, ntapered)``, the fields
    ``params`` times 0 within ``inner`` of the surface of ``sides``, 1 beyond ``outer``, the smoothstep between
    (``mm_distance_taper``).  Every point of a face gets weight 0, not only its nodes; nodes beyond ``outer`` keep their
    bits."""
    return _boundary._taper(_surface_distance, mesh, params, inner, outer, sides, boundary, context)


def blend_models(regional, host, params, inner, outer, sides=("side", "bottom"), nelem_to_search=20, tolerance=1.05,
                 context=None):
    """:func:`multimesh_amd.boundary.blend_models` with the distance to ``regional``'s boundary faces themselves: the blend
    follows the region's outline, not the pattern of the nodes on it.  Same arguments, same ``(values, info)``."""
    return _boundary._blend(_surface_distance, regional, host, params, inner, outer, sides, nelem_to_search, tolerance,
                            context)
