"""Where a mesh ends, and what to do near there: the boundary faces of a hexahedral mesh, told apart as free surface, bottom
and artificial side; the distance of every node to the nearest boundary node up to a cutoff; a taper of fields towards the
boundary and the blend of a regional model into a larger one -- on the GPU, on arrays that need not leave HBM
(include/multimesh_hip.h: mm_boundary_faces, mm_boundary_classify, mm_boundary_nodes, mm_cutoff_distance,
mm_distance_taper).  Imported explicitly (``from multimesh_amd import boundary``); the reference has no counterpart.

The distance is to the nearest boundary NODE, not to the boundary surface: its resolution is the node spacing of the faces
(:mod:`multimesh_amd.surface` has the distance to the faces themselves, with the same tools on top of it).
3-D meshes only."""
from __future__ import annotations

import warnings

import numpy as np

from .api._common import EXODUS_TO_TENSOR  # noqa: F401  (stated there; still reachable here, where it used to live)
from .api._common import _gll_points_order, _mesh_fields, _scatter_back, hex8_corners, named_fields, points_of
from .device import default_context
from .mesh import HexMesh

__all__ = ["mesh_boundary", "distance_to_boundary", "taper_to_boundary", "blend_models"]

#: the side of a boundary face as mm_boundary_classify numbers it
SIDES = {"side": 0, "top": 1, "bottom": 2}
_MIN_CUTOFF = 2.0 ** -500   # the least cutoff mm_cutoff_distance serves


def corner_nodes(order):
    """The node of every tensor corner ``c = i + 2 j + 4 k`` of a GLL element: ``p = n i + m n j + m m n k``, m = n + 1."""
    n, m = int(order), int(order) + 1
    return np.array([n * (c & 1) + m * n * ((c >> 1) & 1) + m * m * n * (c >> 2) for c in range(8)], dtype=np.int64)


def _side_mask(sides):
    if isinstance(sides, str):
        sides = (sides,)
    unknown = [s for s in sides if s not in SIDES]
    if unknown:
        raise ValueError(f'sides are named "side", "top", "bottom", got {unknown}')
    return sum({1 << SIDES[s] for s in sides})


class Boundary:
    """The boundary faces of a mesh, from :func:`mesh_boundary`: ``element`` and ``face`` int64[nb] (local face 0 .. 5 =
    i=0, i=1, j=0, j=1, k=0, k=1 of the element), ``side`` int32[nb] (0 lateral side, 1 top, 2 bottom), all in ascending
    order of ``6 * element + face``; ``nonmanifold``: the number of faces shared by more than two elements (counted as
    interior).  The mesh's nodes and the faces stay on the device for :meth:`nodes`."""

    def __init__(self, ctx, points_d, order, faces_d, side_d, nonmanifold):
        self._ctx, self._points, self._order, self._faces, self._side = ctx, points_d, order, faces_d, side_d
        codes = faces_d.numpy()
        self.element, self.face = codes // 6, codes % 6
        self.side = side_d.numpy()
        self.nonmanifold = int(nonmanifold)

    def __len__(self):
        return len(self.element)

    def count(self, side):
        """The number of boundary faces of ``side`` ("side", "top" or "bottom")."""
        if side not in SIDES:
            raise ValueError('side must be "side", "top" or "bottom"')
        return int((self.side == SIDES[side]).sum())

    def _nodes(self, mask):
        """The nodes of the faces whose side is in ``mask``, f64[K, 3] on the boundary's own context."""
        return self._ctx.boundary_nodes(self._points, self._order, self._faces, self._side, mask)

    def _context(self, context):
        """The boundary's context; the faces and nodes live there, so another one is refused."""
        if context is not None and context is not self._ctx:
            raise ValueError("the boundary lives on another context: pass the one mesh_boundary was given, or None")
        return self._ctx

    def nodes(self, sides=("side", "bottom")):
        """The nodes f64[K, 3] of the faces of ``sides``, face by face, (order+1)^2 per face (a node shared by two faces
        appears twice).  The default leaves the free surface ("top") out."""
        return self._nodes(_side_mask(sides)).numpy()


def mesh_boundary(mesh, up=None, cos_min=0.5, context=None):
    """The :class:`Boundary` of a :class:`GllMesh`, a Salvus mesh (orders 1, 2, 4) or a :class:`HexMesh`: the faces that
    belong to one element only, each classified by its outward normal against ``up`` -- ``None``: radial, for
    Earth-centred coordinates; else a vector such as ``(0, 0, 1)`` -- as top (cosine >= ``cos_min``), bottom
    (<= ``-cos_min``) or lateral side.  GLL elements are joined where their corner nodes have identical coordinates
    (``unique_points``, as the assembly of ``assemble_gll`` does); a :class:`HexMesh` by its connectivity.  Warns when a face
    is shared by more than two elements."""
    if not 0.0 < float(cos_min) <= 1.0:
        raise ValueError("cos_min must lie in (0, 1]")
    if up is not None:
        up = np.asarray(up, dtype=np.float64)
        if up.shape != (3,) or not np.isfinite(up).all() or not up.any():
            raise ValueError("up must be three finite numbers, not all zero (None: radial)")
    hex8 = isinstance(mesh, HexMesh)
    if hex8:
        conn, corners = hex8_corners(mesh)
    else:
        gp, order = _gll_points_order(mesh)
        if gp.shape[2] != 3:
            raise ValueError("3-D meshes only")
        if order not in (1, 2, 4) or gp.shape[1] != (order + 1) ** 3:
            raise ValueError("GLL orders 1, 2 and 4 only")
    ctx = context or default_context()
    if hex8:
        points = corners = ctx.to_device(corners)
        ids, nnodes, order = ctx.to_device(conn), mesh.npoint, 1
    else:
        points = ctx.to_device(gp)
        corners = points if order == 1 else ctx.to_device(gp[:, corner_nodes(order)])
        uniq, inv = ctx.unique_points(corners.reshape(gp.shape[0] * 8, 3), ordered=False)
        ids, nnodes = inv.reshape(gp.shape[0], 8), uniq.shape[0]
    faces, nonmanifold = ctx.boundary_faces(ids, nnodes)
    if nonmanifold:
        warnings.warn(f"{nonmanifold} faces are shared by more than two elements: the mesh is not a manifold; they are "
                      "counted as interior", stacklevel=2)
    side = ctx.boundary_classify(corners, faces, up=up, cos_min=cos_min)
    return Boundary(ctx, points, order, faces, side, nonmanifold)


def _cutoff(cutoff):
    cutoff = float(cutoff)
    if not (np.isfinite(cutoff) and cutoff > 0.0):
        raise ValueError("cutoff must be positive and finite")
    return cutoff


def distance_to_boundary(mesh_or_points, boundary, cutoff, sides=("side", "bottom"), context=None):
    """The distance of every node of a mesh (f64[E, P]; a :class:`HexMesh`: f64[N]) or of points f64[..., 3] to the nearest
    node of ``boundary``'s faces of ``sides``, or ``cutoff`` where none lies within ``cutoff``: bit for bit the brute-force
    minimum of ``sqrt((dx*dx + dy*dy) + dz*dz)``.  The distance is to the nearest boundary node, so its resolution is the
    node spacing.  The default ``sides`` leave the free surface ("top") out.  The call runs on the boundary's own context:
    ``context`` is that one or ``None`` (``ValueError`` otherwise)."""
    bnd = _boundary_of(boundary)
    cutoff, mask = _cutoff(cutoff), _side_mask(sides)
    pts = points_of(mesh_or_points)                       # ([..., 3]: cutoff_distance refuses anything else)
    ctx = bnd._context(context)
    return ctx.cutoff_distance(pts, bnd._nodes(mask), cutoff)[0].numpy()


def _radii(inner, outer):
    inner, outer = float(inner), float(outer)
    if not (np.isfinite(inner) and np.isfinite(outer) and 0.0 <= inner <= outer):
        raise ValueError("the radii need 0 <= inner <= outer, both finite")
    return inner, outer


def taper_to_boundary(mesh, params, inner, outer, sides=("side", "bottom"), boundary=None, context=None):
    """The fields ``params`` of ``mesh`` damped towards its boundary: ``(values, ntapered)`` with values f64[C, E, P] (a
    :class:`HexMesh`: [C, N]) -- new arrays, the mesh's fields are untouched -- times 0 within ``inner`` of a boundary node
    of ``sides``, 1 beyond ``outer``, the smoothstep between, and ``ntapered`` the number of nodes whose weight is below 1.
    The boundary's own nodes get exactly 0; nodes beyond ``outer`` keep their bits.  ``boundary``: what
    :func:`mesh_boundary` returned for this mesh (``None``: computed here, with radial up; given: ``context`` is its own or ``None``).  The default ``sides`` leave the
    free surface ("top") alone: a kernel is damped towards absorbing sides and bottom, not towards the surface."""
    return _taper(_node_distance, mesh, params, inner, outer, sides, boundary, context)


def _boundary_of(boundary):
    """``boundary`` itself; anything that :func:`mesh_boundary` did not return is refused."""
    if not isinstance(boundary, Boundary):
        raise ValueError("boundary must come from mesh_boundary")
    return boundary


def _node_distance(ctx, bnd, points, mask, cutoff):
    """The distance step of this module: to the nearest node of ``bnd``'s faces of ``mask``, up to ``cutoff``, on the device."""
    return ctx.cutoff_distance(points, bnd._nodes(mask), max(cutoff, _MIN_CUTOFF))[0]


def _taper(distance, mesh, params, inner, outer, sides, boundary, context):
    """:func:`taper_to_boundary` with the distance step as an argument, as :func:`_blend` has it."""
    inner, outer = _radii(inner, outer)
    mask = _side_mask(sides)
    pts = points_of(mesh)
    _, fields = named_fields(mesh, params)
    if boundary is None:
        boundary = mesh_boundary(mesh, context=context)
    ctx = _boundary_of(boundary)._context(context)
    dist = distance(ctx, boundary, pts, mask, outer)
    out, ntapered = ctx.distance_taper(dist, inner, outer, fields.reshape(fields.shape[0], -1))
    return out.numpy().reshape(fields.shape), ntapered


def _blend(distance, regional, host, params, inner, outer, sides, nelem_to_search, tolerance, context):
    """:func:`blend_models` with the distance step as an argument: ``distance(ctx, boundary, points, mask, outer)`` gives
    the device array f64[U] that drives the weight (multimesh_amd.surface passes the distance to the faces themselves)."""
    inner, outer = _radii(inner, outer)
    mask = _side_mask(sides)
    gp_r, order_r = _gll_points_order(regional)
    gp_h, _ = _gll_points_order(host)
    if gp_r.shape[2] != 3 or gp_h.shape[2] != 3:
        raise ValueError("3-D meshes only")
    names, f_r = _mesh_fields(regional, params)
    _, f_h = _mesh_fields(host, names)
    ctx = context or default_context()
    bnd = mesh_boundary(regional, context=ctx)
    uniq, inv = ctx.unique_points(gp_h.reshape(-1, 3), ordered=False)
    vals, elem, _, _ = ctx.interpolate_gll(order_r, bnd._points, uniq, f_r, nelem_to_search=nelem_to_search,
                                           tolerance=tolerance, want_operator=True)
    dist = distance(ctx, bnd, uniq, mask, outer)
    inverse = inv.numpy()
    shape = gp_h.shape[:2]
    a = _scatter_back(vals.numpy(), inverse, f_h.shape)
    out, _, w = ctx.distance_taper(dist.numpy()[inverse].reshape(shape), inner, outer, a, b=f_h,
                                   elem=elem.numpy()[inverse].reshape(shape), want_weight=True)
    w = w.numpy()
    info = {"nlocated": int((elem.numpy()[inverse] >= 0).sum()), "nblended": int(((w > 0.0) & (w < 1.0)).sum()),
            "nreplaced": int((w == 1.0).sum())}
    return out.numpy().reshape(f_h.shape), info


def blend_models(regional, host, params, inner, outer, sides=("side", "bottom"), nelem_to_search=20, tolerance=1.05,
                 context=None):
    """A regional model put inside a larger one without a step along the region's outline: ``(values f64[C, E_h, P_h],
    info)``, the fields ``params`` on the nodes of ``host`` (a :class:`GllMesh` or Salvus mesh, as ``regional``).  The
    host's nodes are collapsed to their unique set, ``regional``'s fields are interpolated onto them
    (``Context.interpolate_gll``), every node gets its distance d to the nearest node of ``regional``'s boundary faces of
    ``sides`` (radial up) up to ``outer``, and with ``w`` = 0 for d <= ``inner``, 1 for d >= ``outer``, the smoothstep
    between, and 0 where no regional element holds the node::

        out = host where w == 0,  regional where w == 1,  (w * regional) + ((1 - w) * host)  between

    so host nodes outside the region keep their bits and nodes deeper than ``outer`` carry the interpolated value.
    ``info = {"nlocated", "nblended", "nreplaced"}``: the host's element-nodal nodes inside a regional element, those with
    0 < w < 1 and those with w == 1.  The default ``sides`` leave the free surface ("top") alone: the regional model
    reaches the surface at full weight."""
    return _blend(_node_distance, regional, host, params, inner, outer, sides, nelem_to_search, tolerance, context)
