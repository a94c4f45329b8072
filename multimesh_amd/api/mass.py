"""GLL mass matrices, volume integrals and the mass-weighted adjoint.  A nodal field of a spectral-element mesh is a
density: its inner product is a^T M b with the diagonal GLL mass matrix M[e][p] = w_p |det J_e(xi_p)|
(include/multimesh_hip.h, mm_gll_mass).  The reference has no counterpart: its mass matrix lives in Salvus."""
from __future__ import annotations

import numpy as np

from .. import synth
from ..device import default_context
from ..mesh import HexMesh
from ._common import _gll_points_order, hex8_corners
from .layers import _selected_layers


def gll_quadrature(order):
    """``(nodes, weights, D)`` of the GLL rule of order 1, 2 or 4: the tables ``mm_gll_mass`` is fed.  ``nodes`` =
    :func:`multimesh_amd.synth.gll_nodes_1d`, ``D[i][a] = l_a'(nodes[i])``."""
    return synth.gll_nodes_1d(order), synth.gll_weights_1d(order), synth.gll_derivative_matrix(order)


def _device_mass(points, order, ctx):
    mass, n_bad = ctx.gll_mass(order, points)
    if 0 < n_bad < mass.size:
        print(f"Warning: {n_bad} of {mass.size} GLL nodes have a Jacobian determinant that is not positive "
              "(inverted or collapsed elements); their mass is |det J|")
    return mass


def gll_mass_matrix(mesh, context=None):
    """The diagonal GLL mass matrix of a :class:`GllMesh` or a Salvus mesh, f64[E, P]: ``w_p |det J_e(xi_p)|`` at every
    node, so that ``sum(mass * f)`` is the integral of ``f`` over the mesh and ``sum(mass * a * b)`` the inner product of
    two fields.  Prints a warning when some but not all determinants are not positive (all: a left-handed mesh)."""
    ctx = context or default_context()
    pts, order = _gll_points_order(mesh)
    return _device_mass(pts, order, ctx).numpy()


def _hex8_mass(mesh: HexMesh, ctx):
    conn, corners = hex8_corners(mesh)                                               # the order-1 GLL mesh it is
    mass = _device_mass(corners, 1, ctx)
    with ctx.transpose_nodes(conn, mass, mesh.npoint) as op:
        lumped = op.apply(np.ones(mesh.nelem))                                       # [1, npoint]
    return lumped.reshape(mesh.npoint)


def hex8_mass_matrix(mesh: HexMesh, context=None):
    """The lumped nodal mass of a hex8 mesh, f64[npoint]: the order-1 element-nodal mass summed over the elements that
    share a node (``np.add.at(out, connectivity, mass)`` bit for bit, through the deterministic transpose)."""
    ctx = context or default_context()
    return _hex8_mass(mesh, ctx).numpy()


def integrate(mesh, params=None, layers=None, layer_ids=None, fluid=None, moho_idx=None, context=None):
    """``int f dV`` over a :class:`GllMesh` or a Salvus mesh for every parameter of ``params`` (names of element-nodal
    fields) -> f64[C]; ``params=None``: the volume, a float.  ``layers``: only the elements of these layers, anything
    :func:`assess_layers` takes (``integrate(mesh, layers="mantle")`` is the mantle's volume); ``layer_ids`` / ``fluid`` /
    ``moho_idx`` default to the mesh's ``layer`` and ``fluid`` elemental fields and its ``moho_idx`` global string.
    The sum runs on the device in the fixed order of ``mm_weighted_sum``: the same bits on every run."""
    ctx = context or default_context()
    pts, order = _gll_points_order(mesh)
    fields = None if params is None else np.stack([mesh.element_nodal_fields[p] for p in params])
    if layers is not None:
        picked, ids = _selected_layers(mesh, layers, layer_ids, fluid=fluid, moho_idx=moho_idx)
        mask = np.isin(ids, picked)
        pts = np.ascontiguousarray(pts[mask])
        fields = None if fields is None else np.ascontiguousarray(fields[:, mask])
    total = ctx.weighted_sum(_device_mass(pts, order, ctx), fields)
    return float(total[0]) if params is None else total


def _assemble(ctx, values, op, inverse):
    """values [C, N] (device) summed over the copies of every unique node and written back to every copy -> [C, N]."""
    ones = ctx.to_device(np.ones((inverse.shape[0], 1)))
    return ctx.gather(op.apply(values, point_major=False), inverse, ones, point_major=False)


def _assembler(ctx, gll_points):
    """(transposed scatter-sum operator, inverse int64[N, 1]) over the unique nodes of element-nodal points."""
    pts = ctx.asdevice(np.ascontiguousarray(gll_points, dtype=np.float64), np.float64)
    n = pts.size // pts.shape[-1]
    uniq, inv = ctx.unique_points(pts.reshape(n, pts.shape[-1]), ordered=False)
    inverse = inv.reshape(n, 1)
    return ctx.transpose_nodes(inverse, np.ones((n, 1)), uniq.shape[0]), inverse


def assemble_gll(values, gll_points, context=None):
    """Element-nodal values f64[C, E, P] (or [E, P]) summed over all copies of a shared node and written back to every
    copy -> f64[C, E, P]: the assembly ``A`` of spectral-element codes.  Copies of a node hold identical bits afterwards
    (one deterministic scatter-sum over ``unique_points``' inverse, then a gather)."""
    ctx = context or default_context()
    gp = np.ascontiguousarray(gll_points, dtype=np.float64)
    vals = np.ascontiguousarray(values, dtype=np.float64)
    if vals.shape[-2:] != gp.shape[:2] or vals.ndim not in (2, 3):
        raise ValueError("values must be [C, E, P] (or [E, P]) over gll_points [E, P, dim]")
    vals = vals.reshape(-1, gp.shape[0] * gp.shape[1])
    op, inverse = _assembler(ctx, gp)
    with op:
        return _assemble(ctx, ctx.to_device(vals), op, inverse).numpy().reshape((-1,) + gp.shape[:2])


def _mass_weighted(ctx, values, target_mass, npoints):
    """``target_mass[n] * values[n, c]`` -> device f64[N, C] (a gather with P = 1 over the identity index)."""
    vals = np.ascontiguousarray(values, dtype=np.float64).reshape(npoints, -1)
    tm = np.ascontiguousarray(target_mass, dtype=np.float64)
    if tm.shape != (npoints,):
        raise ValueError("target_mass must be [N], the mass of every target point")
    return ctx.gather(np.ascontiguousarray(vals.T), np.arange(npoints, dtype=np.int64)[:, None], tm[:, None])


def apply_gll_operator_adjoint(elements, coeffs, values, target_mass, source_mesh, assemble=True, context=None):
    """The adjoint of the GLL interpolation in the meshes' own inner products: the kernel ``K_c`` f64[C, E, P] on
    ``source_mesh`` (a :class:`GllMesh` or Salvus mesh) that solves ``A(M_c) K_c = A(P^T (M_f * K_f))``, where ``P`` is
    the operator ``elements`` / ``coeffs`` (:func:`get_element_weights`), ``K_f`` = ``values`` f64[N, C] (or [N]) at the
    targets, ``M_f`` = ``target_mass`` f64[N] the mass of every target point, ``M_c`` = :func:`gll_mass_matrix` of the
    source, ``P^T`` the deterministic :func:`apply_gll_operator_transpose` and ``A`` = :func:`assemble_gll` (the identity
    with ``assemble=False``: every element on its own).  Unlike the plain transpose the result does not grow with the
    number of targets per element, and it conserves the integral: ``sum(M_c * K_c) == sum(M_f * K_f)`` when every target
    was found.

    For targets that are the unique points of a fine GLL mesh, the mass of a point is its assembled mass::

        uniq, inv = get_unique_points(fine.gll_points)
        target_mass = np.empty(len(uniq))
        target_mass[inv] = assemble_gll(gll_mass_matrix(fine), fine.gll_points).reshape(-1)
    """
    ctx = context or default_context()
    el = np.ascontiguousarray(elements, dtype=np.int64)
    pts, order = _gll_points_order(source_mesh)
    weighted = _mass_weighted(ctx, values, target_mass, len(el))
    with ctx.transpose_elem(el, coeffs, pts.shape[0]) as op:
        rhs = op.apply(weighted)                                                      # [C, E, P]
    mass = _device_mass(pts, order, ctx)
    if assemble:
        n = pts.shape[0] * pts.shape[1]
        sum_op, inverse = _assembler(ctx, pts)
        with sum_op:
            rhs = _assemble(ctx, rhs.reshape(rhs.shape[0], n), sum_op, inverse)
            mass = _assemble(ctx, mass.reshape(1, n), sum_op, inverse).reshape(n)
    return ctx.divide_rows(rhs, mass, out=rhs).numpy().reshape((-1,) + pts.shape[:2])


def apply_operator_adjoint(mesh_a: HexMesh, enclosing_elem_node_indices, weights, values, target_mass, context=None):
    """The hex8 form of :func:`apply_gll_operator_adjoint`: ``(P^T (M_f * K_f)) / M_a`` -> f64[C, npoint] on mesh A's
    nodes, with ``M_a`` = :func:`hex8_mass_matrix` (the lumped nodal mass, already assembled)."""
    ctx = context or default_context()
    enc = np.ascontiguousarray(enclosing_elem_node_indices, dtype=np.int64)
    weighted = _mass_weighted(ctx, values, target_mass, len(enc))
    with ctx.transpose_nodes(enc, weights, mesh_a.npoint) as op:
        rhs = op.apply(weighted)                                                      # [C, npoint]
    return ctx.divide_rows(rhs, _hex8_mass(mesh_a, ctx), out=rhs).numpy()
