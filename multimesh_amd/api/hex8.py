"""The hex8 drop-in functions (the path the reference implements in its own C: scripts/cli.py:35-104, api.py:320-393,
interpolator.py:931-977), the operator behind them with its transposes, and the ``stored_array`` operator cache."""
from __future__ import annotations

import os
import time

import numpy as np

from ..device import default_context
from ..mesh import HexMesh
from ._common import TTI_PARAMS, _report, _report_not_found, latlondepth_to_xyz
from .earth import _sphere_mapped


def interpolate_operator(mesh_a: HexMesh, points, nelem_to_search=20, context=None):
    """``(enclosing_elem_node_indices int64[N,8], weights f64[N,8], nfailed)`` for arbitrary points:
    centroid -> kNN -> locate, i.e. reference cli.py:62-95 without the field loop.  This is the
    persistable operator of the reference's ``stored_array`` split."""
    ctx = context or default_context()
    points = np.ascontiguousarray(points, dtype=np.float64)
    field = np.zeros((1, mesh_a.npoint))
    _, enc, w, nfailed = ctx.interpolate_hex8_host(mesh_a.points, mesh_a.connectivity, points, field,
                                                   nelem_to_search=nelem_to_search, want_operator=True)
    return enc, w, nfailed


def apply_operator(mesh_a: HexMesh, enclosing_elem_node_indices, weights, params, context=None):
    """``np.sum(param_a[enc] * weights, axis=1)`` per parameter (reference cli.py:98-100) -> f64[N,C]."""
    ctx = context or default_context()
    return ctx.gather(mesh_a.fields_matrix(params), enclosing_elem_node_indices, weights).numpy()


def apply_operator_transpose(mesh_a: HexMesh, enclosing_elem_node_indices, weights, values, context=None):
    """The transpose of :func:`apply_operator`: values f64[N, C] (or [N]) on the targets -> f64[C, npoint] on mesh A's
    nodes, the layout of ``fields_matrix``.  ``np.add.at(out[c], enc, weights * values[:, c, None])`` bit for bit, the
    same on every run; ``enc`` / ``weights`` as :func:`interpolate_operator` or :func:`load_stored_operator` return them."""
    ctx = context or default_context()
    enc = np.ascontiguousarray(enclosing_elem_node_indices, dtype=np.int64)
    with ctx.transpose_nodes(enc, weights, mesh_a.npoint) as op:
        return op.apply(values).numpy()


def apply_gll_operator_transpose(elements, coeffs, values, nelem, context=None):
    """The transpose of ``np.sum(coeffs * field[elements], axis=1)``: values f64[N, C] (or [N]) on the targets ->
    f64[C, nelem, P] on the source elements' nodes; targets without an element (-1) contribute nothing.  ``elements`` /
    ``coeffs`` as :func:`get_element_weights` or :func:`load_stored_operator` return them."""
    ctx = context or default_context()
    with ctx.transpose_elem(np.ascontiguousarray(elements, dtype=np.int64), coeffs, nelem) as op:
        return op.apply(values).numpy()


def load_stored_operator(stored_array):
    """The reference's operator cache (interpolator.py:724-740): ``elements.npy`` + ``coeffs.npy`` in
    the ``stored_array`` directory.  Returns ``(elements, coeffs)`` or ``None`` when not (fully) there.
    For the hex8 path ``elements`` holds the 8 node ids per point (``enclosing_elem_node_indices``)."""
    if not stored_array:
        return None
    e_path, c_path = os.path.join(stored_array, "elements.npy"), os.path.join(stored_array, "coeffs.npy")
    if not (os.path.exists(e_path) and os.path.exists(c_path)):
        return None
    coeffs = np.load(c_path, allow_pickle=True)
    elements = np.load(e_path, allow_pickle=True)
    assert not np.isnan(coeffs).any(), "Stored coeffs matrix has NaNs"          # interpolator.py:735-740
    return elements, coeffs


def save_stored_operator(stored_array, elements, coeffs):
    """reference interpolator.py:797-810"""
    if not os.path.exists(stored_array):
        os.makedirs(stored_array)
    print("Will save matrices for later usage")
    np.save(os.path.join(stored_array, "elements.npy"), elements, allow_pickle=True)
    np.save(os.path.join(stored_array, "coeffs.npy"), coeffs, allow_pickle=True)


def interpolate_cached(mesh_a: HexMesh, points, params, stored_array=None, nelem_to_search=20, context=None):
    """hex8 interpolation with the reference's ``stored_array`` split: the first
    call builds and stores the operator, later calls skip kNN + locate and run only the HBM-bound
    gather.  Returns f64[N, len(params)]."""
    cached = load_stored_operator(stored_array)
    if cached is None:
        enc, w, _ = interpolate_operator(mesh_a, points, nelem_to_search, context)
        if stored_array:
            save_stored_operator(stored_array, enc, w)
    else:
        print("Matrix was already stored. Will use that one")
        enc, w = cached
    return apply_operator(mesh_a, enc, w, params, context)


def interpolate_mesh_a_to_b(mesh_a: HexMesh, mesh_b: HexMesh, params=("TTI",), context=None):
    """Interpolates values from mesh A onto the nodes of mesh B (reference cli.py:41-104).

    Attaches every parameter to ``mesh_b`` and, like the reference, asserts that no point failed."""
    params = list(params)
    if params and params[0] == "TTI":
        params = list(TTI_PARAMS)
    ctx = context or default_context()
    nelem_to_search = 20  # reference cli.py:69
    values, nfailed = ctx.interpolate_hex8_host(mesh_a.points, mesh_a.connectivity, mesh_b.points,
                                                mesh_a.fields_matrix(params), nelem_to_search=nelem_to_search)
    for i, param in enumerate(params):
        mesh_b.attach_field(param, values[:, i])
    assert nfailed == 0, f"{nfailed} points could not be interpolated."
    return mesh_b


def interpolate_to_points(mesh, points, params_to_interp, make_spherical=False, geocentric=False,
                          nelem_to_search=25, context=None):
    """Maps values from a mesh to predefined points, xyz or geocentric latlondepth
    (reference api.py:320-350).  Returns f64[npoints, nparams]; points that are not found get zero
    (reference interpolator.py:963-977).  ``make_spherical``: the mesh's nodes are mapped onto the sphere of
    its 1-D model first (its ``z_node_1D`` field, :func:`map_to_sphere`) -- a mapped copy: ``mesh`` is not
    changed; the points are taken as they are, as in the reference (interpolator.py:945-946)."""
    if geocentric:
        points = latlondepth_to_xyz(points)
    ctx = context or default_context()
    nodes = _sphere_mapped(mesh, ctx).numpy() if make_spherical else mesh.points
    points = np.ascontiguousarray(points, dtype=np.float64)
    vals, nfailed = ctx.interpolate_hex8_host(nodes, mesh.connectivity, points,
                                              mesh.fields_matrix(params_to_interp), nelem_to_search=nelem_to_search)
    _report_not_found(nfailed)
    return vals


def interpolate_to_mesh(old_mesh, new_mesh, params_to_interp=("VSV", "VSH", "VPV", "VPH"), make_spherical=False,
                        context=None):
    """Interpolate ``params_to_interp`` from old_mesh onto the nodes of new_mesh (reference api.py:353-393).
    Values that are not found are given zero.  The reference ALWAYS maps both meshes onto the sphere of their
    1-D model first (their ``z_node_1D`` fields); here that is ``make_spherical=True``, and the default keeps
    the coordinates as they are.  Either way the meshes' coordinates are not changed (the reference restores
    them, :388-390); only the fields are attached to ``new_mesh``."""
    start = time.time()
    if make_spherical:
        ctx = context or default_context()
        targets = _sphere_mapped(new_mesh, ctx).numpy()
        source = HexMesh(_sphere_mapped(old_mesh, ctx).numpy(), old_mesh.connectivity, old_mesh.nodal_fields)
        vals = interpolate_to_points(source, targets, list(params_to_interp), context=ctx)
    else:
        vals = interpolate_to_points(old_mesh, new_mesh.points, list(params_to_interp), context=context)
    for i, param in enumerate(params_to_interp):
        new_mesh.attach_field(param, vals[:, i])
    _report(start)
    return new_mesh
