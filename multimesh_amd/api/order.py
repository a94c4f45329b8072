"""The GLL order of a model, changed on its own mesh (include/multimesh_hip.h, mm_gll_tensor_apply).
The same elements at another order: every target node sits in a known element at a known reference coordinate, so nothing
is searched, no node can fail, and a node on an element face takes its value from its own element."""
from __future__ import annotations

import time

import numpy as np

from .. import io as mio, synth
from ..device import default_context
from ._common import GllMesh, _gll_points_order, _mesh_fields, _report
from .mass import _device_mass


def gll_order_table(order_in, order_out):
    """``R[q][a] = l_a^in(g_q^out)`` f64[order_out + 1, order_in + 1], the 1-D table ``mm_gll_tensor_apply`` is fed: the
    Lagrange polynomials of the GLL nodes of ``order_in`` at the GLL nodes of ``order_out``
    (:func:`multimesh_amd.synth.gll_nodes_1d`).  A row at a coinciding node is exactly a unit row; every other entry is the
    product of ``(x - g_b) / (g_a - g_b)`` over ``b != a`` in ascending ``b``.  The transpose of the interpolation
    ``order_in -> order_out`` is the same kernel with ``R.T`` (contiguous) and the orders swapped."""
    return synth.gll_order_table(order_in, order_out)


def _order_of(npoints, dim):
    """The GLL order of elements with ``npoints`` nodes in ``dim`` dimensions (1, 2 or 4, else ValueError)."""
    for order in (1, 2, 4):
        if (order + 1) ** int(dim) == int(npoints):
            return order
    raise ValueError(f"{npoints} points per element in {dim} dimensions is not a GLL element of order 1, 2 or 4")


def gll_order_apply(values, order_in, order_out, dim, transpose=False, context=None):
    """The array core: element-nodal values f64[C, E, P_in] (or [E, P_in]) at the GLL nodes of ``order_in`` -> the same
    shape with P_out at the nodes of ``order_out``, by interpolation on every element (up: exact for the polynomial the
    field is; down: the values at the coinciding nodes).  With ``transpose=True`` it applies ``I^T`` of the interpolation
    ``I: order_out -> order_in`` instead: this is how a gradient with respect to an order-4 model becomes the gradient with
    respect to the order-2 model it was interpolated from (``<I u, v> = <u, I^T v>``).  Equal orders return a copy."""
    vals = np.ascontiguousarray(values, dtype=np.float64)
    order_in, order_out = int(order_in), int(order_out)
    synth.gll_nodes_1d(order_in), synth.gll_nodes_1d(order_out)                   # (ValueError for an order without tables)
    if dim not in (2, 3):
        raise ValueError("dim must be 2 or 3")
    if vals.ndim not in (2, 3) or vals.shape[-1] != (order_in + 1) ** dim:
        raise ValueError(f"values must be [C, E, P] (or [E, P]) with P = {(order_in + 1) ** dim}, got {vals.shape}")
    if order_in == order_out:
        return vals.copy()
    ctx = context or default_context()
    out = ctx.gll_tensor_apply(order_in, order_out, dim, vals, layout=0, transpose=transpose).numpy()
    return out[0] if vals.ndim == 2 else out


def resample_gll_order(mesh: GllMesh, new_order, params=None, context=None):
    """``mesh`` at another GLL order: a new :class:`GllMesh` on the same elements whose coordinates and element-nodal
    fields (``params``: names, None = all) are the interpolants of the old ones at the GLL nodes of ``new_order``.  Going up
    is exact for the polynomial a field is on its element; going down is the subsample on the coinciding nodes (up and
    down again returns the input bit for bit).  Unlike the search route of :func:`interpolate_gll_to_gll`, no node can fail
    to locate and a node on an element face takes its value from its own element, so a model that jumps across that face
    stays sharp.  The same order returns a copy; ``mesh`` is not modified."""
    pts, order = _gll_points_order(mesh)
    new_order = int(new_order)
    synth.gll_nodes_1d(new_order), synth.gll_nodes_1d(order)                      # (ValueError for an order without tables)
    names, fields = _mesh_fields(mesh, params)
    if new_order == order:
        return GllMesh(pts.copy(), order, {n: fields[i].copy() for i, n in enumerate(names)})
    dim = pts.shape[2]
    ctx = context or default_context()
    new_pts = ctx.gll_tensor_apply(order, new_order, dim, pts, layout=1).numpy()
    new_fields = ctx.gll_tensor_apply(order, new_order, dim, fields, layout=0).numpy() if names else fields
    return GllMesh(new_pts, new_order, {n: new_fields[i] for i, n in enumerate(names)})


def _restrict(ctx, pts_d, order, coarse_order, dim, values, layout):
    """``M_c^-1 I^T M_f values`` in one pass: (device result, device coarse coordinates)."""
    coarse_pts = ctx.gll_tensor_apply(order, coarse_order, dim, pts_d, layout=1)
    fine_mass = _device_mass(pts_d, order, ctx)
    coarse_mass = _device_mass(coarse_pts, coarse_order, ctx)
    out = ctx.gll_tensor_apply(order, coarse_order, dim, values, layout=layout, transpose=True, scale_in=fine_mass,
                               div_out=coarse_mass)
    return out, coarse_pts


def restrict_gll_kernel(mesh_fine: GllMesh, coarse_order, params=None, context=None):
    """A sensitivity kernel from the simulation's order back to the model's: the mass-weighted adjoint
    ``K_c = M_c^-1 I^T M_f K_f`` of the interpolation ``I: coarse_order -> mesh_fine.shape_order`` on every element, with
    ``M_f`` = :func:`gll_mass_matrix` of ``mesh_fine`` and ``M_c`` that of the coarse mesh (the fine coordinates
    subsampled).  Returns a new :class:`GllMesh` at ``coarse_order`` with the fields ``params`` (names, None = all).

    What it is for: densities -- sensitivity kernels, like :func:`apply_gll_operator_adjoint`.  It keeps the integral of
    the GLL quadratures, ``sum(M_c K_c) == sum(M_f K_f)`` up to rounding, because the rows of ``I`` sum to one.
    What it is not: it does not reproduce constants on deformed elements (``M_c^-1 I^T M_f 1 != 1`` where the Jacobian
    varies), so a MODEL goes through :func:`resample_gll_order` instead; and it is the lumped-mass adjoint per element, not
    a consistent-mass L2 projection, which is out of scope.  ``coarse_order`` must be below the mesh's order."""
    pts, order = _gll_points_order(mesh_fine)
    coarse_order = int(coarse_order)
    synth.gll_nodes_1d(coarse_order), synth.gll_nodes_1d(order)
    if coarse_order >= order:
        raise ValueError(f"a restriction goes down in order: coarse_order {coarse_order} is not below {order}")
    names, fields = _mesh_fields(mesh_fine, params)
    ctx = context or default_context()
    out, coarse_pts = _restrict(ctx, ctx.to_device(pts), order, coarse_order, pts.shape[2], fields, 0)
    out = out.numpy()
    return GllMesh(coarse_pts.numpy(), coarse_order, {n: out[i] for i, n in enumerate(names)})


def _change_order_plan(from_points_shape, to_points_shape, from_data_shape, source_parameters, parameters, kernel):
    """What :func:`gll_change_order` decides from shapes and names alone, before any device is touched:
    (order_from, order_to, dim, parameter names, their indices in the source's data)."""
    if len(from_points_shape) != 3 or len(to_points_shape) != 3:
        raise ValueError("coordinates must be [nelem, P, dim]")
    dim = int(from_points_shape[2])
    if dim not in (2, 3) or int(to_points_shape[2]) != dim:
        raise ValueError(f"both meshes must be 2-D or both 3-D (dimensions {from_points_shape[2]} and {to_points_shape[2]})")
    order_from, order_to = _order_of(from_points_shape[1], dim), _order_of(to_points_shape[1], dim)
    if from_points_shape[0] != to_points_shape[0]:
        raise ValueError(f"the two files must hold the same elements in the same order: {from_points_shape[0]} and "
                         f"{to_points_shape[0]} elements")
    if kernel and order_to >= order_from:
        raise ValueError(f"kernel=True is the mass-weighted restriction and goes down in order only (from {order_from} to "
                         f"{order_to})")
    source_parameters = list(source_parameters)
    if tuple(from_data_shape) != (from_points_shape[0], len(source_parameters), from_points_shape[1]):
        raise ValueError(f"the source model must be [nelem, nparam, P] = {(from_points_shape[0], len(source_parameters), from_points_shape[1])}, "
                         f"it is {tuple(from_data_shape)}")
    if isinstance(parameters, str) and parameters == "all":
        names = source_parameters
    else:
        names = mio.pick_parameters(parameters)
        missing = [p for p in names if p not in source_parameters]
        if missing:
            raise ValueError(f"the source model has no {missing} (it has {source_parameters})")
    return order_from, order_to, dim, names, [source_parameters.index(p) for p in names]


def gll_change_order(from_gll, to_gll, parameters="all", from_model_path="MODEL/data", to_model_path="MODEL/data",
                     coord_rtol=1e-2, kernel=False, context=None):
    """The model of ``from_gll`` written into ``to_gll[to_model_path]``, where both files hold the SAME elements in the same
    order at different GLL orders (read from the point counts): the route from an order-2 model to the order-4 simulation
    mesh and back, without a search.  Paths or open h5py-like objects, as in :func:`gll_2_gll`.

    The ``from`` coordinates are resampled on the device to the order of ``to`` and must agree with ``to``'s coordinates,
    element by element, to within ``coord_rtol`` times the element's largest bounding-box edge; otherwise ``ValueError``
    names the first offending element and nothing is written.  (1e-2 is a condition, not a measurement: a mesher's order-4
    nodes on a sphere differ from the order-1 interpolant by about h / (8 R) of an element of width h, under 1e-2 for
    elements up to 500 km, while a wrong element order differs by order one.)

    Values go through the kernel in the ``[E, C, P]`` layout of ``MODEL/data``.  ``kernel=False``: interpolation
    (:func:`resample_gll_order`).  ``kernel=True``: the mass-weighted restriction of :func:`restrict_gll_kernel`, going down
    only.  ``parameters``: "all" (the source model's own list), a preset of :func:`multimesh_amd.io.pick_parameters` or a
    list of names the source holds; the receiving dataset is replaced and labelled with them."""
    start = time.time()
    from_points, from_data, source_parameters = mio.load_hdf5_params_to_memory(from_gll, from_model_path)
    with mio.open_h5(to_gll, "r+") as new:
        to_points = np.ascontiguousarray(new["MODEL/coordinates"][:], dtype=np.float64)
        order_from, order_to, dim, names, picked = _change_order_plan(from_points.shape, to_points.shape, from_data.shape,
                                                                      source_parameters, parameters, kernel)
        data = np.ascontiguousarray(np.asarray(from_data, dtype=np.float64)[:, picked, :])            # [E, C, P_from]
        nelem = to_points.shape[0]
        ctx = context or default_context()
        pts_d = ctx.to_device(from_points)
        if nelem:
            got = pts_d if order_from == order_to else ctx.gll_tensor_apply(order_from, order_to, dim, pts_d, layout=1)
            deviation, edge = (x.numpy() for x in ctx.element_deviation(got, to_points))                # [E] each
            bad = np.flatnonzero(~(deviation <= float(coord_rtol) * edge))                              # (NaN is bad too)
            if bad.size:
                e = int(bad[0])
                raise ValueError(f"element {e} of the two files is not the same element: its resampled coordinates differ "
                                 f"from the receiving file's by {float(deviation[e]):.3e}, more than coord_rtol = {coord_rtol} "
                                 f"times its largest bounding-box edge {float(edge[e]):.3e} ({int(bad.size)} of {nelem} "
                                 "elements differ); nothing was written")
        if order_from == order_to:
            values = data.copy()
        elif kernel:
            values = _restrict(ctx, pts_d, order_from, order_to, dim, data, 2)[0].numpy()
        else:
            values = ctx.gll_tensor_apply(order_from, order_to, dim, data, layout=2).numpy()
        mio.remove_and_create_empty_dataset(new, names, to_model_path, "MODEL/coordinates")
        new[to_model_path][:, :, :] = values
    _report(start)
