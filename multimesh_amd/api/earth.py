"""Earth meshes on the sphere of their 1-D model and stretched to an ellipse (reference interpolator.py:1085-1144)."""
import numpy as np

from ..device import default_context
from ..mesh import HexMesh
from ._common import R_EARTH, GllMesh, _mesh_points, hex8_corners


def _z_node_1d(mesh):
    """The mesh's ``z_node_1D`` field: element-nodal (``element_nodal_fields``, or a Salvus file's ``MODEL/data``
    read on demand) or nodal (``nodal_fields`` of a :class:`HexMesh`)."""
    for attr in ("element_nodal_fields", "nodal_fields"):
        fields = getattr(mesh, attr, None)
        if fields is not None and "z_node_1D" in fields:
            return np.ascontiguousarray(fields["z_node_1D"], dtype=np.float64)
    if "z_node_1D" in getattr(mesh, "nodal_parameter_indices", ()):
        return np.ascontiguousarray(mesh.get_element_nodal_field("z_node_1D"), dtype=np.float64)
    raise ValueError("the mesh has no z_node_1D field (the radius of its 1-D model over 6371 km, which "
                     "map_to_sphere scales every point to)")


def _sphere_layout(mesh):
    """(points, z_node_1D, connectivity or None) as :meth:`Context.map_to_sphere` takes them."""
    pts = np.asarray(_mesh_points(mesh))
    if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
        raise ValueError(f"map_to_sphere maps 3-D meshes only (points of shape {pts.shape})")
    z = _z_node_1d(mesh)
    if z.shape == pts.shape[:-1]:                  # element-nodal points, or a nodal field: one radius per point
        return pts, z, None
    connectivity = getattr(mesh, "connectivity", None)
    if pts.ndim != 2 or connectivity is None or np.shape(connectivity) != z.shape:
        raise ValueError(f"z_node_1D of shape {z.shape} fits neither the points {pts.shape} nor the connectivity")
    return pts, z, connectivity


def _sphere_mapped(mesh, ctx):
    """The mesh's points mapped onto the sphere of its 1-D model, as a new device array (the mesh is untouched)."""
    pts, z, connectivity = _sphere_layout(mesh)
    return ctx.map_to_sphere(np.ascontiguousarray(pts, dtype=np.float64), z, connectivity=connectivity,
                             r_ref=R_EARTH)


def _set_points(mesh, mapped):
    pts = _mesh_points(mesh)
    if isinstance(pts, np.ndarray) and pts.dtype == np.float64 and pts.flags.writeable and pts.shape == mapped.shape:
        pts[...] = mapped                          # in place, like the reference's x[r > 0] = ... on views
    elif isinstance(mesh, GllMesh):
        mesh.gll_points = mapped
    else:
        mesh.points = mapped


def map_to_sphere(mesh, context=None):
    """Maps an Earth mesh onto the sphere of its 1-D model, IN PLACE (reference interpolator.py:1125-1144):
    every point p with |p| > 0 becomes ``((p * 6371000) * z_node_1D) / |p|``, bit-identical to the reference's
    NumPy statements; points at the centre are left alone.  Runs on the device (:meth:`Context.map_to_sphere`).

    ``mesh``: a :class:`GllMesh` or a Salvus mesh (element-nodal points [E, P, 3] and an element-nodal
    ``z_node_1D``), a :class:`HexMesh` with a nodal ``z_node_1D`` field, or any object with ``points`` [N, 3],
    ``connectivity`` [E, P] and an element-nodal ``z_node_1D`` in ``element_nodal_fields`` -- node n then takes
    the value at its first occurrence in the flattened connectivity, as the reference's UnstructuredMesh branch
    does (a node no element references raises ``ValueError``).  Raises ``ValueError`` without ``z_node_1D`` and
    for 2-D meshes.  Returns the mesh."""
    ctx = context or default_context()
    _set_points(mesh, _sphere_mapped(mesh, ctx).numpy())
    return mesh


def _element_nodal_base(mesh, ctx):
    """(gll_points [E, P, 3], z_node_1D [E, P], shape_order) of a base mesh for map_to_ellipse.  A node layout
    gives every copy of a node the node's own value (first occurrence), as the reference's r_ratio[connectivity]."""
    pts, z, connectivity = _sphere_layout(mesh)
    if pts.ndim == 3:
        return np.ascontiguousarray(pts, dtype=np.float64), z, int(mesh.shape_order)
    if connectivity is not None:
        z = z.reshape(-1)[ctx.first_occurrence(connectivity, pts.shape[0]).numpy()]
    if isinstance(mesh, HexMesh):        # exodus hex8 -> the tensor order of an order-1 GLL element
        conn, order = hex8_corners(mesh)[0], 1
    else:                                # GLL nodes listed in tensor order (p = i + (n+1) j + (n+1)^2 k)
        conn, order = np.asarray(mesh.connectivity), int(mesh.shape_order)
    return np.ascontiguousarray(pts[conn], dtype=np.float64), np.ascontiguousarray(z[conn]), order


def map_to_ellipse(base_mesh, mesh, nelem_to_search=25, tolerance=1.05, context=None):
    """Stretches ``mesh`` (IN PLACE) to the ellipticity and topography of ``base_mesh`` (reference
    interpolator.py:1085-1122, whose call to get_element_weights lacks its shape_order argument and cannot
    run as written; this follows its evident intent):

    1. the radial ratio ``(|p| / 6371000) / z_node_1D`` on the base's element-nodal points;
    2. sphere-mapped copies of both meshes (:func:`map_to_sphere`'s arithmetic);
    3. the ratio interpolated at the mapped points of ``mesh`` through the GLL path of the base
       (:meth:`Context.interpolate_gll`: centroid kNN, ``tolerance``, no snapping);
    4. if any point has no enclosing element, ``ValueError`` -- before anything is written;
    5. ``mesh``'s points become ``ratio * (mapped point)``.

    ``base_mesh`` is never modified.  It needs element-nodal GLL points (a :class:`GllMesh`, a Salvus mesh), a
    :class:`HexMesh`, or ``points`` + ``connectivity`` in GLL tensor order + ``shape_order``.  Returns ``mesh``."""
    ctx = context or default_context()
    gp, z_en, order = _element_nodal_base(base_mesh, ctx)
    gp_d = ctx.to_device(gp)
    ratio = ctx.sphere_ratio(gp_d, z_en, r_ref=R_EARTH)
    base_sphere = ctx.map_to_sphere(gp_d, z_en, r_ref=R_EARTH)
    targets = _sphere_mapped(mesh, ctx)
    flat = targets.reshape(targets.size // 3, 3)
    values, missing = ctx.interpolate_gll(order, base_sphere, flat, ratio, nelem_to_search=nelem_to_search,
                                          tolerance=tolerance)
    if missing:
        raise ValueError(f"{missing} points could not find an enclosing element.")
    ctx.scale_points(targets, values, out=targets)
    _set_points(mesh, targets.numpy())
    return mesh
