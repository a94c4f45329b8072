"""File-level drivers: the reference's names and arguments; files through multimesh_amd.io (h5py for HDF5 paths, scipy's
netCDF reader for classic Exodus files), or already open h5py-like / mesh objects in place of the paths.  The work itself
is the array cores of :mod:`.gll` and :mod:`.layers`."""
import os
import time

import numpy as np

from .. import io as mio
from ..device import default_context
from ..mesh import HexMesh
from ._common import GllMesh, _components_first, _order_from_point_count, _report, latlondepth_to_xyz
from .earth import _sphere_mapped
from .gll import _gll_operator_over_all_points, interpolate_gll_to_nodes, interpolate_hex8_to_gll, query_gll_model
from .hex8 import load_stored_operator, save_stored_operator
from .layers import _layer_metadata, fix_fluid_solid, interpolate_gll_to_gll_layered


def query_model(coordinates, model, nelem_to_search=20, parameters="TTI", model_path="MODEL/data",
                coordinates_path="MODEL/coordinates", context=None):
    """Model parameters at ``coordinates`` f64[N, 3] = (latitude, longitude, depth in m) from a Salvus GLL
    model file (reference api.py:13-58, interpolator.py:60-139) -> f64[N, nparam] in the file's parameter
    order.  ``parameters`` is accepted and ignored, as in the reference."""
    start = time.time()
    points, data, _ = mio.load_hdf5_params_to_memory(model, model_path, coordinates_path)
    coordinates = np.asarray(coordinates, dtype=np.float64)
    assert coordinates.ndim == 2 and coordinates.shape[1] == 3, "Make sure coordinates array has shape N,3"
    values = query_gll_model(points, data, latlondepth_to_xyz(coordinates), nelem_to_search, context=context)
    _report(start)
    return values


def exodus_2_gll(mesh, gll_model, gll_order=4, dimensions=3, nelem_to_search=20, parameters="TTI",
                 model_path="MODEL/data", coordinates_path="MODEL/coordinates", context=None):
    """Nodal parameters of an exodus hex8 mesh onto the GLL points of an HDF5 model, written to
    ``gll_model[model_path]`` as f64[nelem, nparam, P] with fresh dimension labels (reference api.py:61-103,
    interpolator.py:142-224; ``gll_order`` / ``dimensions`` are read off the coordinates).  ``mesh``: an
    Exodus file or a mesh object with ``points``, ``connectivity``, ``get_nodal_field``; ``gll_model``: an HDF5
    file or an open writable h5py-like object."""
    start = time.time()
    exodus = mio.Exodus(mesh) if isinstance(mesh, (str, os.PathLike)) else mesh
    parameters = mio.pick_parameters(parameters)
    mesh_a = HexMesh(exodus.points, exodus.connectivity, {p: exodus.get_nodal_field(p) for p in parameters})
    with mio.open_h5(gll_model, "r+") as gll:
        gll_coords = np.array(gll[coordinates_path][:], dtype=np.float64)
        values, nfailed = interpolate_hex8_to_gll(mesh_a, gll_coords, parameters, nelem_to_search, context=context,
                                                  return_nfailed=True)
        assert nfailed == 0, f"{nfailed} points could not be interpolated."
        mio.remove_and_create_empty_dataset(gll, parameters, model_path, coordinates_path)
        gll[model_path][:, :, :] = values.transpose(1, 0, 2)
    _report(start)


def gll_2_exodus(gll_model, exodus_model, gll_order=4, dimensions=3, nelem_to_search=20, parameters="TTI",
                 model_path="MODEL/data", coordinates_path="MODEL/coordinates", gradient=False, context=None):
    """Every parameter of a GLL model onto the nodes of an exodus mesh, attached as its nodal fields
    (reference api.py:277-317, interpolator.py:227-285; like the reference, ``parameters`` is replaced by
    the model's own list and the exodus variables must exist).  ``exodus_model``: an Exodus file (opened
    in mode "a") or a mesh object with ``points`` and ``attach_field``."""
    start = time.time()
    with mio.open_h5(gll_model, "r") as gll:
        gll_points = np.array(gll[coordinates_path][:], dtype=np.float64)
        gll_data = np.array(gll[model_path][:])
        parameters = mio.dimension_labels(gll[model_path], 1)
    exodus = mio.Exodus(exodus_model, mode="a") if isinstance(exodus_model, (str, os.PathLike)) else exodus_model
    shape_order = _order_from_point_count(gll_points.shape[1], gll_points.shape[2])
    values = interpolate_gll_to_nodes(gll_points, gll_data, exodus.points, shape_order, nelem_to_search, context)
    for i, param in enumerate(parameters):
        exodus.attach_field(param, values[:, i])
    _report(start)


def gll_2_gll(from_gll, to_gll, nelem_to_search=20, parameters="ISO", from_model_path="MODEL/data",
              to_model_path="MODEL/data", from_coordinates_path="MODEL/coordinates",
              to_coordinates_path="MODEL/coordinates", gradient=False, stored_array=None, context=None):
    """All parameters of one GLL model onto the GLL points of another, written to ``to_gll[to_model_path]``
    (reference api.py:106-155, interpolator.py:621-852): unique target points (device ``np.unique``),
    :func:`_gll_operator_over_all_points` with hard elements ignored, ``values[recon]`` scattered back, fluid
    elements and solid elements that caught a zero VS keep their previous values unless ``gradient``.  Like
    the reference, ``parameters`` is replaced by the source model's own list.  ``stored_array``: directory of
    ``elements.npy`` + ``coeffs.npy``; ``coeffs.npy`` is written as f64[1, P, U] -- the reference writes
    ``nparam`` identical copies [nparam, P, U] and broadcasts either on load -- and both are read."""
    start = time.time()
    ctx = context or default_context()
    print("Initialization stage")
    print(f"Stored array: {stored_array}")
    original_points, original_data, parameters = mio.load_hdf5_params_to_memory(from_gll, from_model_path,
                                                                                from_coordinates_path)
    with mio.open_h5(to_gll, "r+") as new:
        new_points = np.array(new[to_coordinates_path][:], dtype=np.float64)
        elem_params = mio.dimension_labels(new["MODEL/element_data"], 1)
        fluid_elements = np.array(new["MODEL/element_data"][:, elem_params.index("fluid")]).astype(bool)
        solid_elements = np.invert(fluid_elements)
        new_values = np.array(new[to_model_path][:], dtype=np.float64)
        unique_new_points, recon = ctx.unique_points(new_points.reshape(-1, new_points.shape[2]))
        stored = load_stored_operator(stored_array)
        if stored is not None:
            print("Matrix was already stored. Will use that one")
            element, coeffs = stored
            element = np.asarray(element).astype(np.int64)
            if coeffs.ndim == 3:                       # [nparam or 1, P, U] as the reference stores it
                coeffs = np.ascontiguousarray(coeffs[0].T)
        else:
            print("Now we start interpolating")
            element, coeffs = _gll_operator_over_all_points(ctx, np.ascontiguousarray(original_points),
                                                            unique_new_points, nelem_to_search, True)
            if stored_array:
                save_stored_operator(stored_array, element.numpy(), coeffs.numpy().T[None, :, :])
        unique_values = ctx.gather_elem(_components_first(original_data), element, coeffs).numpy()     # [U, C]
        values = np.ascontiguousarray(unique_values[recon.numpy()].reshape(new_points.shape[0], new_points.shape[1],
                                                                          len(parameters)).swapaxes(1, 2))
        if not gradient:
            if new_values.shape != values.shape:
                raise ValueError("the receiving model must already hold the source model's parameters "
                                 f"({values.shape[1]}), it has {new_values.shape[1]}")
            values = fix_fluid_solid(values, new_values, solid_elements, parameters, context=ctx)
        mio.remove_and_create_empty_dataset(new, parameters, to_model_path, to_coordinates_path)
        new[to_model_path][:, :, :] = values
    _report(start)


def _gll_2_gll_layered(from_gll, to_gll, layers, nelem_to_search, parameters, stored_array, make_spherical, context,
                       acceptance, keep_existing, tolerance=1.05):
    """The three layered drivers.  ``keep_existing``: elements outside ``layers`` keep ``to_gll``'s values, else zero."""
    original_mesh = mio.SalvusMesh(from_gll, fast_mode=False)
    new_mesh = mio.SalvusMesh(to_gll, fast_mode=False)
    if make_spherical:
        # (reference interpolator.py:326-339, :484-494, :1016-1026: the readers' copies of the coordinates; no file is written)
        ctx = context or default_context()
        original_mesh.points = _sphere_mapped(original_mesh, ctx).numpy()
        new_mesh.points = _sphere_mapped(new_mesh, ctx).numpy()
    if isinstance(parameters, str) and parameters == "all":
        parameters = list(original_mesh.element_nodal_fields.keys())
    parameters = mio.pick_parameters(parameters)
    mesh_a = GllMesh(original_mesh.points, original_mesh.shape_order,
                     {p: original_mesh.element_nodal_fields[p] for p in parameters})
    existing = np.stack([new_mesh.element_nodal_fields[p] for p in parameters]) if keep_existing else None
    values = interpolate_gll_to_gll_layered(mesh_a, original_mesh.elemental_fields["layer"], new_mesh.points,
                                            new_mesh.elemental_fields["layer"], parameters, layers=layers,
                                            nelem_to_search=nelem_to_search, tolerance=tolerance,
                                            stored_array=stored_array, existing=existing, context=context,
                                            acceptance=acceptance, **_layer_metadata(original_mesh))
    for i, param in enumerate(parameters):
        new_mesh.attach_field(name=param, data=values[i])


def gll_2_gll_layered_multi_two(from_gll, to_gll, layers, nelem_to_search=30, parameters="all", stored_array=None,
                                make_spherical=False, tolerance=1.05, context=None):
    """Layer by layer, GLL model to GLL model, through the fast Salvus-mesh reader (reference api.py:645-699,
    interpolator.py:980-1082): the ``layer`` elemental field of both meshes, :func:`interpolate_gll_to_gll_layered`,
    every parameter attached to ``to_gll``.  ``layers``: "all" or a list of layer numbers (the Earth presets
    need mesh metadata).  ``make_spherical``: both meshes' coordinates are mapped onto the sphere of their 1-D
    model (their ``z_node_1D`` fields) right after they are read (:1016-1026); the files' ``MODEL/coordinates``
    are not changed."""
    start = time.time()
    _gll_2_gll_layered(from_gll, to_gll, layers, nelem_to_search, parameters, stored_array, make_spherical, context,
                       acceptance="tolerance", keep_existing=True, tolerance=tolerance)
    _report(start)


def gll_2_gll_layered(from_gll, to_gll, layers, nelem_to_search=20, parameters="ISO", stored_array=None,
                      make_spherical=False, context=None):
    """Layer by layer with the bounding-box acceptance loop (reference api.py:158-211, interpolator.py:288-439);
    elements of ``to_gll`` outside ``layers`` come out ZERO, as the reference's ``np.zeros_like`` fields do
    (:421).  Superseded in the reference by :func:`gll_2_gll_layered_multi_two`."""
    start = time.time()
    print("Initialization stage")
    _gll_2_gll_layered(from_gll, to_gll, layers, nelem_to_search, parameters, stored_array, make_spherical, context,
                       acceptance="bbox", keep_existing=False)
    _report(start)


def gll_2_gll_layered_multi(from_gll, to_gll, layers="nocore", nelem_to_search=20, parameters="all", threads=None,
                            stored_array=None, make_spherical=False, context=None):
    """The same per layer in parallel (reference api.py:214-274, interpolator.py:442-618: a process pool over
    the layers -- here every layer is a device pass, ``threads`` is accepted and ignored); elements outside
    ``layers`` keep the values ``to_gll`` holds (:606)."""
    start = time.time()
    print("Initialization stage")
    _gll_2_gll_layered(from_gll, to_gll, layers, nelem_to_search, parameters, stored_array, make_spherical, context,
                       acceptance="bbox", keep_existing=True)
    _report(start)
