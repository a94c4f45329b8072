"""The constants, :class:`GllMesh`, how a mesh's points and fields are read, and the steps several modules share."""
import time

import numpy as np

TTI_PARAMS = ["VSH", "VSV", "VPV", "VPH", "RHO", "ETA", "QKAPPA", "QMU"]  # reference cli.py:58-59
R_EARTH = 6371000.0   # the radius map_to_sphere scales z_node_1D by (reference interpolator.py:1093, :1137)


def _report(start):
    # the reference prints wall-clock around every API call (api.py:39-57)
    runtime = time.time() - start
    if runtime >= 60:
        print(f"Finished in time: {runtime / 60} minutes")
    else:
        print(f"Finished in time: {runtime} seconds")


def latlondepth_to_xyz(latlondepth):
    """reference utils.py:526-542 (r_earth = 6371000 m, geocentric latitude)."""
    latlondepth = np.asarray(latlondepth, dtype=np.float64)
    r = 6371000.0 - latlondepth[:, 2]
    colat = np.deg2rad(90.0 - latlondepth[:, 0])
    lon = np.deg2rad(latlondepth[:, 1])
    return np.array([r * np.sin(colat) * np.cos(lon), r * np.sin(colat) * np.sin(lon), r * np.cos(colat)]).T


class GllMesh:
    """Element-nodal GLL mesh bundle: what the reference reads from a Salvus mesh for the GLL path
    (``mesh.points[mesh.connectivity]``, ``mesh.shape_order``, ``mesh.element_nodal_fields``;
    interpolator.py:954-976)."""

    def __init__(self, gll_points, shape_order, element_nodal_fields=None):
        self.gll_points = np.ascontiguousarray(gll_points, dtype=np.float64)   # [E, P, dim]
        self.shape_order = int(shape_order)
        self.element_nodal_fields = {k: np.ascontiguousarray(v, dtype=np.float64)
                                     for k, v in (element_nodal_fields or {}).items()}

    @property
    def nelem(self):
        return self.gll_points.shape[0]

    def get_element_centroid(self):
        # the reference takes the mean of the control nodes (salvus_mesh_reader.py:99-100)
        return self.gll_points.mean(axis=1)


def _mesh_points(mesh):
    return mesh.gll_points if isinstance(mesh, GllMesh) else mesh.points


def _gll_points_order(mesh):
    """(element-nodal points [E, P, dim], shape_order) of a :class:`GllMesh` or a Salvus mesh."""
    pts = np.asarray(_mesh_points(mesh))
    if pts.ndim != 3:
        raise ValueError(f"need element-nodal GLL points [E, P, dim] (points of shape {pts.shape})")
    return np.ascontiguousarray(pts, dtype=np.float64), int(mesh.shape_order)


def _element_fields(mesh, params, shape):
    """f64[C, E, P] from names of element-nodal fields or an array [C, E, P] / [E, P]."""
    if isinstance(params, str):
        params = [params]
    if isinstance(params, (list, tuple)) and all(isinstance(p, str) for p in params):
        if not params:
            return np.zeros((0,) + tuple(shape))
        fields = np.stack([np.asarray(mesh.element_nodal_fields[p], dtype=np.float64) for p in params])
    else:
        fields = np.asarray(params, dtype=np.float64)
        if fields.ndim == 2:
            fields = fields[None]
    if fields.ndim != 3 or fields.shape[1:] != tuple(shape):
        raise ValueError(f"params must name element-nodal fields or be an array [C, E, P] / [E, P] over {tuple(shape)}")
    return np.ascontiguousarray(fields)


def _mesh_fields(mesh, params):
    """(names, f64[C, E, P]) of the element-nodal fields ``params`` of a mesh (None: all of them)."""
    names = list(mesh.element_nodal_fields) if params is None else ([params] if isinstance(params, str) else list(params))
    pts = _mesh_points(mesh)
    return names, _element_fields(mesh, names, np.shape(pts)[:2])


def _report_not_found(nfailed):
    if nfailed > 0:
        print(nfailed, "points could not find an enclosing element. These points will be set to zero. "
                       "Please check your domain or the interpolation tuning parameters")


def _scatter_back(vals, inv, shape):
    """Values per unique point [U, C] scattered back through the inverse index -> f64 of ``shape`` = (C, E_t, P_t)."""
    return np.ascontiguousarray(vals[inv].T).reshape(shape)


def _components_first(data):
    """The ``[E, C, P]`` layout of ``MODEL/data`` -> contiguous f64[C, E, P]."""
    return np.ascontiguousarray(np.asarray(data, dtype=np.float64).transpose(1, 0, 2))


def _order_from_point_count(npoints, dim):
    return int(round(npoints ** (1.0 / dim))) - 1
