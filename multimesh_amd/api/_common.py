"""The constants, :class:`GllMesh`, how a mesh's points and fields are read and written -- the one place that answers "is
this a mesh, what are its points, which fields were named, where do results go" for every model tool -- and the steps
several modules share."""
import contextlib
import time

import numpy as np

from .. import io as mio
from ..mesh import HexMesh

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


def is_mesh(x):
    """A :class:`GllMesh`, a :class:`HexMesh`, a Salvus mesh (with or without its fields in memory) or any object with
    ``points`` and ``connectivity``; an array of points is not one."""
    return any(hasattr(x, a) for a in ("gll_points", "points", "element_nodal_fields"))


def points_of(mesh_or_points):
    """Host f64[..., dim], contiguous: the points of a mesh, or the array itself.  What shape a tool takes is its own check."""
    pts = _mesh_points(mesh_or_points) if is_mesh(mesh_or_points) else mesh_or_points
    return np.ascontiguousarray(pts, dtype=np.float64)


def name_list(params, default):
    """The names a caller gave: None is ``default``, a string is one name, anything else the list of them."""
    return list(default) if params is None else ([params] if isinstance(params, str) else list(params))


def field_store(mesh):
    """name -> per-node values: ``nodal_fields`` of a :class:`HexMesh`, ``element_nodal_fields`` of every other mesh (none
    for a Salvus mesh read without them)."""
    return mesh.nodal_fields if isinstance(mesh, HexMesh) else getattr(mesh, "element_nodal_fields", {})


def require_fields(mesh, names):
    """The mesh's :func:`field_store`; ``ValueError`` naming those of ``names`` it does not hold."""
    store = field_store(mesh)
    missing = [p for p in names if p not in store]
    if missing:
        raise ValueError(f"the mesh has no field {missing}")
    return store


def named_fields(mesh, params=None, default=None):
    """``(names, f64[C, *lead])`` of the per-node fields ``params`` of a mesh (None: ``default``, or all it holds), over the
    leading shape of its points ([E, P]; a :class:`HexMesh`: [N]).  No names: f64[0, *lead]."""
    names = name_list(params, field_store(mesh) if default is None else default)
    store = require_fields(mesh, names)
    if not names:
        return names, np.zeros((0,) + np.shape(_mesh_points(mesh))[:-1])
    return names, np.ascontiguousarray(np.stack([np.asarray(store[p], dtype=np.float64) for p in names]))


#: a hex8 connectivity in exodus order -> tensor order (corner i + 2 j + 4 k)
EXODUS_TO_TENSOR = [0, 1, 3, 2, 4, 5, 7, 6]


def hex8_corners(mesh):
    """(connectivity int64[E, 8] in tensor order, corner points f64[E, 8, 3]) of a :class:`HexMesh`: the order-1 GLL mesh
    it is."""
    if mesh.points.shape[1] != 3 or mesh.connectivity.shape[1] != 8:
        raise ValueError("3-D hexahedral meshes only")
    conn = np.ascontiguousarray(mesh.connectivity[:, EXODUS_TO_TENSOR])
    return conn, np.ascontiguousarray(mesh.points[conn])


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
    names, fields = named_fields(mesh, params)
    return names, _element_fields(mesh, fields, np.shape(_mesh_points(mesh))[:2])


class ImportTarget:
    """The mesh a model is imported onto, open for the length of a ``with`` block: a :class:`GllMesh` (a new contiguous
    f64[E, P] array is bound per name), a :class:`HexMesh` (``attach_field``) or a writable Salvus model -- an h5py-like
    object or a path, opened once, for update: only the named columns of its model data are assigned.  ``points``: host
    f64[..., dim]; ``lead``: their leading shape, the shape of one field."""

    def __init__(self, mesh):
        self.mesh, self._model = mesh, None

    def __enter__(self):
        with contextlib.ExitStack() as stack:
            if isinstance(self.mesh, (GllMesh, HexMesh)):
                self.points = np.asarray(_mesh_points(self.mesh))
            else:
                f = stack.enter_context(mio.open_h5(self.mesh, "r+"))
                self._model = f["MODEL/data"]
                self._labels = mio.dimension_labels(self._model, 1)
                self.points = np.array(f["MODEL/coordinates"][()], dtype=np.float64)
                if self.points.ndim != 3:
                    raise ValueError(f"MODEL/coordinates must be [nelem, P, dim], got {self.points.shape}")
            self._close = stack.pop_all().close
        self.lead = tuple(self.points.shape[:-1])
        return self

    def __exit__(self, *exc):
        self._close()

    def _column(self, name):
        return self._model[:, self._labels.index(name), :]

    def require(self, names, values=False):
        """``ValueError``, before anything runs or is written, unless the target can take ``names``: a model file needs a
        column for each; a mesh, whose fields are created, needs them only when their ``values`` are read (keep, blend)."""
        if self._model is None:
            if values:
                require_fields(self.mesh, names)
        elif unknown := [p for p in names if p not in self._labels]:
            raise ValueError(f"parameters {unknown} are not in MODEL/data (it holds {self._labels})")

    def existing(self, names):
        """f64[C, *lead]: what the target holds for ``names`` now."""
        if self._model is None:
            return named_fields(self.mesh, list(names))[1].reshape((len(names),) + self.lead)
        return np.array([self._column(p) for p in names], dtype=np.float64).reshape((len(names),) + self.lead)

    def sphere_mesh(self):
        """What ``map_to_sphere`` reads of the target, for sampling on its 1-D sphere: the mesh itself, or the file's
        coordinates with its ``z_node_1D`` column."""
        if self._model is None:
            return self.mesh
        if "z_node_1D" not in self._labels:
            raise ValueError("make_spherical needs the model's z_node_1D, which MODEL/data does not hold")
        order = _order_from_point_count(self.points.shape[1], 3)
        return GllMesh(self.points, order, {"z_node_1D": np.array(self._column("z_node_1D"), dtype=np.float64)})

    def write(self, names, values):
        """values f64[C, *lead] become the fields ``names`` of the target; nothing else of it changes."""
        for p, v in zip(names, values):
            if self._model is not None:
                self._model[:, self._labels.index(p), :] = v
            elif isinstance(self.mesh, HexMesh):
                self.mesh.attach_field(p, v)
            else:
                self.mesh.element_nodal_fields[p] = np.ascontiguousarray(v)


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
