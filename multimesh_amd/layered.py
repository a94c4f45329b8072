"""Layered column models: on a latitude x longitude map the depths of a stack of interfaces (topography, sediment bottoms,
Conrad, Moho, ...) and one value per layer and parameter, evaluated on the nodes of a mesh or on points on the GPU
(include/multimesh_layered.h: ``mm_layered_model_apply``; the header holds the statement, operation by operation, which the
device reproduces bit for bit).  Imported explicitly (``from multimesh_amd import layered``); the reference has no
counterpart.

This is the form crustal models are distributed in.  Evaluating it directly avoids rasterising it into a
latitude x longitude x depth cube (:func:`multimesh_amd.api.import_regular_grid`), which smears every interface over one
depth cell, and it tells for every node which layer it lies in, so "crust from one model, mantle from another" can be
expressed: :func:`import_layered_model` with ``outside="keep"`` after :func:`multimesh_amd.harmonics.import_harmonic_model`.
Geometry is ``mm_sample_grid``'s: ``z`` is the pole, latitude is geocentric, longitude runs from ``x`` towards ``y``, depth is
``6371000 - |p|``.  There is NO reader for any external file format here: the caller brings the model as arrays.

The symbol is an extension of the library's C ABI with a header of its own: this module keeps its signature table and
applies it to the handle of :func:`multimesh_amd.helpers.load_lib` on first use; the call itself goes through
:func:`multimesh_amd.device._call` and the :class:`Context` checks like every other call of the package."""
from __future__ import annotations

import numpy as np

from . import device as _device
from .api._common import ImportTarget, name_list, points_of
from .api.grids import RegularGrid, prepare_regular_grid
from .device import default_context
from .helpers import f64, i32, i64, load_lib, vp

__all__ = ["LayeredModel", "layered_model_apply", "evaluate_layered_model", "layer_index", "import_layered_model",
           "LATERAL", "PICK", "OUTSIDE"]

MAX_P = 256     # MM_LAYERED_MAX_P
MAX_NB = 256    # MM_LAYERED_MAX_NB
#: names -> their numbers in the C ABI (MM_LAYERED_LATERAL_*, _PICK_*, _OUTSIDE_*)
LATERAL = {"cell": 0, "bilinear": 1}
PICK = {"node": 0, "element": 1}
OUTSIDE = {"fill": 0, "clamp": 1, "keep": 2}

#: name -> (restype, argtypes) of the function include/multimesh_layered.h declares (tests/test_layered.py compares it with
#: the header); it is not part of helpers.SIGNATURES, the table of include/multimesh_hip.h
SIGNATURES = {
    "mm_layered_model_apply": (i32, (vp, vp, i64, i64, vp, i32, vp, i32, i32, vp, i32, vp, i64, i32, i32, i32, f64,
                                     vp, vp, vp, vp, vp)),
}


def bind(lib=None):
    """The library handle with :data:`SIGNATURES` applied (once)."""
    lib = lib or load_lib()
    if getattr(lib, "_layered_bound", False) is not True:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        lib._layered_bound = True
    return lib


def _number(table, key, what):
    if key not in table:
        raise ValueError(f"{what} must be one of {list(table)}, got {key!r}")
    return table[key]


_BOUNDS = "\0bounds"     # the name the interfaces travel under through prepare_regular_grid (no parameter can have it)


class LayeredModel:
    """A layered column model on a latitude x longitude map.

    ``lat`` f64[nlat], ``lon`` f64[nlon]: degrees, finite and strictly monotone (either way).  ``bounds`` f64[nb, nlat, nlon]:
    the depths of the interfaces in metres, positive down from 6 371 000 m (a negative value lies above that radius), top
    first, finite and nowhere decreasing downwards; two equal bounds are a layer of zero thickness, which no node lies in.
    ``values``: name -> f64[nlayer, nlat, nlon], ``nlayer = nb - 1``.  ``layer_names``: nlayer names, for the caller's use.
    ``lon_periodic``: None detects a global longitude axis as :func:`multimesh_amd.api.prepare_regular_grid` does.

    The axes are prepared by that function -- descending axes are flipped with their data, a global longitude axis is
    closed by the column ``lon[0] + 360`` -- so this is stated once; ``lat``, ``lon``, ``bounds`` and ``values`` hold the
    prepared model, ``flipped`` (axis name -> bool), ``appended`` (whether a closing column was added) and ``periodic`` what
    was done.  ``ValueError`` for what is refused."""

    def __init__(self, lat, lon, bounds, values, layer_names=None, lon_periodic=None):
        bounds = np.asarray(bounds, dtype=np.float64)
        if bounds.ndim != 3 or bounds.shape[1:] != (np.size(lat), np.size(lon)) or not 2 <= bounds.shape[0] <= MAX_NB:
            raise ValueError(f"bounds must be [nb, {np.size(lat)}, {np.size(lon)}] with 2 <= nb <= {MAX_NB}, got {bounds.shape}")
        nb = bounds.shape[0]
        if not np.isfinite(bounds).all():
            raise ValueError("the bounds must be finite")
        if (np.diff(bounds, axis=0) < 0).any():
            raise ValueError("the bounds decrease downwards somewhere: every interface must lie at or below the one above it")
        fields = {}
        for name, v in dict(values).items():
            v = np.asarray(v, dtype=np.float64)
            if v.shape != (nb - 1,) + bounds.shape[1:]:
                raise ValueError(f"values[{name!r}] must be {(nb - 1,) + bounds.shape[1:]} ([layer][lat][lon]), got {v.shape}")
            fields[name] = np.concatenate([v, v[-1:]])          # (padded to nb rows: one shape through the preparation)
        if layer_names is not None and len(layer_names) != nb - 1:
            raise ValueError(f"layer_names must name the {nb - 1} layers, got {len(layer_names)}")
        self.layer_names = None if layer_names is None else list(layer_names)
        lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        grid = RegularGrid(np.arange(nb, dtype=np.float64), lat, lon, {_BOUNDS: bounds, **fields})
        _, self.lat, self.lon, data, names, self.periodic = prepare_regular_grid(grid, lon_periodic=lon_periodic)
        self.flipped = {"latitude": bool(lat.size > 1 and lat[0] > lat[-1]), "longitude": bool(lon.size > 1 and lon[0] > lon[-1])}
        self.appended = data.shape[-1] != lon.size
        self.bounds = np.ascontiguousarray(data[0])
        self.values = {p: np.ascontiguousarray(data[k][:-1]) for k, p in enumerate(names) if k > 0}

    @classmethod
    def from_thickness(cls, lat, lon, top, thickness, values, layer_names=None, lon_periodic=None):
        """A model from the depth of its top ``top`` f64[nlat, nlon] and the thicknesses ``thickness`` f64[nlayer, nlat, nlon]
        (metres, not negative): ``bounds[0] = top``, ``bounds[1:] = top + np.cumsum(thickness, axis=0)``, in that order."""
        top, thickness = np.asarray(top, dtype=np.float64), np.asarray(thickness, dtype=np.float64)
        if thickness.ndim != 3 or thickness.shape[1:] != top.shape:
            raise ValueError(f"thickness must be [nlayer, nlat, nlon] over top {top.shape}, got {thickness.shape}")
        if not (thickness >= 0).all():
            raise ValueError("a thickness is negative or not a number")
        return cls(lat, lon, np.concatenate([top[None], top[None] + np.cumsum(thickness, axis=0)]), values, layer_names,
                   lon_periodic)

    @property
    def nb(self):
        return self.bounds.shape[0]

    @property
    def nlayer(self):
        return self.bounds.shape[0] - 1

    @property
    def parameters(self):
        return list(self.values)

    def names(self, params=None):
        names = name_list(params, self.parameters)
        if missing := [p for p in names if p not in self.values]:
            raise ValueError(f"the layered model has no {missing} (it has {self.parameters})")
        return names

    def packed(self, params=None):
        """(names, bounds f64[nlat, nlon, nb], values f64[nlat, nlon, nlayer, C]): the two column-major tables of ``params``
        (default: all) as the device reads them -- the column of a map node is one contiguous run."""
        names = self.names(params)
        shape = self.bounds.shape[1:]
        values = np.zeros(shape + (self.nlayer, len(names)))
        for c, p in enumerate(names):
            values[..., c] = self.values[p].transpose(1, 2, 0)
        return names, np.ascontiguousarray(self.bounds.transpose(1, 2, 0)), values

    def _like(self, values):
        new = object.__new__(LayeredModel)
        new.__dict__.update(self.__dict__)
        new.values = values
        return new

    def fill_empty_layers(self):
        """A model in which the values of a layer at the columns where it has zero thickness are replaced by the mean of the
        non-empty ones among the column's eight neighbours on the map, repeated -- filled columns count as non-empty in the
        next round -- until nothing changes or no empty column has such a neighbour (a layer that is empty everywhere stays as
        it is).  A longitude-periodic model wraps in longitude.  Grid-sized NumPy work on the host.

        Why: where a layer pinches out, ``lateral="bilinear"`` blends the values of the four columns around a node, the
        filler values of the empty ones among them included (see :func:`evaluate_layered_model`)."""
        thick = np.diff(self.bounds, axis=0) > 0                       # [nlayer, nlat, nlon]
        nlon = thick.shape[2]
        ring = self.periodic and nlon > 1                              # (the closing column repeats column 0)

        def neighbours(a, fill):
            """The eight shifted copies of a map a[nlat, nlon] (without its closing column), ``fill`` beyond its edge."""
            pad = np.pad(a, 1, mode="wrap") if ring else np.pad(a, 1, constant_values=fill)
            if ring:
                pad[0], pad[-1] = fill, fill
            n0, n1 = a.shape
            return [pad[1 + dj:1 + dj + n0, 1 + di:1 + di + n1] for dj in (-1, 0, 1) for di in (-1, 0, 1) if dj or di]

        values = {p: v.copy() for p, v in self.values.items()}
        for l in range(thick.shape[0]):
            known = (thick[l, :, :-1] if ring else thick[l]).copy()
            work = {p: (v[l, :, :-1] if ring else v[l]).copy() for p, v in values.items()}
            while not known.all():
                flags = neighbours(known, False)
                count = np.sum(flags, axis=0)
                take = ~known & (count > 0)
                if not take.any():
                    break
                for p, w in work.items():
                    total = np.sum([np.where(f, nb_, 0.0) for f, nb_ in zip(flags, neighbours(w, 0.0))], axis=0)
                    w[take] = total[take] / count[take]
                known = known | take
            for p, w in work.items():
                values[p][l] = np.concatenate([w, w[:, :1]], axis=1) if ring else w
        return self._like(values)


# ------------------------------------------------------------------------------------------------------------- the call
def layered_model_apply(ctx, points, lat, lon, bounds, values=None, lon_periodic=False, lateral="bilinear", pick="node",
                        outside="fill", fill_value=np.nan, out=None, want_layers=False, want_span=False,
                        want_latlondepth=False, noutside=None):
    """``mm_layered_model_apply`` on the context ``ctx``: points f64[G, P, 3] (P nodes per element, at most 256) or f64[N, 3]
    (P = 1); ``lat`` f64[nlat], ``lon`` f64[nlon] strictly ascending (a periodic ``lon`` closed at ``lon[0] + 360``: host axes
    are checked as :meth:`Context.sample_grid` checks them, device axes are the caller's word); ``bounds``
    f64[nlat, nlon, nb] and ``values`` f64[nlat, nlon, nlayer, C] (None: no components, layers only), the column-major
    tables of :meth:`LayeredModel.packed`.  ``lateral`` "bilinear" or "cell", ``pick`` "node" or "element", ``outside`` "fill",
    "clamp" or "keep" (``out``, which is then required, keeps the entries of outside nodes): include/multimesh_layered.h
    states each.  ``noutside``: int64[1] on the device, added to (not zeroed), or None.  Every array may be a host array, a
    :class:`DeviceArray` or a torch-like tensor on the GPU.  Returns a dict of device arrays: "out" f64[C, G, P] (or [C, N])
    and, as asked for, "layer" int32[G, P], "span" f64[G, P, 2], "latlondepth" f64[G, P, 3].  Runs on the context's stream and
    does not synchronise.  ``ValueError`` with the library's message for what it refuses.

    (A function of this module and not a method of :class:`Context`: the set of that class's public methods is pinned by the
    tests of the binding layer, as the set of functions of multimesh_hip.h is.)"""
    nlateral, npick, noutmode = _number(LATERAL, lateral, "lateral"), _number(PICK, pick, "pick"), _number(OUTSIDE, outside, "outside")
    lib = bind(ctx.lib)
    pts, ngroups, P = ctx._node_groups(points)
    _, la, lo = ctx._grid_axes(np.zeros(1), lat, lon, lon_periodic)
    b = ctx.asdevice(bounds, np.float64)
    if len(b.shape) != 3 or b.shape[:2] != (la.shape[0], lo.shape[0]) or not 2 <= b.shape[2] <= MAX_NB:
        raise ValueError(f"bounds must be [{la.shape[0]}, {lo.shape[0]}, nb] over the axes with 2 <= nb <= {MAX_NB}, got {b.shape}")
    nb = b.shape[2]
    v, ncomp = None, 0
    if values is not None:
        v = ctx.asdevice(values, np.float64)
        if len(v.shape) != 4 or v.shape[:3] != (la.shape[0], lo.shape[0], nb - 1):
            raise ValueError(f"values must be [{la.shape[0]}, {lo.shape[0]}, {nb - 1}, C], got {v.shape}")
        ncomp = v.shape[3]
    lead = pts.shape[:-1]
    if out is None and outside == "keep" and ncomp:
        raise ValueError('outside="keep" keeps the entries of out: pass out')
    if noutside is not None:
        noutside = ctx.asdevice(noutside, np.int64)
        if noutside.size != 1:
            raise ValueError("noutside must be int64[1]")
    out = ctx._out(out, (ncomp,) + lead, "out must hold one value per component and node", size_only=True)
    res = {"out": out, "layer": ctx._wanted(want_layers, lead, np.int32), "span": ctx._wanted(want_span, lead + (2,)),
           "latlondepth": ctx._wanted(want_latlondepth, lead + (3,))}
    _device._call(lib, "mm_layered_model_apply", ctx.handle, pts, ngroups, P, la, la.shape[0], lo, lo.shape[0],
                  int(bool(lon_periodic)), b, nb, v if ncomp else None, ncomp, nlateral, npick, noutmode, float(fill_value),
                  out if ncomp else None, res["layer"], res["span"], res["latlondepth"], noutside, arg_error=True)
    return {k: a for k, a in res.items() if a is not None}


def _points(mesh_or_points, who):
    pts = points_of(mesh_or_points)
    if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
        raise ValueError(f"{who} needs 3-D points [E, P, 3] or [N, 3], got {pts.shape}")
    return pts


def evaluate_layered_model(model: LayeredModel, mesh_or_points, params=None, lateral="bilinear", pick="node", outside="fill",
                           fill_value=np.nan, return_layers=False, context=None):
    """``model`` on the nodes of a mesh or on points: f64[C, E, P] for a :class:`GllMesh` or a Salvus mesh, f64[C, N] for the
    nodes of a :class:`HexMesh` or an [N, 3] array.  ``params``: names of the model (default: all).

    ``lateral``: "bilinear" interpolates the interface depths AND the values of the node's layer between the four map nodes
    around it; where a layer pinches out (zero thickness at some of the four columns), their values of that layer, which
    mean nothing there, are blended in at the layer's edge -- call :meth:`LayeredModel.fill_empty_layers` first.  "cell" reads
    the nearest map node's column unchanged: the model is piecewise constant around its map nodes.
    ``pick``: "node" finds the layer by the node's own depth; "element" by the depth of the centre of its element (points
    [E, P, 3]), so that on a mesh that honours an interface a node on it takes the side of its own element; the lateral
    position is the node's own either way.  ``outside``: "fill" (nodes outside the map, above the top or below the bottom get
    ``fill_value``) or "clamp" (the map's edge and the first and last layer extend).  With ``return_layers``:
    ``(values, layer int32[...], span f64[..., 2])`` -- the layer index (-1 outside) and its top and bottom depth at the node."""
    if outside == "keep":
        raise ValueError('outside="keep" needs values to keep: use import_layered_model, or layered_model_apply with out')
    names, bounds, values = model.packed(params)
    pts = _points(mesh_or_points, "evaluate_layered_model")
    ctx = context or default_context()
    res = layered_model_apply(ctx, pts, model.lat, model.lon, bounds, values, lon_periodic=model.periodic, lateral=lateral,
                              pick=pick, outside=outside, fill_value=fill_value, want_layers=return_layers,
                              want_span=return_layers)
    return (res["out"].numpy(), res["layer"].numpy(), res["span"].numpy()) if return_layers else res["out"].numpy()


def layer_index(model: LayeredModel, mesh_or_points, lateral="bilinear", pick="node", outside="fill", context=None):
    """Which layer of ``model`` every node lies in: ``(layer int32[...], span f64[..., 2])`` over the leading shape of the
    points -- the index (-1 outside) and the top and bottom depth of that layer at the node's column (NaN outside).  No
    values are read (``ncomp = 0``).  ``lateral``, ``pick``, ``outside`` ("fill" or "clamp") as :func:`evaluate_layered_model`."""
    if outside == "keep":
        raise ValueError('outside must be "fill" or "clamp" here: there are no values to keep')
    _, bounds, _ = model.packed([])
    pts = _points(mesh_or_points, "layer_index")
    ctx = context or default_context()
    res = layered_model_apply(ctx, pts, model.lat, model.lon, bounds, None, lon_periodic=model.periodic, lateral=lateral,
                              pick=pick, outside=outside, want_layers=True, want_span=True)
    return res["layer"].numpy(), res["span"].numpy()


def import_layered_model(model: LayeredModel, mesh, params=None, lateral="bilinear", pick="element", outside="keep",
                         fill_value=np.nan, context=None):
    """A layered model onto a mesh.  ``mesh``: a :class:`GllMesh` (``element_nodal_fields[p]`` becomes a new f64[E, P]
    array), a :class:`HexMesh` (nodal fields through ``attach_field``; its nodes belong to no single element: ``pick`` falls
    to the node's own depth) or a writable Salvus model -- an h5py-like object (:class:`multimesh_amd.io.MemoryH5`) or, with
    h5py, a path: the columns of ``MODEL/data`` that ``DIMENSION_LABELS`` names are overwritten in place, every other column
    stays as it is -- the targets of :func:`multimesh_amd.api.import_regular_grid`, through the same access.  ``params``:
    names of the model (default: all).  ``outside``: "keep" (default: nodes the model does not reach keep the mesh's value,
    bit for bit -- a crust laid over an existing model; the fields must exist, else ``ValueError``), "fill" or "clamp".
    ``lateral`` and ``pick`` as :func:`evaluate_layered_model`.  Returns the number of nodes the model did not reach."""
    _number(OUTSIDE, outside, "outside"), _number(LATERAL, lateral, "lateral"), _number(PICK, pick, "pick")
    names, bounds, values = model.packed(params)
    with ImportTarget(mesh) as target:
        pts = _points(target.points, "import_layered_model")
        target.require(names, values=outside == "keep")
        existing = target.existing(names) if outside == "keep" else None
        if not names:
            return 0
        ctx = context or default_context()
        count = ctx.zeros((1,), np.int64)
        res = layered_model_apply(ctx, pts, model.lat, model.lon, bounds, values, lon_periodic=model.periodic, lateral=lateral,
                                  pick=pick, outside=outside, fill_value=fill_value,
                                  out=None if existing is None else ctx.to_device(existing), noutside=count)
        target.write(names, res["out"].numpy().reshape((len(names),) + target.lead))
        return int(count.numpy()[0])
