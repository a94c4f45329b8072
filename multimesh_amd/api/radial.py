"""Radial 1-D profiles, reference models and perturbations.  A 1-D model is a table radius -> value whose repeated radii
mark discontinuities; the lateral mean of a model per depth shell is a mass-weighted sum per radial bin
(include/multimesh_hip.h: mm_radial_bins, mm_binned_weighted_sum, mm_radial_model_apply).  The reference has no
counterpart."""
from __future__ import annotations

import numpy as np

from ..device import default_context
from ..mesh import HexMesh
from ._common import name_list, named_fields, points_of
from .mass import _device_mass, _hex8_mass


def _radial_layers(radius):
    """The rows [a, b] (inclusive) of every layer of a 1-D table: the maximal strictly ascending runs of ``radius``.
    ``ValueError`` for what ``mm_radial_model_apply`` refuses: a non-finite radius, a descending step, a run of one row."""
    r = np.asarray(radius, dtype=np.float64)
    if r.ndim != 1 or r.size < 2:
        raise ValueError("a radial model needs a 1-D radius of at least two rows")
    if not np.isfinite(r).all():
        raise ValueError("a radius of the table is not finite")
    step = np.diff(r)
    if (step < 0).any():
        raise ValueError("the radii of the table descend (a repeated radius marks a discontinuity; nothing may go down)")
    starts = np.concatenate([[0], np.nonzero(step == 0)[0] + 1, [r.size]])
    if (np.diff(starts) < 2).any():
        raise ValueError("a layer of the table has a single row (three equal radii, or a discontinuity at either end)")
    return [(int(a), int(b) - 1) for a, b in zip(starts[:-1], starts[1:])]


class RadialModel:
    """A 1-D reference model: ``radius`` f64[m] (m, ascending; a REPEATED radius marks a discontinuity, the row before it
    is the lower side, the row after it the upper side) and ``values`` {name: f64[m]}.  ``layers``: the rows (a, b),
    inclusive, of every maximal strictly ascending run."""

    def __init__(self, radius, values):
        self.radius = np.ascontiguousarray(radius, dtype=np.float64)
        self.layers = _radial_layers(self.radius)
        self.values = {}
        for name, v in dict(values).items():
            v = np.ascontiguousarray(v, dtype=np.float64)
            if v.shape != self.radius.shape:
                raise ValueError(f"values[{name!r}] must have the shape of radius {self.radius.shape}, got {v.shape}")
            self.values[name] = v

    @classmethod
    def from_arrays(cls, radius, values, names):
        """``values`` f64[C, m] (or [m] with one name) and the C names of its rows."""
        v = np.atleast_2d(np.asarray(values, dtype=np.float64))
        names = name_list(names, ())
        if v.shape[0] != len(names):
            raise ValueError(f"{len(names)} names for {v.shape[0]} rows of values")
        return cls(radius, dict(zip(names, v)))

    @property
    def parameters(self):
        return list(self.values)

    def table(self, params=None):
        """f64[C, m]: the rows of ``params`` (default: all, in the order given)."""
        names = name_list(params, self.parameters)
        missing = [p for p in names if p not in self.values]
        if missing:
            raise ValueError(f"the radial model has no {missing} (it has {self.parameters})")
        return names, np.ascontiguousarray(np.stack([self.values[p] for p in names])) if names else np.zeros((0, self.radius.size))


class RadialProfile:
    """What :func:`radial_profile` returns: ``edges`` f64[nbins + 1], ``centres`` f64[nbins], ``volume`` f64[nbins]
    (the mass per bin), ``count`` int64[nbins] (nodes per bin), ``noutside`` (nodes outside the edges), and per parameter
    ``mean[name]`` = sum(m f) / sum(m) and ``rms[name]`` = sqrt(sum(m f^2) / sum(m)), f64[nbins], NaN for an empty bin."""

    def __init__(self, edges, volume, count, noutside, mean, rms):
        self.edges = np.asarray(edges, dtype=np.float64)
        self.centres = 0.5 * (self.edges[:-1] + self.edges[1:])
        self.volume = np.asarray(volume, dtype=np.float64)
        self.count = np.asarray(count, dtype=np.int64)
        self.noutside = int(noutside)
        self.mean = dict(mean)
        self.rms = dict(rms)

    def to_radial_model(self):
        """The means as a :class:`RadialModel`: piecewise linear through the centres of the non-empty bins, no
        discontinuities (constant beyond the first and the last centre).  Needs two non-empty bins."""
        full = self.count > 0
        if full.sum() < 2:
            raise ValueError("a radial model needs at least two non-empty bins")
        return RadialModel(self.centres[full], {name: v[full] for name, v in self.mean.items()})


def radial_edges(points, nbins):
    """``nbins`` equal shells between the least and the greatest radius of ``points`` f64[..., 3]: f64[nbins + 1] whose
    first and last entries ARE those radii, computed as the device computes them (sqrt((x*x + y*y) + z*z)), so that every
    finite point falls in a bin."""
    nbins = int(nbins)
    if nbins < 1:
        raise ValueError("nbins must be at least 1")
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    r = r[np.isfinite(r)]
    if r.size == 0 or not r.max() > r.min():
        raise ValueError("the points span no range of radii: pass edges")
    return np.linspace(r.min(), r.max(), nbins + 1)


def _radial_mesh(mesh, params):
    """(points [E, P, 3] or [N, 3], names, fields [C, ...] or None, is_hex) of a GllMesh / Salvus mesh or a HexMesh."""
    pts = points_of(mesh)
    if not isinstance(mesh, HexMesh) and pts.ndim != 3:
        raise ValueError(f"need a HexMesh or element-nodal GLL points [E, P, 3] (points of shape {pts.shape})")
    if pts.shape[-1] != 3:
        raise ValueError(f"radial profiles are for 3-D meshes (points of shape {pts.shape})")
    names, fields = named_fields(mesh, params, default=())
    return pts, names, fields, isinstance(mesh, HexMesh)


def radial_profile(mesh, params=None, edges=None, nbins=None, context=None):
    """The lateral mean and rms of every parameter of ``params`` per radial bin, the volume and the node count per bin:
    a :class:`RadialProfile`.  ``mesh``: a :class:`GllMesh` or a Salvus mesh (the mass is :func:`gll_mass_matrix`'s, on
    the device, the values element-nodal) or a :class:`HexMesh` (:func:`hex8_mass_matrix`'s lumped mass, nodal values).
    ``edges`` f64[nbins + 1], strictly ascending, or ``nbins`` (default 64) equal shells between the mesh's least and
    greatest node radius (:func:`radial_edges`); not both.  ``edges[b] <= r < edges[b + 1]``, the last edge belongs to the
    last bin.  One pass over the mesh per parameter and moment, for all bins together, in the fixed order
    ``mm_binned_weighted_sum`` states: the same bits on every run.

    Radii are geometric, ``|p|``.  On an elliptic mesh with topography a shell of constant ``|p|`` cuts through the 1-D
    layers: map the mesh with :func:`map_to_sphere` first to bin by 1-D radius."""
    if edges is not None and nbins is not None:
        raise ValueError("pass edges or nbins, not both")
    pts, names, fields, is_hex = _radial_mesh(mesh, params)
    if edges is None:
        edges = radial_edges(pts, 64 if nbins is None else nbins)
    else:
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        if edges.ndim != 1 or edges.size < 2 or not np.isfinite(edges).all() or not (np.diff(edges) > 0).all():
            raise ValueError("edges must be 1-D, finite and strictly ascending, with at least two entries")
    nb = edges.size - 1
    ctx = context or default_context()
    mass = _hex8_mass(mesh, ctx) if is_hex else _device_mass(pts, int(mesh.shape_order), ctx)
    bins, noutside = ctx.radial_bins(pts, edges)
    volume, count = ctx.binned_weighted_sum(mass, bins, nb, want_count=True)
    volume = volume[0]
    mean, rms = {}, {}
    if names:
        f = ctx.to_device(fields.reshape(len(names), -1))
        m_flat = mass.reshape(mass.size)
        s1 = ctx.binned_weighted_sum(m_flat, bins, nb, f)
        s2 = ctx.binned_weighted_sum(m_flat, bins, nb, f, square=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            for c, name in enumerate(names):
                mean[name] = np.where(count > 0, s1[c] / volume, np.nan)
                rms[name] = np.where(count > 0, np.sqrt(s2[c] / volume), np.nan)
    return RadialProfile(edges, volume, count, noutside, mean, rms)


def evaluate_radial_model(model: RadialModel, mesh_or_points, params=None, context=None):
    """``model`` on the nodes of a mesh or on points: f64[C, E, P] for a :class:`GllMesh` (every element reads the layer
    its centre lies in, so a node on a discontinuity takes the side of its own element), f64[C, N] for the nodes of a
    :class:`HexMesh` or an [N, 3] array (a point on a discontinuity takes the upper side).  Piecewise linear within a
    layer, constant beyond the table's ends.  ``params``: names of the model (default: all)."""
    _, table = model.table(params)
    pts = points_of(mesh_or_points)
    if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
        raise ValueError(f"points must be [E, P, 3] or [N, 3], got {pts.shape}")
    ctx = context or default_context()
    return ctx.radial_model_apply(pts, model.radius, table).numpy()


def _perturbation(mesh, params, reference, mode, nbins, context):
    pts, names, fields, _ = _radial_mesh(mesh, params)
    if not names:
        raise ValueError("params must name at least one field")
    if not isinstance(reference, RadialModel):
        if not (isinstance(reference, str) and reference == "mean"):
            raise ValueError(f'reference must be a RadialModel or "mean", got {reference!r}')
        if mode in (3, 4):
            raise ValueError('from_perturbation needs the RadialModel the perturbation refers to: "mean" of a '
                             "perturbation is not its reference")
    ctx = context or default_context()
    if not isinstance(reference, RadialModel):
        reference = radial_profile(mesh, names, nbins=nbins, context=ctx).to_radial_model()
    _, table = reference.table(names)
    out = ctx.radial_model_apply(pts, reference.radius, table, mode=mode, values_in=fields.reshape(len(names), -1))
    return out.numpy().reshape(fields.shape)


def to_perturbation(mesh, params, reference, relative=True, nbins=None, context=None):
    """The fields ``params`` of a mesh as perturbations of a 1-D reference: ``(f - ref) / ref`` (``relative``; a
    fraction, not per cent) or ``f - ref``, f64[C, E, P] (a :class:`HexMesh`: [C, N]); new arrays, the mesh's fields
    are untouched.  ``reference``: a :class:`RadialModel`, or ``"mean"``: the mesh's own lateral mean, from
    :func:`radial_profile` with ``nbins`` passed through.  One fused pass (``mm_radial_model_apply`` modes 1 and 2)."""
    return _perturbation(mesh, params, reference, 2 if relative else 1, nbins, context)


def from_perturbation(mesh, params, reference, relative=True, nbins=None, context=None):
    """The inverse of :func:`to_perturbation`: the fields ``params`` of a mesh hold perturbations of the
    :class:`RadialModel` ``reference``; returns ``ref + f * ref`` (``relative``) or ``f + ref``.  ``"mean"`` is refused
    here: the mean of a perturbation is not the model it refers to."""
    return _perturbation(mesh, params, reference, 4 if relative else 3, nbins, context)
