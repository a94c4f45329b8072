"""Does this model fit this mesh?  The time step a model forces on its GLL mesh -- the least node spacing over the fastest
velocity, times a Courant number -- and the shortest period the mesh still resolves with it -- the element size over the
slowest velocity, times the elements wanted per wavelength -- element by element, on the GPU, in one pass over arrays that
need not leave HBM (include/multimesh_hip.h: mm_gll_resolution, mm_arg_extreme).  The check that belongs between putting a
3-D model on a mesh built for a 1-D one and handing both to a solver.  Imported explicitly
(``from multimesh_amd import resolution``); the reference has no counterpart.

An element's size is measured by its straight corner-to-corner edges: on a curved order-4 element that is the chord, not
the arc.  ``courant`` and ``elements_per_wavelength`` are conventions the caller can override, not measurements."""
from __future__ import annotations

import numpy as np

from .api._common import _element_fields, _gll_points_order, field_store, hex8_corners, name_list, named_fields
from .device import default_context
from .mesh import HexMesh

__all__ = ["element_sizes", "time_step", "resolved_period", "elements_per_wavelength", "check_model"]

#: the fields read as fast and slow velocities when none are named
FAST_NAMES = ("VP", "VPV", "VPH")
SLOW_NAMES = ("VS", "VSV", "VSH")


def _velocities(mesh, conn, shape, given, names, what):
    """f64[C, E, P] (or None) from names of the mesh's fields, an array, or None: those of ``names`` the mesh carries."""
    hex8 = conn is not None
    if given is None or isinstance(given, str):
        given = name_list(given, [n for n in names if n in field_store(mesh)])
    if isinstance(given, (list, tuple)) and all(isinstance(g, str) for g in given):
        if not given:
            return None
        fields = named_fields(mesh, given)[1]
        return np.ascontiguousarray(fields[:, conn]) if hex8 else _element_fields(mesh, fields, shape)
    v = np.asarray(given, dtype=np.float64)
    if hex8 and v.shape[-1:] == (mesh.npoint,) and v.ndim in (1, 2):   # nodal values: gathered like the corners
        return np.ascontiguousarray(np.atleast_2d(v)[:, conn])
    if v.ndim == 2:
        v = v[None]
    if v.ndim != 3 or v.shape[1:] != tuple(shape) or v.shape[0] == 0:
        raise ValueError(f"{what} must name fields of the mesh or be an array [C, E, P] / [E, P] over {tuple(shape)}"
                         + (" (or nodal, [C, N] / [N])" if hex8 else ""))
    return np.ascontiguousarray(v)


def _mesh_arrays(mesh, fast, slow, need_fast):
    """(order, points f64[E, P, dim], fast f64[C, E, P] or None, slow or None).  A :class:`HexMesh` is an order-1 mesh:
    its corners, and its nodal fields, gathered through the connectivity in tensor order."""
    conn = None
    if isinstance(mesh, HexMesh):
        (conn, gp), order = hex8_corners(mesh), 1
    else:
        gp, order = _gll_points_order(mesh)
        if gp.shape[2] not in (2, 3) or order not in (1, 2, 4) or gp.shape[1] != (order + 1) ** gp.shape[2]:
            raise ValueError("GLL orders 1, 2 and 4 in 2-D or 3-D only")
    if not need_fast:
        return order, gp, None, None
    f = _velocities(mesh, conn, gp.shape[:2], fast, FAST_NAMES, "fast")
    if f is None:
        raise ValueError(f"no fast velocity: the mesh carries none of {FAST_NAMES}; name one or pass an array")
    return order, gp, f, _velocities(mesh, conn, gp.shape[:2], slow, SLOW_NAMES, "slow")


def _positive(value, name):
    value = float(value)
    if not (np.isfinite(value) and value > 0.0):
        raise ValueError(f"{name} must be positive and finite")
    return value


class _Pass:
    """One pass of the kernel over a mesh: the rows on the device, the counts, and the extremes asked of them."""

    def __init__(self, mesh, fast, slow, need_fast, context):
        order, gp, f, s = _mesh_arrays(mesh, fast, slow, need_fast)
        self.ctx = context or default_context()
        self.out, info = self.ctx.gll_resolution(order, gp, fast=f, slow=s)
        self.ngeometry, self.nmodel = (int(v) for v in info.numpy())

    def row(self, r):
        return self.out.rows(r, r + 1)

    def extreme(self, r, want_max):
        """(value, element) of row r: the least or greatest valid entry and the lowest element that holds it; NaN, -1."""
        value, index, _ = self.ctx.arg_extreme(self.row(r), want_max=want_max)
        return float(value.numpy()[0]), int(index.numpy()[0])


def element_sizes(mesh, context=None):
    """The sizes of every element of a :class:`GllMesh`, a Salvus mesh (orders 1, 2, 4; 2-D or 3-D) or a :class:`HexMesh`
    (order 1): ``(spacing, edge_min, edge_max, ninvalid)``, three f64[E] and a count.  ``spacing`` is the least distance
    between neighbouring GLL nodes of the element, ``edge_min`` and ``edge_max`` the least and greatest of its 12 (2-D: 4)
    corner-to-corner edges -- the chord, not the arc, where an element is curved.  An element with a coordinate that is
    not finite gets NaN and is counted in ``ninvalid``."""
    p = _Pass(mesh, None, None, False, context)
    rows = p.out.numpy()
    return rows[0], rows[1], rows[2], p.ngeometry


def time_step(mesh, fast=None, courant=0.6, context=None):
    """The time step a model forces on its mesh: ``(dt, element, step, ninvalid)`` with ``step[e] = min_p h[e][p] /
    vfast[e][p]`` (f64[E]; h the least distance of node p to its tensor-line neighbours, vfast the greatest of the fast
    velocities there), ``dt = courant * min_e step[e]`` and ``element`` the lowest element that sets it.  ``fast``: names
    of fields, an array [C, E, P] / [E, P], or None: those of VP, VPV, VPH the mesh carries (``ValueError`` when there is
    none).  ``courant`` is a convention the caller can override, not a measurement.  Elements with a coordinate or velocity
    that is not finite, or a fast velocity <= 0, get NaN, are left out of the minimum and are counted in ``ninvalid``."""
    courant = _positive(courant, "courant")
    p = _Pass(mesh, fast, (), True, context)
    least, element = p.extreme(3, False)
    return courant * least, element, p.row(3).numpy()[0], p.nmodel


def resolved_period(mesh, fast=None, slow=None, elements_per_wavelength=2.0, context=None):
    """The shortest period the mesh resolves with its model: ``(period, element, period_e)`` with ``period_e[e] =
    edge_max[e] / min_p vslow[e][p]`` (f64[E]), ``period = elements_per_wavelength * max_e period_e[e]`` and ``element`` the
    lowest element that sets it.  vslow is the least of the ``slow`` velocities above zero at the node, or the least
    ``fast`` one where there is none: a fluid element (VS = 0) is resolved by its P wavelength.  ``fast`` / ``slow``: names,
    arrays, or None (VP, VPV, VPH and VS, VSV, VSH as far as the mesh carries them).  ``elements_per_wavelength`` is a
    convention, not a measurement.  edge_max is the longest corner-to-corner chord.  Invalid elements get NaN."""
    per = _positive(elements_per_wavelength, "elements_per_wavelength")
    p = _Pass(mesh, fast, slow, True, context)
    greatest, element = p.extreme(4, True)
    return per * greatest, element, p.row(4).numpy()[0]


def elements_per_wavelength(mesh, period, fast=None, slow=None, minimum=2.0, context=None):
    """How many elements the shortest wavelength of ``period`` spans: ``(epw, least, element, nbelow)`` with ``epw[e] =
    period / period_e[e]`` (f64[E], ``period_e`` as in :func:`resolved_period`), its least value, the lowest element that
    has the greatest ``period_e`` (and so the least ``epw``), and the number of elements with ``epw < minimum``."""
    period = _positive(period, "period")
    p = _Pass(mesh, fast, slow, True, context)
    greatest, element = p.extreme(4, True)
    with np.errstate(divide="ignore", invalid="ignore"):
        epw = period / p.row(4).numpy()[0]
        return epw, period / greatest, element, int((epw < float(minimum)).sum())


class ModelCheck:
    """What :func:`check_model` found.  Per element, f64[E]: ``spacing``, ``edge_min``, ``edge_max``, ``step``,
    ``period_e`` and ``epw`` (elements per wavelength at ``period``).  The verdicts: ``dt`` and ``dt_element``;
    ``resolved_period`` and ``period_element``; ``least_epw``; ``nbelow``, the elements with fewer than
    ``elements_per_wavelength`` elements per wavelength at ``period``; ``ninvalid_geometry`` and ``ninvalid_model``."""

    def __init__(self, **values):
        self.__dict__.update(values)

    @property
    def ok(self):
        """No invalid element, and every element resolves ``period``."""
        return self.ninvalid_model == 0 and self.nbelow == 0

    def __str__(self):
        lines = [f"{len(self.step)} elements, {self.ninvalid_geometry} with invalid geometry, {self.ninvalid_model} invalid in all",
                 f"node spacing {np.nanmin(self.spacing) if len(self.spacing) else np.nan:.6g} .. "
                 f"{np.nanmax(self.spacing) if len(self.spacing) else np.nan:.6g}, longest edge "
                 f"{np.nanmax(self.edge_max) if len(self.edge_max) else np.nan:.6g}",
                 f"time step {self.dt:.6g} (courant {self.courant:g}), set by element {self.dt_element}",
                 f"resolved period {self.resolved_period:.6g} ({self.elements_per_wavelength:g} elements per wavelength), "
                 f"set by element {self.period_element}",
                 f"at period {self.period:g}: at least {self.least_epw:.4g} elements per wavelength, {self.nbelow} elements "
                 f"below {self.elements_per_wavelength:g}"]
        return "\n".join(lines)


def check_model(mesh, period, fast=None, slow=None, courant=0.6, elements_per_wavelength=2.0, context=None):
    """:func:`element_sizes`, :func:`time_step`, :func:`resolved_period` and :func:`elements_per_wavelength` (with
    ``minimum = elements_per_wavelength``) from ONE pass of the kernel over the mesh: a :class:`ModelCheck`, whose ``str``
    is a short report.  ``period`` is the shortest period the simulation is meant to carry."""
    period = _positive(period, "period")
    courant = _positive(courant, "courant")
    per = _positive(elements_per_wavelength, "elements_per_wavelength")
    p = _Pass(mesh, fast, slow, True, context)
    least_step, dt_element = p.extreme(3, False)
    greatest, period_element = p.extreme(4, True)
    rows = p.out.numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        epw = period / rows[4]
        return ModelCheck(spacing=rows[0], edge_min=rows[1], edge_max=rows[2], step=rows[3], period_e=rows[4], epw=epw,
                          dt=courant * least_step, dt_element=dt_element, resolved_period=per * greatest,
                          period_element=period_element, least_epw=period / greatest, nbelow=int((epw < per).sum()),
                          ninvalid_geometry=p.ngeometry, ninvalid_model=p.nmodel, period=period, courant=courant,
                          elements_per_wavelength=per)
