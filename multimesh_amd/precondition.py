"""Kernel preconditioning: what stands between "sum the event kernels" and "smooth" when an FWI sensitivity kernel is
conditioned -- the cut-out around sources and receivers, exact quantiles of a field, clipping at a quantile of |K| -- on
the GPU, on arrays that need not leave HBM (include/multimesh_hip.h: mm_point_taper, mm_order_statistics, mm_clamp).
Imported explicitly (``from multimesh_amd import precondition``); the reference has no counterpart."""
from __future__ import annotations

import numpy as np

from .api._common import is_mesh, latlondepth_to_xyz, named_fields, points_of
from .device import default_context

__all__ = ["taper_around_points", "cut_around_points", "field_quantiles", "clip_fields", "precondition_kernel"]


def _points_of(mesh_or_points):
    """f64[E, P, 3] of a GLL mesh, f64[N, 3] of a HexMesh or of an array of points."""
    pts = points_of(mesh_or_points)
    if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
        raise ValueError(f"points must be [E, P, 3] or [N, 3], got {pts.shape}")
    if pts.ndim == 3 and not 1 <= pts.shape[1] <= 256:
        raise ValueError("an element has between 1 and 256 nodes")
    return pts


def _centres(centres, inner, outer, geocentric):
    """(centres f64[K, 3] in metres, inner f64[K], outer f64[K]), checked: ``ValueError`` for what mm_point_taper refuses."""
    c = np.asarray(centres, dtype=np.float64)
    c = c.reshape(0, 3) if c.size == 0 else np.atleast_2d(c)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"centres must be [K, 3], got {c.shape}")
    if len(c) > 1 << 20:
        raise ValueError("at most 2^20 centres")
    if geocentric:
        c = latlondepth_to_xyz(c) if len(c) else c
    if not np.isfinite(c).all():
        raise ValueError("a centre is not finite")
    radii = []
    for name, r in (("inner", inner), ("outer", outer)):
        if r is None:
            raise ValueError(f"{name} is required: no radius is invented")
        r = np.asarray(r, dtype=np.float64)
        if r.ndim == 0:
            r = np.full(len(c), float(r))
        if r.shape != (len(c),):
            raise ValueError(f"{name} must be a scalar or [K] = [{len(c)}], got {r.shape}")
        if not np.isfinite(r).all():
            raise ValueError(f"{name} is not finite")
        radii.append(np.ascontiguousarray(r))
    if (radii[0] < 0).any() or (radii[1] < radii[0]).any():
        raise ValueError("the radii need 0 <= inner <= outer")
    return np.ascontiguousarray(c), radii[0], radii[1]


def _values_of(values_or_mesh, params):
    """f64[C, ...] from a mesh and names of its fields, or from an array [C, ...] / [n] (one component)."""
    if is_mesh(values_or_mesh):
        return named_fields(values_or_mesh, params)[1]
    if params is not None:
        raise ValueError("params name the fields of a mesh: pass a mesh, or values without params")
    v = np.ascontiguousarray(values_or_mesh, dtype=np.float64)
    if v.ndim == 0:
        raise ValueError("values must be an array [C, ...] or [n]")
    return v[None] if v.ndim == 1 else v


def _check_q(q):
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or not 1 <= q.size <= 16:
        raise ValueError("between 1 and 16 quantiles per call")
    if not ((q >= 0.0) & (q <= 1.0)).all():
        raise ValueError("every quantile must lie in [0, 1]")
    return q


def taper_around_points(mesh_or_points, centres, inner, outer, geocentric=False, context=None):
    """The cut-out weight around ``centres``: at every node the least, over the centres, of ``0`` within ``inner``,
    ``1`` beyond ``outer`` and the smoothstep ``s*s*(3 - 2*s)``, ``s = (d - inner) / (outer - inner)``, between them.
    ``mesh_or_points``: a :class:`GllMesh` or Salvus mesh (-> f64[E, P]), a :class:`HexMesh` or points f64[N, 3]
    (-> f64[N]).  ``centres`` f64[K, 3] in metres, or (lat, lon, depth in m) with ``geocentric``; ``inner`` and ``outer``
    a scalar or f64[K], ``0 <= inner <= outer`` (``ValueError`` otherwise); ``outer == inner`` is a hard cut.  One
    streaming pass (``mm_point_taper``): elements far from every centre are skipped by an exact bounding-box test."""
    pts = _points_of(mesh_or_points)
    c, ri, ro = _centres(centres, inner, outer, geocentric)
    ctx = context or default_context()
    return ctx.point_taper(pts, c, ri, ro, want_weight=True)[2].numpy()


def cut_around_points(mesh, params, centres, inner, outer, geocentric=False, context=None):
    """The fields ``params`` of ``mesh`` times :func:`taper_around_points`' weight, in one pass: ``(values, ncut)`` with
    values f64[C, E, P] (a :class:`HexMesh`: [C, N]) -- new arrays, the mesh's fields are untouched -- and ``ncut`` the
    number of nodes whose weight is below 1.  Arguments as :func:`taper_around_points`."""
    pts = _points_of(mesh)
    _, fields = named_fields(mesh, params)
    c, ri, ro = _centres(centres, inner, outer, geocentric)
    ctx = context or default_context()
    out, ncut = ctx.point_taper(pts, c, ri, ro, values_in=fields.reshape(fields.shape[0], -1))
    return out.numpy().reshape(fields.shape), ncut


def _quantiles(ctx, values, q, method, absolute):
    """f64[C, m] on the host from device values [C, ...]: lower, higher, or the two combined for "linear"."""
    if method in ("lower", "higher"):
        return ctx.order_statistics(values, q, absolute=absolute, method=method)[0].numpy()
    lo, nvalid = ctx.order_statistics(values, q, absolute=absolute, method="lower")
    hi = ctx.order_statistics(values, q, absolute=absolute, method="higher")[0].numpy()
    lo, nvalid = lo.numpy(), nvalid.numpy()
    pos = q[None, :] * (nvalid[:, None] - 1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        mixed = lo + (hi - lo) * (pos - np.floor(pos))
    return np.where(hi == lo, lo, mixed)   # (equal neighbours, infinities among them: no inf - inf)


def field_quantiles(values_or_mesh, q, params=None, method="linear", absolute=False, context=None):
    """Exact quantiles of every field: f64[C, m] for ``q`` (a scalar or up to 16 values in [0, 1]) over values
    f64[C, ...] (or f64[n]: one field), or over the fields ``params`` of a mesh.  NaNs are left out; ``absolute``: of
    ``|v|``.  ``method``: ``"lower"`` / ``"higher"`` -- the value of rank ``floor`` / ``ceil`` of ``q * (nvalid - 1)``, an
    element of the data, by radix select on the device (``mm_order_statistics``: no sort, no copy to the host) -- or
    ``"linear"``: ``lo + (hi - lo) * (pos - floor(pos))`` formed on the host from the two, NumPy's default.  A field
    without a valid value gives NaN."""
    if method not in ("linear", "lower", "higher"):
        raise ValueError('method must be "linear", "lower" or "higher"')
    q = _check_q(q)
    values = _values_of(values_or_mesh, params)
    ctx = context or default_context()
    return _quantiles(ctx, ctx.to_device(values), q, method, absolute)


def _clip_on_device(ctx, values, quantile, lower, upper, symmetric):
    """(values, bounds f64[C] on the device or None, nclipped int64[C] on the device): ``values`` clipped IN PLACE."""
    ncomp = values.shape[0]
    if quantile is not None:
        bound = ctx.order_statistics(values, [quantile], absolute=True, method="higher")[0].reshape(ncomp)
        _, changed = ctx.clamp(values, upper=bound, symmetric=True, out=values)
        return values, bound, changed
    lo = None if lower is None else ctx.to_device(lower)
    hi = None if upper is None else ctx.to_device(upper)
    _, changed = ctx.clamp(values, lower=lo, upper=hi, symmetric=symmetric and lower is None, out=values)
    return values, hi if hi is not None else lo, changed


def _bounds(ncomp, quantile, lower, upper, symmetric):
    """The checked arguments of :func:`clip_fields`: (quantile or None, lower f64[C] or None, upper f64[C] or None)."""
    if quantile is not None:
        if lower is not None or upper is not None:
            raise ValueError("pass quantile, or lower / upper, not both")
        if not symmetric:
            raise ValueError("a quantile of |v| is a symmetric bound")
        return float(_check_q(quantile).reshape(1)[0]), None, None
    if lower is None and upper is None:
        raise ValueError("pass quantile, lower or upper")
    if symmetric and lower is not None:
        raise ValueError("symmetric takes upper alone (the lower bound is -upper): pass symmetric=False with lower")
    out = []
    for b in (lower, upper):
        if b is not None:
            b = np.asarray(b, dtype=np.float64)
            b = np.full(ncomp, float(b)) if b.ndim == 0 else np.ascontiguousarray(b)
            if b.shape != (ncomp,):
                raise ValueError(f"a bound is a scalar or one value per field [{ncomp}]")
        out.append(b)
    return None, out[0], out[1]


def clip_fields(values_or_mesh, params=None, quantile=None, lower=None, upper=None, symmetric=True, context=None):
    """Clip every field: ``(values, bounds f64[C], nclipped int64[C])``, values a new array of the input's shape
    ([C, ...]; [1, n] for f64[n]).  ``quantile`` q in [0, 1]: field c is clipped to ``[-b_c, b_c]`` with ``b_c`` the
    ``higher`` order statistic of ``|v|`` at q (0.999: the 99.9th percentile of |K|), which goes from the select to the
    clamp without leaving the device.  Or ``upper`` (and, with ``symmetric=False``, ``lower``): a scalar or f64[C];
    ``symmetric`` clips to ``[-upper, upper]``.  ``bounds`` is the upper bound (the lower one when only that is given).
    A NaN passes through and is not counted, -0.0 is kept."""
    values = _values_of(values_or_mesh, params)
    quantile, lower, upper = _bounds(values.shape[0], quantile, lower, upper, symmetric)
    ctx = context or default_context()
    out, bound, changed = _clip_on_device(ctx, ctx.to_device(values), quantile, lower, upper, symmetric)
    return out.numpy(), bound.numpy(), changed.numpy()


def _cut_list(name, points, cut):
    """(points [K, 3], inner, outer) of the sources or the receivers; a list needs its radii and the radii their list."""
    if points is None:
        if cut is not None:
            raise ValueError(f"{name}_cut without {name}s")
        return np.zeros((0, 3)), 0.0, 0.0
    if cut is None:
        raise ValueError(f"{name}s need {name}_cut=(inner, outer) in metres: no radius is invented as a default")
    if np.ndim(cut) != 1 or len(cut) != 2:
        raise ValueError(f"{name}_cut must be (inner, outer)")
    pts = np.asarray(points, dtype=np.float64)
    return (pts.reshape(0, 3) if pts.size == 0 else np.atleast_2d(pts)), float(cut[0]), float(cut[1])


def precondition_kernel(mesh, params, sources=None, receivers=None, source_cut=None, receiver_cut=None,
                        clip_quantile=None, geocentric=True, context=None):
    """The conditioning of a summed sensitivity kernel before it is smoothed, on the device from end to end: the fields
    ``params`` of ``mesh`` are damped to zero around ``sources`` and ``receivers`` (f64[S, 3], f64[R, 3]: (lat, lon, depth
    in m) with ``geocentric``, else metres) with ``source_cut`` / ``receiver_cut`` = (inner, outer) in metres -- each
    required when its list is given -- in ONE :func:`cut_around_points` pass over the S + R centres, then clipped at the
    ``clip_quantile`` of their absolute values (:func:`clip_fields`) when that is given.  Returns ``({name: f64[E, P]},
    report)`` (a :class:`HexMesh`: f64[N]) with ``report = {"ncut": int, "bound": {name: float or None}, "nclipped":
    {name: int}}``.  Bit for bit the composition of the three statements of include/multimesh_hip.h."""
    src, s_in, s_out = _cut_list("source", sources, source_cut)
    rec, r_in, r_out = _cut_list("receiver", receivers, receiver_cut)
    if src.ndim != 2 or src.shape[1] != 3 or rec.ndim != 2 or rec.shape[1] != 3:
        raise ValueError("sources and receivers must be [K, 3]")
    c, ri, ro = _centres(np.concatenate([src, rec]), np.concatenate([np.full(len(src), s_in), np.full(len(rec), r_in)]),
                         np.concatenate([np.full(len(src), s_out), np.full(len(rec), r_out)]), geocentric)
    if clip_quantile is not None:
        clip_quantile = float(_check_q(clip_quantile).reshape(1)[0])
    pts = _points_of(mesh)
    names, fields = named_fields(mesh, params)
    ctx = context or default_context()
    flat = ctx.to_device(fields.reshape(len(names), -1))
    out, ncut = ctx.point_taper(pts, c, ri, ro, values_in=flat, out=flat)
    report = {"ncut": ncut, "bound": dict.fromkeys(names), "nclipped": dict.fromkeys(names, 0)}
    if clip_quantile is not None and names:
        out, bound, changed = _clip_on_device(ctx, out.reshape(len(names), flat.shape[1]), clip_quantile, None, None, True)
        report["bound"] = dict(zip(names, (float(b) for b in bound.numpy())))
        report["nclipped"] = dict(zip(names, (int(n) for n in changed.numpy())))
    values = out.numpy().reshape(fields.shape)
    return dict(zip(names, values)), report
