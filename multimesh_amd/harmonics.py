"""Spherical-harmonic Earth models: ``f(r, theta, phi) = sum_lm c_lm(r) Y_lm(theta, phi)`` with the coefficients given per
radial knot, evaluated on the nodes of a mesh or on points on the GPU (include/multimesh_harmonics.h:
``mm_harmonic_model_apply``; the header holds the statement, operation by operation, which the device reproduces bit for
bit).  Imported explicitly (``from multimesh_amd import harmonics``); the reference has no counterpart.

This is the form global mantle models are distributed in.  Evaluating it directly avoids the detour over a
latitude x longitude x depth cube (:func:`multimesh_amd.api.import_regular_grid`), whose trilinear error the model does not have.
Geometry is ``mm_sample_grid``'s: ``z`` is the pole, latitude is geocentric, longitude runs from ``x`` towards ``y``.  The
device's convention is 4-pi-normalised real harmonics without the Condon-Shortley phase; :class:`SphericalHarmonicModel`
converts the others on the host (table-sized NumPy work).  There is NO reader for any external file format here: no sample
file of one was at hand to test a reader against, so the caller brings the coefficients as arrays.

The symbol is an extension of the library's C ABI with a header of its own: this module keeps its signature table and
applies it to the handle of :func:`multimesh_amd.helpers.load_lib` on first use; the call itself goes through
:func:`multimesh_amd.device._call` and the :class:`Context` checks like every other call of the package."""
from __future__ import annotations

import numpy as np

from . import device as _device
from .api._common import ImportTarget, name_list, points_of
from .api.radial import _radial_layers
from .device import default_context
from .helpers import i32, i64, load_lib, vp

__all__ = ["SphericalHarmonicModel", "evaluate_harmonic_model", "import_harmonic_model", "harmonic_model_apply",
           "convert_coefficients", "pack_coefficients", "unpack_coefficients", "coefficient_index", "coefficient_count",
           "NORMALIZATIONS", "MODES"]

MAX_LMAX = 255   # MM_HARMONIC_MAX_LMAX
MAX_P = 256      # MM_HARMONIC_MAX_P
#: mode name -> its number in the C ABI (MM_HARMONIC_REPLACE, _ADD, _RELATIVE)
MODES = {"replace": 0, "add": 1, "relative": 2}
NORMALIZATIONS = ("4pi", "ortho", "schmidt")

#: name -> (restype, argtypes) of the function include/multimesh_harmonics.h declares (tests/test_harmonics.py compares it
#: with the header); it is not part of helpers.SIGNATURES, the table of include/multimesh_hip.h
SIGNATURES = {
    "mm_harmonic_model_apply": (i32, (vp, vp, i64, i64, vp, i64, i32, vp, i64, i32, i32, vp, vp, vp)),
}


def bind(lib=None):
    """The library handle with :data:`SIGNATURES` applied (once)."""
    lib = lib or load_lib()
    if getattr(lib, "_harmonics_bound", False) is not True:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        lib._harmonics_bound = True
    return lib


# ------------------------------------------------------------------------------------------------ the coefficient layout
def _check_lmax(lmax):
    if isinstance(lmax, (bool, np.bool_)) or int(lmax) != lmax or not 0 <= int(lmax) <= MAX_LMAX:
        raise ValueError(f"lmax must be an integer in 0..{MAX_LMAX}, got {lmax!r}")
    return int(lmax)


def coefficient_count(lmax):
    """``NLM = (L + 1)(L + 2) / 2``: the (degree, order) pairs up to ``lmax``."""
    return (lmax + 1) * (lmax + 2) // 2


def coefficient_index(l, k, lmax):
    """``idx(l, k) = k (L + 1) - k (k - 1) / 2 + (l - k)``: the order is the major index, its degrees are contiguous."""
    return k * (lmax + 1) - k * (k - 1) // 2 + (l - k)


def pack_coefficients(cos, sin, lmax):
    """``cos``, ``sin`` f64[..., L+1, L+1] indexed ``[l][k]`` -> f64[..., 2, NLM]: plane 0 the cosine, plane 1 the sine
    coefficients at :func:`coefficient_index`.  Entries with ``k > l`` are not looked at; the sine of order 0 is packed as it
    is given (the device never reads it)."""
    cos, sin = np.asarray(cos, dtype=np.float64), np.asarray(sin, dtype=np.float64)
    out = np.zeros(cos.shape[:-2] + (2, coefficient_count(lmax)))
    for k in range(lmax + 1):
        base = coefficient_index(k, k, lmax)
        out[..., 0, base:base + lmax + 1 - k] = cos[..., k:lmax + 1, k]
        out[..., 1, base:base + lmax + 1 - k] = sin[..., k:lmax + 1, k]
    return out


def unpack_coefficients(packed, lmax):
    """The inverse of :func:`pack_coefficients`: f64[..., 2, NLM] -> (cos, sin) f64[..., L+1, L+1], zero where ``k > l``."""
    packed = np.asarray(packed, dtype=np.float64)
    cos = np.zeros(packed.shape[:-2] + (lmax + 1, lmax + 1))
    sin = np.zeros_like(cos)
    for k in range(lmax + 1):
        base = coefficient_index(k, k, lmax)
        cos[..., k:lmax + 1, k] = packed[..., 0, base:base + lmax + 1 - k]
        sin[..., k:lmax + 1, k] = packed[..., 1, base:base + lmax + 1 - k]
    return cos, sin


def _factors(lmax, normalization, csphase):
    """f64[L+1, L+1]: what a coefficient of the convention (``normalization``, ``csphase``) is multiplied by to become
    one of the device's (4-pi-normalised, no Condon-Shortley phase): with ``Y_conv = Y_4pi / n_l`` the same function has
    ``c_4pi = c_conv / n_l``, ``n_l = sqrt(4 pi)`` ("ortho": the integral of Y^2 is 1) or ``sqrt(2 l + 1)`` ("schmidt":
    4 pi / (2 l + 1)); ``csphase = -1`` (the convention includes the phase) flips the sign of the odd orders."""
    if normalization not in NORMALIZATIONS:
        raise ValueError(f"normalization must be one of {list(NORMALIZATIONS)}, got {normalization!r}")
    if csphase not in (1, -1):
        raise ValueError(f"csphase must be 1 (no Condon-Shortley phase) or -1 (with it), got {csphase!r}")
    l = np.arange(lmax + 1, dtype=np.float64)[:, None]
    k = np.arange(lmax + 1)[None, :]
    scale = {"4pi": np.ones_like(l), "ortho": np.full_like(l, 1.0 / np.sqrt(4.0 * np.pi)),
             "schmidt": 1.0 / np.sqrt(2.0 * l + 1.0)}[normalization]
    sign = np.where(k % 2 == 1, float(csphase), 1.0)
    return scale * sign


def convert_coefficients(cos, sin, lmax, frm=("4pi", 1), to=("4pi", 1)):
    """Coefficients ``[..., l, k]`` of one convention ``(normalization, csphase)`` as those of another, for the same
    function: multiplied by ``frm``'s factor, divided by ``to``'s (two roundings; a change of phase alone is exact)."""
    lmax = _check_lmax(lmax)
    f, t = _factors(lmax, *frm), _factors(lmax, *to)
    cos, sin = np.asarray(cos, dtype=np.float64), np.asarray(sin, dtype=np.float64)
    if cos.shape[-2:] != (lmax + 1, lmax + 1) or sin.shape != cos.shape:
        raise ValueError(f"cos and sin must be [..., {lmax + 1}, {lmax + 1}] ([l][k]), got {cos.shape} and {sin.shape}")
    return cos * f / t, sin * f / t


class SphericalHarmonicModel:
    """A model as spherical-harmonic coefficients per radial knot.

    ``radii`` f64[m], ascending; a REPEATED radius marks a discontinuity (the row before it is the lower side, the row
    after it the upper side), as in :class:`multimesh_amd.api.RadialModel`; between knots the coefficients are piecewise
    linear in the radius.  ``coefficients``: name -> ``(cos, sin)``, each f64[m, L+1, L+1] indexed ``[knot][l][k]`` (entries
    with ``k > l`` and the sine of order 0 are ignored).  ``normalization``: "4pi" (geodesy), "ortho" (orthonormal) or
    "schmidt" (semi-normalised); ``csphase``: 1 = without the Condon-Shortley phase, -1 = with it.  The coefficients are
    converted to the device's convention ("4pi", 1) here, on the host; ``cos`` / ``sin`` hold them per name.

    No reader for any external file format: there was no sample file to test one against."""

    def __init__(self, lmax, radii, coefficients, normalization="4pi", csphase=1):
        self.lmax = _check_lmax(lmax)
        self.normalization, self.csphase = normalization, csphase   # (what the coefficients were given in; kept for the adjoint)
        self.radii = np.ascontiguousarray(radii, dtype=np.float64)
        self.layers = _radial_layers(self.radii)
        shape = (self.radii.size, self.lmax + 1, self.lmax + 1)
        mask = np.tril(np.ones(shape[1:], dtype=bool))
        self.cos, self.sin = {}, {}
        for name, (c, s) in dict(coefficients).items():
            c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
            if c.shape != shape or s.shape != shape:
                raise ValueError(f"coefficients[{name!r}] must be two arrays {shape} ([knot][l][k]), got {c.shape} and {s.shape}")
            c, s = convert_coefficients(c, s, self.lmax, frm=(normalization, csphase))
            self.cos[name] = np.ascontiguousarray(np.where(mask, c, 0.0))
            self.sin[name] = np.ascontiguousarray(np.where(mask, s, 0.0))

    @classmethod
    def from_radial_basis(cls, lmax, basis, radii, coefficients, normalization="4pi", csphase=1):
        """A model whose radial dependence is an expansion in K basis functions (splines, say): ``basis`` f64[K, m], the
        functions tabulated at the knots ``radii`` f64[m]; ``coefficients``: name -> ``(cos, sin)``, each f64[K, L+1, L+1].
        The knot coefficients are the contraction ``sum_K basis[K][j] * c[K]`` (host, table-sized).  Between the knots the
        model is then piecewise linear: choose knots dense enough for the basis."""
        basis = np.asarray(basis, dtype=np.float64)
        if basis.ndim != 2 or basis.shape[1] != np.size(radii):
            raise ValueError(f"basis must be [K, m] over the m = {np.size(radii)} radii, got {basis.shape}")
        knots = {}
        for name, (c, s) in dict(coefficients).items():
            c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
            if c.shape[:1] != basis.shape[:1] or s.shape != c.shape or c.ndim != 3:
                raise ValueError(f"coefficients[{name!r}] must be two arrays [K = {basis.shape[0]}, L+1, L+1]")
            knots[name] = (np.tensordot(basis.T, c, axes=1), np.tensordot(basis.T, s, axes=1))
        return cls(lmax, radii, knots, normalization, csphase)

    @property
    def parameters(self):
        return list(self.cos)

    def names(self, params=None):
        names = name_list(params, self.parameters)
        if missing := [p for p in names if p not in self.cos]:
            raise ValueError(f"the harmonic model has no {missing} (it has {self.parameters})")
        return names

    def truncate(self, lmax):
        """The same model without the degrees above ``lmax``."""
        lmax = _check_lmax(lmax)
        if lmax > self.lmax:
            raise ValueError(f"cannot truncate a model of degree {self.lmax} to {lmax}")
        return SphericalHarmonicModel(lmax, self.radii, {p: (self.cos[p][:, :lmax + 1, :lmax + 1],
                                                             self.sin[p][:, :lmax + 1, :lmax + 1]) for p in self.cos})

    def packed(self, params=None):
        """(names, f64[C, m, 2, NLM]): the coefficients of ``params`` (default: all) as the device reads them."""
        names = self.names(params)
        if not names:
            return names, np.zeros((0, self.radii.size, 2, coefficient_count(self.lmax)))
        return names, np.ascontiguousarray(np.stack([pack_coefficients(self.cos[p], self.sin[p], self.lmax) for p in names]))


# ------------------------------------------------------------------------------------------------------------- the call
def harmonic_model_apply(ctx, points, radius, coef, lmax, mode=0, extend=False, values_in=None, out=None, noutside=None):
    """``mm_harmonic_model_apply`` on the context ``ctx``: points f64[G, P, 3] (P nodes per element, at most 256; the
    element's centre picks the layer) or f64[N, 3] (P = 1), radius f64[m], coef f64[C, m, 2, NLM] (or [m, 2, NLM]: one
    component) as :func:`pack_coefficients` lays them out.  ``mode`` 0: the model's value ``s``; with ``values_in``
    f64[C, G * P] (any shape of that size): 1 ``in + s``, 2 ``in + in * s``.  ``out`` may be ``values_in``.  ``extend``: radii
    outside the table are clamped; otherwise elements whose centre lies outside it get ``s = +0.0`` and their nodes are
    counted into ``noutside``, int64[1] on the device (added to, not zeroed), or None.  Every array may be a host array, a
    :class:`DeviceArray` or a torch-like tensor on the GPU.  Returns f64[C, G, P] (or [C, N]) on the device; runs on the
    context's stream and does not synchronise after its table check.  ``ValueError`` with the library's message for what it
    refuses.

    (A function of this module and not a method of :class:`Context`: the set of that class's public methods is pinned by the
    tests of the binding layer, as the set of functions of multimesh_hip.h is.)"""
    lib = bind(ctx.lib)
    lmax = _check_lmax(lmax)
    pts, ngroups, P = ctx._node_groups(points)
    r = ctx.asdevice(radius, np.float64)
    c = ctx.asdevice(coef, np.float64)
    nlm = coefficient_count(lmax)
    if len(r.shape) != 1 or len(c.shape) not in (3, 4) or c.shape[-3:] != (r.shape[0], 2, nlm):
        raise ValueError(f"radius must be [m] and coef [C, m, 2, {nlm}] (or [m, 2, {nlm}])")
    ncomp = c.shape[0] if len(c.shape) == 4 else 1
    if mode not in (0, 1, 2):
        raise ValueError("mode must be 0 .. 2")
    n = ngroups * P
    src = None
    if mode != 0:
        if values_in is None:
            raise ValueError("modes 1 and 2 need values_in")
        src = ctx.asdevice(values_in, np.float64)
        if src.size != ncomp * n:
            raise ValueError("values_in must hold one value per component and node")
    if noutside is not None:
        noutside = ctx.asdevice(noutside, np.int64)
        if noutside.size != 1:
            raise ValueError("noutside must be int64[1]")
    out = ctx._out(out, (ncomp,) + pts.shape[:-1], "out must hold one value per component and node", size_only=True)
    _device._call(lib, "mm_harmonic_model_apply", ctx.handle, pts, ngroups, P, r, r.shape[0], lmax, c, ncomp, int(mode),
                  int(bool(extend)), src, out, noutside, arg_error=True)
    return out


def _points(mesh_or_points, who):
    pts = points_of(mesh_or_points)
    if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
        raise ValueError(f"{who} needs 3-D points [E, P, 3] or [N, 3], got {pts.shape}")
    return pts


def evaluate_harmonic_model(model: SphericalHarmonicModel, mesh_or_points, params=None, extend=False, context=None):
    """``model`` on the nodes of a mesh or on points: f64[C, E, P] for a :class:`GllMesh` or a Salvus mesh (every element
    reads the layer its centre lies in, so a node on a discontinuity takes the side of its own element), f64[C, N] for the
    nodes of a :class:`HexMesh` or an [N, 3] array (a point on a discontinuity takes the upper side).  ``params``: names of
    the model (default: all).  ``extend``: False gives 0.0 in elements whose centre lies outside the model's radii, True
    extends the first and the last knot."""
    names, coef = model.packed(params)
    pts = _points(mesh_or_points, "evaluate_harmonic_model")
    ctx = context or default_context()
    return harmonic_model_apply(ctx, pts, model.radii, coef, model.lmax, extend=extend).numpy()


def import_harmonic_model(model: SphericalHarmonicModel, mesh, params=None, mode="replace", extend=False, context=None):
    """A harmonic model onto a mesh.  ``mesh``: a :class:`GllMesh` (``element_nodal_fields[p]`` becomes a new f64[E, P]
    array), a :class:`HexMesh` (nodal fields through ``attach_field``) or a writable Salvus model -- an h5py-like object
    (:class:`multimesh_amd.io.MemoryH5`) or, with h5py, a path: the columns of ``MODEL/data`` that ``DIMENSION_LABELS`` names
    are overwritten in place, every other column stays as it is -- the targets of
    :func:`multimesh_amd.api.import_regular_grid`, through the same access.  ``params``: names of the model (default: all).
    ``mode``: "replace" (the field is the model's value ``s``), "add" (``field + s``) or "relative" (``field + field * s``:
    ``s`` is a relative perturbation such as dlnVs of the mesh's own value); the last two need the field to exist.
    ``extend`` as :func:`evaluate_harmonic_model`.  Returns the number of nodes in elements outside the model's radii
    (0 with ``extend``)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {list(MODES)}, got {mode!r}")
    names, coef = model.packed(params)
    with ImportTarget(mesh) as target:
        pts = _points(target.points, "import_harmonic_model")
        target.require(names, values=mode != "replace")
        existing = target.existing(names) if mode != "replace" else None
        if not names:
            return 0
        ctx = context or default_context()
        count = ctx.zeros((1,), np.int64)
        values = harmonic_model_apply(ctx, pts, model.radii, coef, model.lmax, mode=MODES[mode], extend=extend,
                                      values_in=existing, noutside=count)
        target.write(names, values.numpy().reshape((len(names),) + target.lead))
        return int(count.numpy()[0])
