"""The way back from a mesh to spherical-harmonic coefficients: the transpose ``H^T`` of the evaluation ``f = H c`` of
:mod:`multimesh_amd.harmonics` (include/multimesh_harmonic_adjoint.h: ``mm_harmonic_model_transpose``; the header holds the
statement, sum by sum, which the device reproduces bit for bit), the mass-weighted adjoint of a field on a mesh, the
least-squares expansion of a mesh field in spherical harmonics (CGLS over ``H`` and ``H^T``), and the power per degree.
Imported explicitly (``from multimesh_amd import harmonic_adjoint``); the reference has no counterpart.

The symbol has an extension header of its own: this module keeps its signature table and applies it to the handle of
:func:`multimesh_amd.helpers.load_lib` on first use; the call goes through :func:`multimesh_amd.device._call` and the
:class:`Context` checks like every other call of the package."""
from __future__ import annotations

import numpy as np

from . import device as _device
from .api._common import GllMesh, ImportTarget, _order_from_point_count, name_list
from .api.mass import gll_mass_matrix, hex8_mass_matrix
from .device import default_context
from .harmonics import (SphericalHarmonicModel, _check_lmax, _factors, _points, coefficient_count, harmonic_model_apply,
                        unpack_coefficients)
from .helpers import i32, i64, load_lib, vp
from .mesh import HexMesh

__all__ = ["harmonic_model_transpose", "harmonic_adjoint", "fit_harmonic_model", "degree_power", "SEGMENT_NODES"]

SEGMENT_NODES = 16384   # MM_HARMONIC_SEGMENT_NODES: the nodes of a segment of the stated order of the sums

#: name -> (restype, argtypes) of the function include/multimesh_harmonic_adjoint.h declares (tests/test_harmonic_adjoint.py
#: compares it with the header); part of neither helpers.SIGNATURES nor harmonics.SIGNATURES
SIGNATURES = {
    "mm_harmonic_model_transpose": (i32, (vp, vp, i64, i64, vp, i64, i32, vp, vp, i64, i32, vp, vp, i64)),
}


def bind(lib=None):
    """The library handle with :data:`SIGNATURES` applied (once)."""
    lib = lib or load_lib()
    if getattr(lib, "_harmonic_adjoint_bound", False) is not True:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        lib._harmonic_adjoint_bound = True
    return lib


# ------------------------------------------------------------------------------------------------------------- the call
def harmonic_model_transpose(ctx, points, radius, lmax, values, weight=None, extend=False, out=None, noutside=None,
                             scratch_limit=0):
    """``mm_harmonic_model_transpose`` on the context ``ctx``: points f64[G, P, 3] or f64[N, 3] (P = 1) and radius f64[m] as
    :func:`multimesh_amd.harmonics.harmonic_model_apply` takes them, ``values`` f64[C, G * P] (any shape of C rows; f64[G * P]
    or the shape of the points: one component), ``weight`` one value per node or None.  Returns ``H^T (weight * values)``,
    f64[C, m, 2, NLM] on the device in the layout of the coefficients (``out``: the caller's array of that size, overwritten).
    ``extend`` and ``noutside`` (int64[1] on the device, added to) as in the forward call: with ``extend`` off the nodes of
    elements outside the table take no part and are counted.  ``scratch_limit``: bytes the segment sums may take (0: the
    library's default, 1 GiB); the result does not depend on it.  Every array may be a host array, a :class:`DeviceArray` or a
    torch-like tensor on the GPU.  Runs on the context's stream and does not synchronise after its table check.
    ``ValueError`` with the library's message for what it refuses; a limit that order 0 of one component does not fit raises
    :class:`multimesh_amd.device.MultiMeshHipError` (MM_ERR_UNSUPPORTED)."""
    lib = bind(ctx.lib)
    lmax = _check_lmax(lmax)
    pts, ngroups, P = ctx._node_groups(points)
    r = ctx.asdevice(radius, np.float64)
    if len(r.shape) != 1:
        raise ValueError("radius must be [m]")
    n = ngroups * P
    v = ctx.asdevice(values, np.float64)
    if len(v.shape) == 0 or (n == 0 and len(v.shape) < 2):
        raise ValueError("values must be [C, G * P]")
    ncomp = 1 if v.shape == pts.shape[:-1] or len(v.shape) == 1 else v.shape[0]
    if v.size != ncomp * n:
        raise ValueError("values must hold one value per component and node")
    w = None
    if weight is not None:
        w = ctx.asdevice(weight, np.float64)
        if w.size != n:
            raise ValueError("weight must hold one value per node")
    if noutside is not None:
        noutside = ctx.asdevice(noutside, np.int64)
        if noutside.size != 1:
            raise ValueError("noutside must be int64[1]")
    if isinstance(scratch_limit, (bool, np.bool_)) or int(scratch_limit) != scratch_limit:
        raise ValueError("scratch_limit must be an integer number of bytes")
    out = ctx._out(out, (ncomp, r.shape[0], 2, coefficient_count(lmax)), "out must hold [C, m, 2, NLM] values", size_only=True)
    _device._call(lib, "mm_harmonic_model_transpose", ctx.handle, pts, ngroups, P, r, r.shape[0], lmax, w, v, ncomp,
                  int(bool(extend)), out, noutside, int(scratch_limit), arg_error=True)
    return out


def _node_mass(target, ctx):
    """The mass of every node of an open :class:`ImportTarget`: the GLL mass matrix, or the lumped mass of a hex8 mesh."""
    mesh = target.mesh
    if isinstance(mesh, HexMesh):
        return hex8_mass_matrix(mesh, context=ctx)
    if not isinstance(mesh, GllMesh):
        mesh = GllMesh(target.points, _order_from_point_count(target.points.shape[1], 3), {})
    return gll_mass_matrix(mesh, context=ctx)


def harmonic_adjoint(template: SphericalHarmonicModel, mesh, params=None, mass=True, extend=False, context=None):
    """Fields of a mesh brought onto the coefficients of a harmonic model: ``H^T (M o K)`` per field ``K`` of ``params``
    (default: all the mesh holds), ``M`` the mass matrix of the mesh (:func:`multimesh_amd.api.gll_mass_matrix`, for a
    :class:`HexMesh` :func:`multimesh_amd.api.hex8_mass_matrix`), or ``H^T K`` with ``mass=False``.  With ``K`` a sensitivity
    kernel this is the gradient of the misfit with respect to the coefficients ``c_lm(r)``.  ``template``: a
    :class:`SphericalHarmonicModel`; only its radii, ``lmax`` and the convention it was given in (``normalization``,
    ``csphase``) are read.  ``mesh``: a :class:`GllMesh`, a :class:`HexMesh` or a Salvus model (h5py-like object or path).
    The gradient is taken with respect to the coefficients in the template's convention: if ``c_device = s o c_user`` then
    ``d/dc_user = s o d/dc_device``, the same factor as for the coefficients, not its inverse.

    Returns ``(gradient, noutside)``: a :class:`SphericalHarmonicModel` of the template's radii and degree whose ``cos`` /
    ``sin`` hold the gradient per name as it is (a gradient is not a model: nothing converts it further, and it carries the
    default convention tag), and the number of nodes in elements outside the template's radii (0 with ``extend``), which
    took no part."""
    ctx = context or default_context()
    with ImportTarget(mesh) as target:
        pts = _points(target.points, "harmonic_adjoint")
        store = getattr(target.mesh, "nodal_fields", None) if isinstance(target.mesh, HexMesh) else \
            getattr(target.mesh, "element_nodal_fields", None)
        names = name_list(params, store if store is not None else target._labels)
        target.require(names, values=True)
        values = target.existing(names).reshape(len(names), -1) if names else np.zeros((0, pts[..., 0].size))
        weight = _node_mass(target, ctx).reshape(-1) if mass else None
    count = ctx.zeros((1,), np.int64)
    grad = harmonic_model_transpose(ctx, pts, template.radii, template.lmax, values, weight=weight, extend=extend,
                                    noutside=count).numpy()
    scale = _factors(template.lmax, template.normalization, template.csphase)
    coefficients = {}
    for p, g in zip(names, grad):
        cos, sin = unpack_coefficients(g, template.lmax)
        coefficients[p] = (cos * scale, sin * scale)
    return SphericalHarmonicModel(template.lmax, template.radii, coefficients), int(count.numpy()[0])


# -------------------------------------------------------------------------------------------------------------- the fit
def fit_harmonic_model(mesh_or_points, values_or_params, radius, lmax, mass=True, damping=0.0, rtol=1e-8, max_iter=200,
                       normalization="4pi", csphase=1, extend=False, context=None):
    """The least-squares expansion of fields on a mesh in spherical harmonics per radial knot:
    ``min |W^(1/2) (H c - f)|^2 + damping |c|^2`` by CGLS, ``H`` the evaluation
    (:func:`multimesh_amd.harmonics.harmonic_model_apply`), ``H^T`` :func:`harmonic_model_transpose`, ``W`` the mass matrix
    of the mesh (``mass=True``; ``mass`` may also be an array, one weight per node) or 1.  ``mesh_or_points``: a
    :class:`GllMesh` or :class:`HexMesh` with ``values_or_params`` the names of its fields (None: all), or points
    f64[G, P, 3] / f64[N, 3] with ``values_or_params`` f64[C, n] (``mass=True`` then needs a mesh).  ``radius`` f64[m] and
    ``lmax``: the knots and the degree of the expansion.  The unknowns are the device's coefficients (4-pi-normalised, no
    Condon-Shortley phase): the damping acts on them, whatever convention the result is reported in.

    The iteration runs on the device: the vectors are torch tensors on the context's GPU (on torch's current stream, which
    must be the context's: both are the default stream unless the caller chose otherwise), and one scalar per iteration is
    read back, the relative residual of the normal equations ``|H^T W (f - H c) - damping c| / |H^T W f|`` that the
    stopping rule ``<= rtol`` needs.  It stops after ``max_iter`` iterations at the latest and never raises for not
    converging: compare the returned residual with ``rtol``.  A rank-deficient problem (``lmax`` beyond what a regional
    chunk constrains, knots no node touches) with ``damping = 0`` returns the iterate CGLS has reached from zero, which
    converges to the minimum-norm solution.  With ``extend`` off the nodes of elements outside ``radius`` are no equations
    of the system (``H`` is zero there and ``H^T`` skips them).  The coordinates must be finite.

    Returns ``(model, iterations, residual, untouched)``: a :class:`SphericalHarmonicModel` (names ``values_or_params`` or
    "0", "1", ... for arrays; ``model.cos`` / ``model.sin`` hold the device's coefficients as every model does, and the model
    carries ``normalization`` / ``csphase`` as the convention it is to be reported in:
    :func:`multimesh_amd.harmonics.convert_coefficients` with ``to=(normalization, csphase)`` gives those numbers), the
    number of iterations, the final relative residual, and the knot rows no node touches, bool[m] (their coefficients stay
    0)."""
    import torch

    ctx = context or default_context()
    lmax = _check_lmax(lmax)
    _factors(lmax, normalization, csphase)   # (checks the two)
    radius = np.ascontiguousarray(radius, dtype=np.float64)
    if isinstance(mesh_or_points, (GllMesh, HexMesh)):
        with ImportTarget(mesh_or_points) as target:
            pts = _points(target.points, "fit_harmonic_model")
            store = target.mesh.nodal_fields if isinstance(target.mesh, HexMesh) else target.mesh.element_nodal_fields
            names = name_list(values_or_params, store)
            target.require(names, values=True)
            f = target.existing(names).reshape(len(names), -1)
            weight = _node_mass(target, ctx).reshape(-1) if mass is True else None
    else:
        pts = _points(mesh_or_points, "fit_harmonic_model")
        f = np.asarray(values_or_params, dtype=np.float64)
        f = f.reshape(1, -1) if f.ndim == 1 else f.reshape(f.shape[0], -1)
        names = [str(c) for c in range(f.shape[0])]
        if mass is True:
            raise ValueError("mass=True needs a mesh; pass the weights as an array, or mass=False")
        weight = None
    if mass is not True and mass is not False and mass is not None:
        weight = np.ascontiguousarray(mass, dtype=np.float64).reshape(-1)
    n = pts[..., 0].size
    if f.shape[1] != n or (weight is not None and weight.size != n):
        raise ValueError("values and weights must hold one value per node")
    if not damping >= 0.0:
        raise ValueError("damping must not be negative")
    device = torch.device("cuda", ctx.device)
    m, nlm, nc = radius.size, coefficient_count(lmax), f.shape[0]
    tp, tr = torch.from_numpy(pts).to(device), torch.from_numpy(radius).to(device)
    tf = torch.from_numpy(np.ascontiguousarray(f)).to(device)
    tw = None if weight is None else torch.from_numpy(weight).to(device)

    def forward(c, out):       # out = H c
        harmonic_model_apply(ctx, tp, tr, c, lmax, extend=extend, out=out)
        return out

    def transpose(r, out):     # out = H^T (W r)
        harmonic_model_transpose(ctx, tp, tr, lmax, r, weight=tw, extend=extend, out=out)
        return out

    # rows no node touches: the transpose of ones at degree 0 is the sum of the lerp weights per row
    ones = torch.ones((1, n), dtype=torch.float64, device=device)
    touched = torch.empty((1, m, 2, 1), dtype=torch.float64, device=device)
    harmonic_model_transpose(ctx, tp, tr, 0, ones, extend=extend, out=touched)
    untouched = (touched[0, :, 0, 0] == 0.0).cpu().numpy()

    x = torch.zeros((nc, m, 2, nlm), dtype=torch.float64, device=device)
    r = tf.clone()                                    # f - H x
    s = transpose(r, torch.empty_like(x))             # H^T W r - damping x
    p = s.clone()
    q = torch.empty_like(r)
    gamma = (s * s).sum()
    gamma0 = gamma.clone()
    iterations, residual = 0, 1.0
    if float(gamma0.item()) == 0.0:
        residual = 0.0
    else:
        while iterations < max_iter:
            forward(p, q)
            delta = (q * q * tw).sum() if tw is not None else (q * q).sum()
            if damping:
                delta = delta + damping * (p * p).sum()
            alpha = gamma / delta
            x += alpha * p
            r -= alpha * q
            transpose(r, s)
            if damping:
                s -= damping * x
            gamma_new = (s * s).sum()
            iterations += 1
            residual = float(torch.sqrt(gamma_new / gamma0).item())   # the one readback of the iteration
            if not residual > rtol:
                break
            p = s + (gamma_new / gamma) * p
            gamma = gamma_new
    packed = x.cpu().numpy()
    coefficients = {name: unpack_coefficients(packed[c], lmax) for c, name in enumerate(names)}
    model = SphericalHarmonicModel(lmax, radius, coefficients)
    model.normalization, model.csphase = normalization, csphase
    return model, iterations, residual, untouched


def degree_power(model: SphericalHarmonicModel, params=None):
    """The power per degree and knot row of a model in the 4-pi convention, ``sum_k (A_lk^2 + B_lk^2)``: name -> f64[m, L+1]
    (host work, table-sized).  With 4-pi-normalised harmonics the sum over the degrees is the mean square of the field over
    the sphere; the comparison plots of tomographic models at ``lmax = 20`` are made from these numbers."""
    return {p: (model.cos[p] ** 2 + model.sin[p] ** 2).sum(axis=2) for p in model.names(params)}
