"""Diffusion: the stiffness operator of a GLL mesh and the smoothing it gives (include/multimesh_hip.h,
mm_gll_diffusion_apply).  The reference has no counterpart: its smoothing lives in Salvus."""
import numpy as np

from .. import synth
from ..device import default_context
from ._common import _element_fields, _gll_points_order
from .layers import _selected_layers


def _sigma_lengths(sigma, shape, dim):
    """sigma -> (lateral, radial or None), each a float or f64[E, P]: validated, nothing squared yet."""
    def one(x, name):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 0 and x.shape != tuple(shape):
            raise ValueError(f"{name} must be a number or an element-nodal array {tuple(shape)}, not of shape {x.shape}")
        if np.isnan(x).any() or np.isinf(x).any() or (x < 0).any():
            raise ValueError(f"{name} must be finite and >= 0")
        return float(x) if x.ndim == 0 else np.ascontiguousarray(x)

    if isinstance(sigma, (tuple, list)):
        if len(sigma) != 2:
            raise ValueError("sigma must be a length, an element-nodal array, or a pair (lateral, radial) of either")
        if dim != 3:
            raise ValueError("a (lateral, radial) pair needs a 3-D mesh: in 2-D there is no radial direction to split off")
        return one(sigma[0], "sigma[0]"), one(sigma[1], "sigma[1]")
    return one(sigma, "sigma"), None


def _diffusion(ctx, pts, order, lengths):
    lat, rad = lengths
    return ctx.diffusion(order, pts, lat * lat, None if rad is None else rad * rad)


def gll_stiffness_apply(mesh, values, sigma=None, context=None):
    """``K_e u`` per element (not assembled) of a :class:`GllMesh` or a Salvus mesh -> f64[C, E, P]: the weak Laplacian
    ``K_e[p][q] = int grad phi_p . kappa grad phi_q dV`` by GLL quadrature, applied matrix-free (``mm_gll_diffusion_apply``,
    bit for bit the statement of include/multimesh_hip.h).  ``values``: names of element-nodal fields or an array
    [C, E, P] / [E, P].  ``sigma``: None for kappa = 1, else as :func:`smooth_gll` takes it (kappa = sigma^2)."""
    ctx = context or default_context()
    pts, order = _gll_points_order(mesh)
    synth.gll_derivative_matrix(order)                                            # (ValueError for an order without tables)
    u = _element_fields(mesh, values, pts.shape[:2])
    lengths = (1.0, None) if sigma is None else _sigma_lengths(sigma, pts.shape[:2], pts.shape[2])
    with _diffusion(ctx, pts, order, lengths) as op:
        return op.apply(u).numpy()


def gll_roughness(mesh, params, sigma=None, context=None):
    """``u^T K u = int grad u . kappa grad u dV`` for every parameter -> f64[C], the roughness a regularisation term
    penalises; summed on the device in the fixed order of ``mm_weighted_sum``.  Arguments as :func:`gll_stiffness_apply`."""
    ctx = context or default_context()
    pts, order = _gll_points_order(mesh)
    synth.gll_derivative_matrix(order)
    u = _element_fields(mesh, params, pts.shape[:2])
    lengths = (1.0, None) if sigma is None else _sigma_lengths(sigma, pts.shape[:2], pts.shape[2])
    with _diffusion(ctx, pts, order, lengths) as op:
        return op.roughness(u)


def smooth_gll(mesh, params, sigma, steps=4, rtol=1e-10, max_iter=2000, layers=None, layer_ids=None, context=None):
    """Element-nodal fields of a :class:`GllMesh` or a Salvus mesh smoothed by diffusion on the device -> f64[C, E, P].

    Smoothing with a Gaussian of standard deviation ``sigma`` is diffusion to the time ``sigma^2 / 2``; it is taken in
    ``steps`` backward-Euler steps ``(M + tau K) u_new = M u_old`` with ``tau = 1 / (2 steps)``, ``M`` the assembled GLL
    mass (:func:`gll_mass_matrix`) and ``K`` the assembled stiffness operator with ``kappa = sigma^2``
    (:func:`gll_stiffness_apply`), under natural boundary conditions: constants are kept and ``sum(M u)`` is conserved.
    A mode of eigenvalue ``lam`` is scaled by ``(1 + sigma^2 lam / (2 steps))^-steps``, which tends to the Gaussian's
    ``exp(-sigma^2 lam / 2)`` as ``steps`` grows: more steps, a truer Gaussian, at proportionally more work.

    ``sigma``: a length in the mesh's units -- a number, an element-nodal array [E, P], or a pair ``(lateral, radial)`` of
    either for a 3-D Earth mesh (``(L, 0)`` smooths along the spherical shells only).  ``params``: names of element-nodal
    fields, or an array [C, E, P] / [E, P].  Copies of a shared node that differ are first reduced to their mass-weighted
    mean (which keeps ``sum(M u)``); the copies of a node in the result hold identical bits.  Every step is solved by
    conjugate gradients preconditioned with ``M``, all components together, each stopped when
    ``sqrt(r^T M^-1 r) <= rtol * ||u_old||_M``, which bounds its error by ``||u - u*||_M <= rtol ||u_old||_M``; a step that
    needs more than ``max_iter`` iterations raises ``RuntimeError``.  ``sigma = 0`` returns the node-averaged input.

    ``layers`` (anything :func:`assess_layers` takes; ``layer_ids`` etc. default as in :func:`integrate`): each selected
    layer's elements are smoothed as a mesh of their own -- nothing diffuses across a layer boundary -- and all other
    elements are returned unchanged."""
    ctx = context or default_context()
    pts, order = _gll_points_order(mesh)
    synth.gll_derivative_matrix(order)                                            # (ValueError for an order without tables)
    fields = _element_fields(mesh, params, pts.shape[:2])
    lengths = _sigma_lengths(sigma, pts.shape[:2], pts.shape[2])
    if int(steps) < 1 or int(max_iter) < 1 or not 0.0 < float(rtol) < 1.0:
        raise ValueError("need steps >= 1, max_iter >= 1 and 0 < rtol < 1")

    def run(sub_pts, sub_fields, sub_lengths):
        with _diffusion(ctx, sub_pts, order, sub_lengths) as op:
            nsteps = 0 if all(x is None or not np.any(x) for x in sub_lengths) else int(steps)     # (sigma = 0: no step)
            return op.smooth(sub_fields, steps=nsteps, rtol=rtol, max_iter=max_iter).numpy()

    if layers is None:
        return run(pts, fields, lengths)
    picked, ids = _selected_layers(mesh, layers, layer_ids, nelem=pts.shape[0])
    out = fields.copy()
    for layer in picked:
        mask = ids == layer
        if mask.any():
            sub = tuple(x if x is None or np.ndim(x) == 0 else np.ascontiguousarray(x[mask]) for x in lengths)
            out[:, mask] = run(np.ascontiguousarray(pts[mask]), np.ascontiguousarray(fields[:, mask]), sub)
    return out


# ---- the gradient of element-nodal fields, as fields (include/multimesh_hip.h, mm_gll_gradient).  The
# stiffness operator forms it at every node and folds it into its flux; here it is written out.
def _gradient(mesh, params, assemble, ctx, wanted):
    """The planes ``wanted`` (flags of :meth:`Context.gll_gradient`) as NumPy arrays, node-averaged when ``assemble``."""
    pts, order = _gll_points_order(mesh)
    synth.gll_derivative_matrix(order)                                            # (ValueError for an order without tables)
    u = _element_fields(mesh, params, pts.shape[:2])
    if (wanted.get("radial") or wanted.get("lateral")) and pts.shape[2] != 3:
        raise ValueError("the radial / lateral split needs a 3-D mesh: on a 2-D mesh use gll_gradient")
    ctx = ctx or default_context()
    gp = ctx.to_device(pts)
    planes = ctx.gll_gradient(order, gp, u, **wanted)
    planes = planes if isinstance(planes, tuple) else (planes,)
    if assemble:
        with ctx.diffusion(order, gp) as op:                                      # (its smooth(steps=0) IS the node average)
            planes = tuple(op.smooth(v.reshape(int(np.prod(v.shape[:-2])), *pts.shape[:2]), steps=0) if v.size else v
                           for v in planes)
    return pts, u.shape[0], [v.numpy() for v in planes]


def gll_gradient(mesh, params, assemble=False, context=None):
    """The spatial gradient of element-nodal fields of a :class:`GllMesh` or a Salvus mesh -> f64[C, dim, E, P]:
    ``grad u = J^-1 grad_ref u`` at every GLL node, with the Jacobian of the element's own geometry (``mm_gll_gradient``,
    bit for bit the statement of include/multimesh_hip.h; the gradient the stiffness operator of
    :func:`gll_stiffness_apply` integrates).  ``params``: names of element-nodal fields, or an array [C, E, P] / [E, P].
    Every ``[c, d]`` plane is an ordinary element-nodal field: it can be integrated, smoothed, gathered or put on a grid.

    The gradient of a continuous field jumps across element faces, so the copies of a shared node differ.  With
    ``assemble=True`` every plane is replaced by the mass-weighted mean over the copies of each unique node,
    ``A(M_e v) / A(M_e)`` with ``M_e`` = :func:`gll_mass_matrix` and ``A`` = :func:`assemble_gll` -- the reduction
    :func:`smooth_gll` applies to input copies that differ; the copies of a node then hold identical bits.  The mean is
    taken of the planes as the kernel wrote them."""
    pts, ncomp, (grad,) = _gradient(mesh, params, assemble, context, dict(grad=True))
    return grad.reshape((ncomp, pts.shape[2]) + pts.shape[:2])


def gll_gradient_parts(mesh, params, assemble=False, context=None):
    """What an Earth model's gradient is read by, on a 3-D mesh: a dict of f64[C, E, P] with ``radial`` = the derivative
    along ``x / |x|`` (signed), ``lateral`` = the norm of the gradient without its radial part, ``norm`` = ``|grad u|``
    (``lateral^2 + radial^2 = norm^2`` up to rounding).  Arguments as :func:`gll_gradient`, which is the function for a 2-D
    mesh (``ValueError`` here).  ``assemble=True`` node-averages every plane as the kernel wrote it: ``norm`` is then the
    mean of the norms, not the norm of the mean gradient (and likewise ``lateral``)."""
    pts, ncomp, parts = _gradient(mesh, params, assemble, context, dict(grad=False, radial=True, lateral=True, norm=True))
    return {name: v.reshape((ncomp,) + pts.shape[:2]) for name, v in zip(("radial", "lateral", "norm"), parts)}
