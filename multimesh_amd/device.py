"""Thin ctypes layer over the device-pointer API of ``multi_mesh_hip.so``.

Arrays handed to a :class:`Context` method may be NumPy arrays (copied to HBM for the call),
:class:`DeviceArray` objects, or anything exposing ``data_ptr()`` / ``shape`` / ``dtype``
(``torch`` CUDA tensors -- torch is only plumbing for device memory and RCCL here).  Results
are :class:`DeviceArray` objects; ``.numpy()`` copies them back.

No CPU fallback: every method ends in a HIP kernel launch and raises
:class:`multimesh_amd.helpers.MultiMeshHipError` when the GPU is missing.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import helpers as H
from .helpers import MM_FP_EXACT, MM_FP_TOL, MM_KNN_MAX_K, STAGES, MultiMeshHipError, check, load_lib
from .synth import gll_derivative_matrix, gll_order_table, gll_weights_1d   # (ValueError for an order without tables)

# MM_KNN_RAN_* in bit order
KNN_KERNELS = ("lane", "strip", "cell", "list", "generic", "levels", "tree", "one_pass", "target_replay")
#: centres per LDS batch of the taper kernel (kBatch in csrc/mm_precondition.hip)
POINT_TAPER_BATCH = 256

_NP2ITEM = {np.dtype(np.float64): 8, np.dtype(np.int64): 8, np.dtype(np.int32): 4, np.dtype(np.uint8): 1}


class _Released:
    """Whatever holds device memory or a library handle is released when it is collected: ``__del__`` runs ``free()`` (or
    the method ``_release`` names), which may have run before, and never raises."""
    _release = "free"

    def __del__(self):
        try:
            getattr(self, self._release)()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        getattr(self, self._release)()


class _Handle(_Released):
    """A library handle on a context; the subclass names the symbol that destroys it.  After ``free()`` it is None."""
    _destroy = None

    def free(self):
        if self.handle and self.ctx.handle:
            getattr(self.ctx.lib, self._destroy)(self.ctx.handle, self.handle)
        self.handle = None


# ---- the one place where Python calls the library ---------------------------------------------------
# (what releases -- DeviceArray.free, _Handle.free, Context.close -- stays direct: no status comes back and nothing may raise)
def _call(lib, symbol, *args, what=None, arg_error=False):
    """``lib.symbol(*args)`` with every :class:`DeviceArray` passed as its address; None (a null pointer), flags (ctypes
    takes a ``bool`` as 0 / 1), numbers, addresses and ctypes objects go as they are.  Returns the status, a count >= 0; a
    negative one raises through :func:`check`, which names ``what`` (the symbol unless given) -- or, with ``arg_error``,
    status -1 (MM_ERR_ARG) is the caller's mistake: ``ValueError`` with the library's message."""
    rc = getattr(lib, symbol)(*[a.ptr if type(a) is DeviceArray else a for a in args])
    if rc < 0:
        if arg_error and rc == -1:
            raise ValueError(lib.mm_last_error().decode(errors="replace"))
        check(rc, what or symbol)
    return rc


def _create(lib, symbol, *args):
    """The value of the handle that ``symbol`` writes through its last argument."""
    h = C.c_void_p()
    _call(lib, symbol, *args, C.byref(h))
    return h.value


def _components(x, ndim):
    """A single component given without its leading axis ([M], [E, P], [D, LA, LO]: ``ndim`` axes) as [1, ...]."""
    return x.reshape(1, *x.shape) if len(x.shape) == ndim else x


def _major(n, ncomp, point_major):
    """The shape of ``ncomp`` values at each of ``n`` points: [N, C] point-major, else [C, N]."""
    return (n, ncomp) if point_major else (ncomp, n)


def _list_width(nn):
    """``k`` of candidate lists int64[N, k]; a flat array holds no lists."""
    return nn.shape[1] if len(nn.shape) == 2 else 0


def _element_nodal(ctx, values, nelem, P, name):
    """``values`` as f64[C, E, P] on the device over the nodes of a GLL mesh."""
    v = _components(ctx.asdevice(values, np.float64), 2)
    if len(v.shape) != 3 or v.shape[1:] != (nelem, P):
        raise ValueError(f"{name} must be [C, E, P] (or [E, P]) over gll_points [E, P, dim]")
    return v


def _hex8_arrays(ctx, nnodes, points, fields, want_operator, out):
    """What interpolate_hex8 and Source.interpolate hand to their call besides the mesh: (points, fields f64[C, M], values
    f64[N, C], enc, weights), the last two None unless the operator is wanted.  ``out`` is taken at the caller's word."""
    pts = ctx.asdevice(points, np.float64)
    f = _components(ctx.asdevice(fields, np.float64), 1)
    if f.shape[1] != nnodes:
        raise ValueError("fields must be [C, number of nodes]")
    n = pts.shape[0]
    out = ctx._out(out, (n, f.shape[0]))
    return pts, f, out, ctx._wanted(want_operator, (n, 8), np.int64), ctx._wanted(want_operator, (n, 8))


def _with_operator(want_operator, values, index, weights, count):
    """(values, count) or, with the operator, (values, index, weights, count)."""
    return (values, index, weights, int(count)) if want_operator else (values, int(count))


class DeviceArray(_Released):
    """A C-contiguous array resident in HBM, owned (or merely viewed) by a Context."""

    def __init__(self, ctx, ptr, shape, dtype, owner=True, keepalive=None):
        self.ctx = ctx
        self.ptr = int(ptr)
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self._owner = owner
        self._keepalive = keepalive

    @property
    def nbytes(self):
        return int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def data_ptr(self):
        return self.ptr

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if out.nbytes:
            self.ctx._call("mm_copy_d2h", out.ctypes.data, self, out.nbytes)
        return out

    def rows(self, start, stop):
        """A non-owning view of rows [start, stop) (first axis)."""
        row_bytes = self.nbytes // max(self.shape[0], 1) if self.shape[0] else 0
        return DeviceArray(self.ctx, self.ptr + start * row_bytes, (stop - start,) + self.shape[1:], self.dtype,
                           owner=False, keepalive=self)

    def reshape(self, *shape):
        """A non-owning view of the same bytes in another shape of the same size; it keeps this array alive."""
        view = DeviceArray(self.ctx, self.ptr, shape, self.dtype, owner=False, keepalive=self)
        if view.size != self.size:
            raise ValueError(f"cannot reshape {self.shape} to {view.shape}")
        return view

    def free(self):
        if self._owner and self.ptr and self.ctx.handle:
            self.ctx.lib.mm_device_free(self.ctx.handle, self.ptr)
        self.ptr = 0
        self._owner = False


class KnnIndex(_Handle):
    """Device-resident search structure over source points (the cKDTree stand-in)."""
    _destroy = "mm_knn_destroy"

    def __init__(self, ctx, handle, nsrc, ndim, keepalive):
        self.ctx, self.handle, self.nsrc, self.ndim = ctx, handle, nsrc, ndim
        self._keepalive = keepalive

    def query(self, points, k, want_dist=False):
        """``tree.query(points, k)`` of reference scripts/cli.py:71-73 -> idx int64[N,k] (, dist)."""
        ctx = self.ctx
        pts = ctx.asdevice(points, np.float64)
        if len(pts.shape) != 2 or pts.shape[1] != self.ndim:
            raise ValueError("points must be [N, ndim]")
        if not 0 <= k <= MM_KNN_MAX_K:
            raise ValueError(f"k must be in 0..{MM_KNN_MAX_K}")
        n = pts.shape[0]
        idx = ctx.empty((n, k), np.int64)
        dist = ctx._wanted(want_dist, (n, k))
        ctx._call("mm_knn_query", self.handle, pts, n, k, idx, dist)
        return (idx, dist) if want_dist else idx


class Source(_Handle):
    """A hex8 source mesh kept resident for repeated calls (mm_source_create): nodes, connectivity, element centroids and
    the search grid over them -- built once, like the reference's cKDTree (scripts/cli.py:66, queried at :141-195)."""
    _destroy = "mm_source_destroy"

    def __init__(self, ctx, handle, nodes, conn):
        self.ctx, self.handle = ctx, handle
        self.nodes, self.conn = nodes, conn      # (borrowed by the library: kept alive here)

    def interpolate(self, points, fields, nelem_to_search=20, want_operator=False, out=None):
        """:meth:`Context.interpolate_hex8` without the centroid and grid-build stages; identical results."""
        ctx = self.ctx
        pts, f, out, enc, w = _hex8_arrays(ctx, self.nodes.shape[0], points, fields, want_operator, out)
        nf = ctx._call("mm_interpolate_hex8_on", self.handle, pts, pts.shape[0], f, f.shape[0], nelem_to_search, out, enc, w)
        return _with_operator(want_operator, out, enc, w, nf)


class TransposedOperator(_Handle):
    """The transpose of an interpolation operator, grouped by destination once (mm_transpose_create_nodes / _elem) and
    applied to any number of value sets: bit for bit ``np.add.at`` on zeros (include/multimesh_hip.h)."""
    _destroy = "mm_transpose_destroy"

    def __init__(self, ctx, handle, npoints, out_shape, keepalive):
        self.ctx, self.handle, self.npoints = ctx, handle, int(npoints)
        self.out_shape = tuple(int(s) for s in out_shape)   # one component: (nsrc,) or (nelem, P)
        self._keepalive = keepalive                         # (the element form's coeffs are borrowed by the library)

    def apply(self, values, point_major=True, out=None):
        """values f64[N, C] (point_major; [N] = one component) or f64[C, N] -> f64[C, nsrc] / f64[C, nelem, P]."""
        ctx = self.ctx
        if not self.handle:
            raise ValueError("the operator has been freed")
        v = ctx.asdevice(values, np.float64)
        if len(v.shape) == 1:
            v = v.reshape(*_major(v.shape[0], 1, point_major))
        if len(v.shape) != 2 or v.shape[0 if point_major else 1] != self.npoints:
            raise ValueError("values must be [N, C] (point_major) or [C, N]")
        ncomp = v.shape[1 if point_major else 0]
        shape = (ncomp,) + self.out_shape
        out = ctx._out(out, shape, f"out must be {shape}")
        ctx._call("mm_transpose_apply", self.handle, v, ncomp, bool(point_major), out)
        return out

    def free(self):
        super().free()
        self._keepalive = None


class Diffusion(_Released):
    """The stiffness operator ``K`` of an element-nodal GLL mesh with its diffusivity (``mm_gll_diffusion_apply``), and the
    backward-Euler diffusion steps ``(M + tau K) u_new = M u_old`` on the assembled space that smooth a field with it.
    What depends on the mesh alone -- the tables, the scatter-sum over shared nodes, the inverse index, the assembled mass
    -- is built once (the assembly on the first :meth:`smooth`) and reused over steps, components and calls."""

    def __init__(self, ctx, order, gll_points, kappa_h, kappa_r, tables):
        self.ctx, self.order = ctx, int(order)
        self.gp = gll_points                                    # device f64[E, P, dim]
        self.nelem, self.P, self.dim = gll_points.shape
        self.kappa_h, self.kappa_r = kappa_h, kappa_r           # (scalar, device array or None); kappa_r None: isotropic
        self._deriv, self._weights = tables
        self._asm = None
        self.last_iterations = []                               # of the last smooth(): [steps][C] PCG iterations

    # ---- K u ------------------------------------------------------------------------------
    def _apply(self, u, ncomp, y):
        kh_s, kh_a = self.kappa_h
        kr_s, kr_a = self.kappa_r if self.kappa_r is not None else (0.0, None)
        self.ctx._call("mm_gll_diffusion_apply", self.order, self.dim, self.gp, self.nelem, self._deriv, self._weights, u,
                       ncomp, float(kh_s), kh_a, self.kappa_r is not None, float(kr_s), kr_a, y)

    def _fields(self, values):
        return _element_nodal(self.ctx, values, self.nelem, self.P, "values")

    def apply(self, u, out=None):
        """``K_e u`` per element, not assembled: u f64[C, E, P] (or [E, P]) -> f64[C, E, P]."""
        if self.gp is None:
            raise ValueError("the operator has been freed")
        v = self._fields(u)
        out = self.ctx._out(out, v.shape, "out must be another array of the shape of u")
        if out.ptr == v.ptr:
            raise ValueError("out must be another array of the shape of u")
        self._apply(v, v.shape[0], out)
        return out

    def roughness(self, u):
        """``u^T K u`` = ``int grad u . kappa grad u dV`` per component -> f64[C] (NumPy), in the fixed order of
        ``mm_weighted_sum`` with ``u`` in the mass slot."""
        ctx = self.ctx
        v = self._fields(u)
        y = self.apply(v)
        n, ncomp = self.nelem * self.P, v.shape[0]
        out = ctx.empty((ncomp,), np.float64)
        for c in range(ncomp):
            ctx._call("mm_weighted_sum", v.ptr + 8 * c * n, y.ptr + 8 * c * n, n, 1, out.ptr + 8 * c)
        return out.numpy()

    # ---- the assembled space ------------------------------------------------------------------
    def _assembly(self):
        if self._asm is None:
            ctx = self.ctx
            n = self.nelem * self.P
            uniq, inv = ctx.unique_points(self.gp.reshape(n, self.dim), ordered=False)
            nu = uniq.shape[0]
            inverse = inv.reshape(n, 1)
            ones = ctx.to_device(np.ones((n, 1)))
            op = ctx.transpose_nodes(inverse, ones, nu)
            elem_mass, _ = ctx.gll_mass(self.order, self.gp)
            mass = op.apply(elem_mass.reshape(1, n), point_major=False)   # [1, U]: the assembled mass
            self._asm = dict(op=op, inverse=inverse, ones=ones, elem_mass=elem_mass, mass=mass, n=n, nu=nu)
        return self._asm

    def _gather(self, x, ncomp, out):
        """unique nodes [C, U] -> every copy [C, N]"""
        a = self._asm
        self.ctx._call("mm_gather", x, a["nu"], ncomp, a["inverse"], a["ones"], a["n"], 1, out, 0)

    def _combine(self, mass, p, tau, kp, n, ncomp, out):
        self.ctx._call("mm_pcg_combine", mass, p, float(tau), kp, n, ncomp, out)

    def _dots(self, a, b, n, ncomp, state, slot):
        for c in range(ncomp):
            self.ctx._call("mm_weighted_sum", a.ptr + 8 * c * n, b.ptr + 8 * c * n, n, 1,
                           state.ptr + 8 * (c * H.MM_PCG_STATE + slot))

    def smooth(self, values, steps=4, rtol=1e-10, max_iter=2000):
        """``steps`` backward-Euler steps of ``tau = 1 / (2 steps)`` each: ``(M + tau K) u_new = M u_old`` on the unique
        nodes, by conjugate gradients preconditioned with ``M`` and stopped, per component, when
        ``sqrt(r^T M^-1 r) <= rtol * sqrt(b^T M^-1 b)``; so ``||u - u*||_M <= rtol ||u_old||_M`` per step.  values
        f64[C, E, P] (or [E, P]); copies of a shared node that differ are first reduced to their mass-weighted mean.
        Returns f64[C, E, P] on the device, copies of a node bit-identical.  ``steps=0`` returns the node-averaged input.
        Raises ``RuntimeError`` when a step needs more than ``max_iter`` iterations.  ``last_iterations[step][c]``: the
        iterations every component took."""
        if self.gp is None:
            raise ValueError("the operator has been freed")
        steps, max_iter, rtol = int(steps), int(max_iter), float(rtol)
        if steps < 0 or max_iter < 1 or not 0.0 < rtol < 1.0:
            raise ValueError("need steps >= 0, max_iter >= 1 and 0 < rtol < 1")
        ctx = self.ctx
        v = self._fields(values)
        ncomp = v.shape[0]
        a = self._assembly()
        n, nu, op, mass = a["n"], a["nu"], a["op"], a["mass"]
        ve = ctx.empty((ncomp, n), np.float64)                  # element-nodal work array
        ye = ctx.empty((ncomp, n), np.float64)
        self._combine(a["elem_mass"], v, 0.0, None, n, ncomp, ve)
        x = op.apply(ve, point_major=False)                     # [C, U]
        ctx._call("mm_divide_rows", x, mass, nu, ncomp, x)
        self.last_iterations = []
        if steps and ncomp and n:
            tau = 1.0 / (2.0 * steps)
            r, z, ap, kp = (ctx.empty((ncomp, nu), np.float64) for _ in range(4))
            p = ctx.zeros((ncomp, nu), np.float64)
            state = ctx.zeros((ncomp, H.MM_PCG_STATE), np.float64)
            nactive = ctx.zeros((1,), np.int64)

            def stiffness(src):                                 # kp = A^T K_e A src
                self._gather(src, ncomp, ve)
                self._apply(ve, ncomp, ye)
                op.apply(ye, point_major=False, out=kp)

            for _ in range(steps):
                ctx._call("mm_pcg_scalars", state, ncomp, H.MM_PCG_PHASE_START, rtol, None)
                self._combine(mass, x, 0.0, None, nu, ncomp, ap)            # b = M u_old
                self._dots(ap, x, nu, ncomp, state, H.MM_PCG_BB)            # b^T M^-1 b = ||u_old||_M^2
                stiffness(x)
                self._combine(None, None, -tau, kp, nu, ncomp, r)           # r = b - (M + tau K) u_old
                done_at = [None] * ncomp
                left = ncomp
                for it in range(max_iter + 1):
                    ctx._call("mm_divide_rows", r, mass, nu, ncomp, z)
                    self._dots(r, z, nu, ncomp, state, H.MM_PCG_RZ)
                    ctx._call("mm_pcg_scalars", state, ncomp, H.MM_PCG_PHASE_BETA, rtol, nactive)
                    now = int(nactive.numpy()[0])                           # the one number read back per iteration
                    if now != left:
                        active = state.numpy()[:, H.MM_PCG_ACTIVE]
                        for c in range(ncomp):
                            if done_at[c] is None and active[c] == 0.0:
                                done_at[c] = it
                        left = now
                    if now == 0:
                        break
                    if it == max_iter:
                        raise RuntimeError(f"smooth: {now} of {ncomp} components did not reach rtol = {rtol} within "
                                           f"{max_iter} iterations of a diffusion step")
                    ctx._call("mm_pcg_direction", state, z, nu, ncomp, p)
                    stiffness(p)
                    self._combine(mass, p, tau, kp, nu, ncomp, ap)
                    self._dots(p, ap, nu, ncomp, state, H.MM_PCG_PAP)
                    ctx._call("mm_pcg_scalars", state, ncomp, H.MM_PCG_PHASE_ALPHA, rtol, None)
                    ctx._call("mm_pcg_advance", state, p, ap, nu, ncomp, x, r)
                self.last_iterations.append(done_at)
        out = ctx.empty((ncomp, self.nelem, self.P), np.float64)
        if n and ncomp:
            self._gather(x, ncomp, out)
        ctx.synchronize()                                       # (the work arrays are released when this returns)
        return out

    def free(self):
        if self._asm is not None:
            self._asm["op"].free()
        self._asm = None
        self.gp = None
        self.kappa_h, self.kappa_r = (1.0, None), None


class Context(_Released):
    """One GPU + one HIP stream.  ``stream`` is a raw hipStream_t value (e.g.
    ``torch.cuda.current_stream().cuda_stream``); None = the device's default stream."""
    _release = "close"

    def __init__(self, device=0, stream=None):
        self.lib = load_lib()
        self.handle = _create(self.lib, "mm_context_create", int(device), C.c_void_p(stream) if stream else None)
        self.device = int(device)

    # ---- library calls on this context: the handle goes first ------------------------------
    def _call(self, symbol, *args, what=None):
        return _call(self.lib, symbol, self.handle, *args, what=what)

    def _call_args(self, symbol, *args):
        """:meth:`_call` for the symbols whose status -1 (MM_ERR_ARG) is the caller's mistake: ``ValueError`` with the
        library's message."""
        return _call(self.lib, symbol, self.handle, *args, arg_error=True)

    def _create(self, symbol, *args):
        return _create(self.lib, symbol, self.handle, *args)

    # ---- memory -------------------------------------------------------------------------
    def empty(self, shape, dtype):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        return DeviceArray(self, self._create("mm_device_alloc", nbytes), shape, dtype)

    def zeros(self, shape, dtype):
        a = self.empty(shape, dtype)
        if a.nbytes:
            self._call("mm_memset", a, 0, a.nbytes)
        return a

    def to_device(self, array, dtype=None):
        a = np.ascontiguousarray(array, dtype=dtype)
        d = self.empty(a.shape, a.dtype)
        if a.nbytes:
            self._call("mm_copy_h2d", d, a.ctypes.data, a.nbytes)
        return d

    @staticmethod
    def _on_host(x):
        """Whether ``x`` names a ``device`` that is not a GPU (a CPU tensor); no ``device`` at all: not on the host."""
        device = getattr(x, "device", None)
        return device is not None and getattr(device, "type", "cuda") != "cuda"

    def asdevice(self, x, dtype):
        """NumPy -> copy to HBM; DeviceArray / torch-like on this GPU -> wrap without copying.  A torch-like object whose
        ``device`` is not a GPU is copied like NumPy; one on another GPU raises ``ValueError``; one without a ``device``
        is device memory at the caller's word."""
        dtype = np.dtype(dtype)
        if isinstance(x, DeviceArray):
            if x.dtype != dtype:
                raise TypeError(f"expected {dtype}, got {x.dtype}")
            return x
        if hasattr(x, "data_ptr") and hasattr(x, "shape") and not self._on_host(x):
            index = getattr(getattr(x, "device", None), "index", None)
            if index is not None and index != self.device:
                raise ValueError(f"tensor lives on GPU {index}, this context on GPU {self.device}")
            name = str(getattr(x, "dtype", "")).replace("torch.", "")
            if name and np.dtype(name) != dtype:
                raise TypeError(f"expected {dtype}, got {name}")
            if hasattr(x, "is_contiguous") and not x.is_contiguous():
                raise ValueError("device tensor must be contiguous")
            return DeviceArray(self, x.data_ptr(), tuple(x.shape), dtype, owner=False, keepalive=x)
        return self.to_device(np.asarray(x), dtype)

    def synchronize(self):
        self._call("mm_synchronize")

    # ---- checks that many methods share ------------------------------------------------------
    def _out(self, out, shape, message=None, size_only=False):
        """The f64 output of a call: a new array of ``shape`` or the caller's ``out``, which must have that shape (with
        ``size_only``: that many values in any shape) or ``message`` is raised; no message: the caller's word."""
        if out is None:
            return self.empty(shape, np.float64)
        if not isinstance(out, DeviceArray):             # (a copy of it would receive the result and be lost)
            index = getattr(getattr(out, "device", None), "index", None)
            if not (hasattr(out, "data_ptr") and hasattr(out, "shape")) or self._on_host(out) or \
                    (index is not None and index != self.device):
                raise ValueError(f"out must live on GPU {self.device}")
        out = self.asdevice(out, np.float64)
        if message and (out.size != int(np.prod(shape, dtype=np.int64)) if size_only else out.shape != tuple(shape)):
            raise ValueError(message)
        return out

    def _wanted(self, want, shape, dtype=np.float64):
        """An optional output: a new array when it is wanted, else None -- a null pointer to the library."""
        return self.empty(shape, dtype) if want else None

    def _node_groups(self, points):
        """(points f64[G, P, 3] on the device -- or [N, 3]: P = 1 --, G, P) with at most 256 nodes per group."""
        pts = self.asdevice(points, np.float64)
        if len(pts.shape) not in (2, 3) or pts.shape[-1] != 3:
            raise ValueError("points must be [G, P, 3] or [N, 3]")
        ngroups, P = (pts.shape[0], pts.shape[1]) if len(pts.shape) == 3 else (pts.shape[0], 1)
        if not 1 <= P <= 256:
            raise ValueError("P must lie in [1, 256]")
        return pts, ngroups, P

    def _flat_rows(self, values, message):
        """(values on the device, rows, values per row) of f64[C, ...], every row read flat, or f64[n]: one row."""
        v = self.asdevice(values, np.float64)
        if len(v.shape) == 0:
            raise ValueError(message)
        nrows = v.shape[0] if len(v.shape) > 1 else 1
        return v, nrows, v.size // nrows if nrows else 0

    def _pairs(self, ids, weights):
        """(ids int64[N, P], weights f64[N, P], N, P) of an operator on the device."""
        idv = self.asdevice(ids, np.int64)
        w = self.asdevice(weights, np.float64)
        if idv.shape != w.shape or len(idv.shape) != 2:
            raise ValueError("ids and weights must both be [N, P]")
        return (idv, w) + idv.shape

    def _gll_points(self, shape_order, gll_points):
        """(gll_points f64[nelem, P, dim] on the device, nelem, P, dim) of a 2-D or 3-D GLL mesh of ``shape_order``."""
        gp = self.asdevice(gll_points, np.float64)
        if len(gp.shape) != 3 or gp.shape[2] not in (2, 3) or gp.shape[1] != (shape_order + 1) ** gp.shape[2]:
            raise ValueError("gll_points must be [nelem, (order+1)^dim, dim] with dim 2 or 3")
        return (gp,) + gp.shape

    def _fields_over(self, m, fields):
        """(fields on the device or None, number of components) for fields over the values of ``m``."""
        if fields is None:
            return None, 1
        f = self.asdevice(fields, np.float64)
        if f.shape == m.shape:
            return f, 1
        if f.shape[1:] == m.shape:
            return f, f.shape[0]
        raise ValueError("fields must be [C, ...] over the shape of mass, or the shape of mass")

    # ---- timers -------------------------------------------------------------------------
    def set_profiling(self, on=True):
        """Stage timers: False / True (all stages) / 2 (only the kNN tile kernel and the first locate pass)."""
        self._call("mm_set_profiling", 2 if on == 2 and on is not True else bool(on))

    def set_lazy_lists(self, on=True):
        """interpolate_hex8 asks the kNN stage for the 8 nearest first and for the full list only for
        targets that exhaust them (bit-identical outputs; default on)."""
        self._call("mm_set_lazy_lists", bool(on))

    def set_fp_mode(self, mode):
        """Arithmetic of the hex8 locate stage: "exact" (default: the reference's operations, every output bit-identical)
        or "tol" (cheaper Newton arithmetic that certifies every decision of the reference's iteration or repeats the
        solve exactly: node ids / failed count still bit-identical, weights and values to ~1e-12; include/multimesh_hip.h)."""
        m = {"exact": MM_FP_EXACT, "tol": MM_FP_TOL, MM_FP_EXACT: MM_FP_EXACT, MM_FP_TOL: MM_FP_TOL}[mode]
        self._call("mm_set_fp_mode", m)

    def fp_mode(self):
        return "tol" if self._call("mm_get_fp_mode") == MM_FP_TOL else "exact"

    def last_locate_stats(self):
        """Of the last hex8 locate stage: solves MM_FP_TOL repeated in the reference's arithmetic, targets the first pass
        left over (for the reference-order kernel, or a long on-demand list's second pass), targets that second pass left
        over for the reference-order kernel (synchronises)."""
        buf = (C.c_longlong * 4)()
        self._call("mm_last_locate_stats", buf)
        return {"redone_exact": int(buf[0]), "reference_order": int(buf[1]), "second_pass": int(buf[2])}

    def last_knn_kernels(self):
        """Names of the kNN kernels the last call launched: a subset of KNN_KERNELS (include/multimesh_hip.h)."""
        m = C.c_int()
        self._call("mm_last_knn_kernels", C.byref(m))
        return {name for bit, name in enumerate(KNN_KERNELS) if m.value >> bit & 1}

    def last_timings(self):
        """Per-stage milliseconds of the last call (hipEvents on this context's stream)."""
        buf = (C.c_double * len(STAGES))()
        self._call("mm_last_timings", buf, len(STAGES))
        return {name: buf[i] for i, name in enumerate(STAGES)}

    # ---- A1 -----------------------------------------------------------------------------
    def centroid(self, connectivity, points):
        conn = self.asdevice(connectivity, np.int64)
        pts = self.asdevice(points, np.float64)
        nelem, nper = conn.shape
        ndim = pts.shape[1]
        out = self.empty((nelem, ndim), np.float64)
        self._call("mm_centroid", ndim, nelem, nper, conn, pts, out)
        return out

    # ---- A2 -----------------------------------------------------------------------------
    def knn_build(self, sources):
        src = self.asdevice(sources, np.float64)
        if len(src.shape) != 2 or not 1 <= src.shape[1] <= 3:
            raise ValueError("sources must be [nsrc, ndim] with ndim in 1..3")
        handle = self._create("mm_knn_build", src, src.shape[0], src.shape[1])
        return KnnIndex(self, handle, src.shape[0], src.shape[1], keepalive=src)

    # ---- A4 -----------------------------------------------------------------------------
    def locate_hex8(self, nearest_element_indices, connectivity, nodes, points, enc=None, weights=None,
                    conn_is_exodus=False):
        """Returns (enc int64[N,8], weights f64[N,8], nfailed).  ``enc``/``weights`` given ->
        updated in place (rows of failed points untouched), else zero-initialised here as the
        reference's callers do (scripts/cli.py:77-78)."""
        nn = self.asdevice(nearest_element_indices, np.int64)
        conn = self.asdevice(connectivity, np.int64)
        nod = self.asdevice(nodes, np.float64)
        pts = self.asdevice(points, np.float64)
        n = pts.shape[0]
        if conn.shape[1] != 8 or nod.shape[1] != 3 or pts.shape[1] != 3 or nn.shape[0] != n:
            raise ValueError("shape mismatch: need nn[N,k], connectivity[E,8], nodes[M,3], points[N,3]")
        enc = self.zeros((n, 8), np.int64) if enc is None else self.asdevice(enc, np.int64)
        w = self.zeros((n, 8), np.float64) if weights is None else self.asdevice(weights, np.float64)
        nf = self._call("mm_locate_hex8", _list_width(nn), n, nn, conn, conn.shape[0], bool(conn_is_exodus), enc, nod, w, pts)
        return enc, w, int(nf)

    # ---- A9 -----------------------------------------------------------------------------
    def gather(self, fields, ids, weights, point_major=True):
        """fields f64[C,M] (or [M]) -> f64[N,C] (point_major) or f64[C,N]."""
        f = _components(self.asdevice(fields, np.float64), 1)
        idv, w, n, p = self._pairs(ids, weights)
        ncomp, nsrc = f.shape
        out = self.empty(_major(n, ncomp, point_major), np.float64)
        self._call("mm_gather", f, nsrc, ncomp, idv, w, n, p, out, bool(point_major))
        return out

    # ---- A10 (GLL) ------------------------------------------------------------------------
    def _locate_gll(self, symbol, shape_order, nearest_element_indices, gll_points, points, *options):
        nn = self.asdevice(nearest_element_indices, np.int64)
        gp = self.asdevice(gll_points, np.float64)
        pts = self.asdevice(points, np.float64)
        nelem, P, dim = gp.shape
        if P != (shape_order + 1) ** dim or pts.shape[1] != dim:
            raise ValueError("gll_points must be [nelem, (order+1)^dim, dim] and points [N, dim]")
        n = pts.shape[0]
        elem = self.empty((n,), np.int64)
        coeffs = self.empty((n, P), np.float64)
        count = self._call(symbol, shape_order, dim, _list_width(nn), n, nn, gp, nelem, pts, *options, elem, coeffs)
        return elem, coeffs, int(count)

    def locate_gll(self, shape_order, nearest_element_indices, gll_points, points, tolerance=1.05,
                   snap_to_nearest=False):
        """``get_element_weights`` core (reference interpolator.py:1181-1233) for
        gll_points f64[E, (order+1)^dim, dim].  Returns (elem int64[N], coeffs f64[N,P], nmissing)."""
        return self._locate_gll("mm_locate_gll", shape_order, nearest_element_indices, gll_points, points,
                                float(tolerance), bool(snap_to_nearest))

    def locate_gll_bbox(self, shape_order, nearest_element_indices, gll_points, points):
        """The bounding-box variant ``_check_if_inside_element`` (reference interpolator.py:1409-1473)
        for gll_points f64[E, (order+1)^dim, dim].  Returns (elem int64[N], coeffs f64[N,P], number
        of points whose final inverse transform failed)."""
        return self._locate_gll("mm_locate_gll_bbox", shape_order, nearest_element_indices, gll_points, points)

    def points_to_elements(self, indices, nodes_per_element):
        """Indices of GLL points, int64 of any shape on the device, replaced in place by the element each point belongs
        to, ``floor(index / nodes_per_element)`` (``mm_points_to_elements``).  Returns the array."""
        idx = self.asdevice(indices, np.int64)
        self._call("mm_points_to_elements", idx, idx.size, int(nodes_per_element))
        return idx

    def gather_elem(self, element_nodal_fields, elem, coeffs, point_major=True):
        """``np.sum(coeffs * field[elem], axis=1)`` (reference interpolator.py:976);
        element_nodal_fields f64[C, E, P] (or [E, P]) -> f64[N, C]."""
        f = _components(self.asdevice(element_nodal_fields, np.float64), 2)
        el = self.asdevice(elem, np.int64)
        co = self.asdevice(coeffs, np.float64)
        ncomp, nelem, P = f.shape
        n = el.shape[0]
        if co.shape != (n, P):
            raise ValueError("coeffs must be [N, P]")
        out = self.empty(_major(n, ncomp, point_major), np.float64)
        self._call("mm_gather_elem", f, nelem, ncomp, el, co, n, P, out, bool(point_major))
        return out

    # ---- the transposes of gather / gather_elem ------------------------------------------------
    def transpose_nodes(self, ids, weights, nsrc):
        """Group the operator (ids int64[N, P], weights f64[N, P]) by source node: a :class:`TransposedOperator` whose
        ``apply(values)`` is ``np.add.at(out[c], ids, weights * values[:, c, None])`` -> f64[C, nsrc]."""
        idv, w, n, p = self._pairs(ids, weights)
        handle = self._create("mm_transpose_create_nodes", idv, w, n, p, int(nsrc))
        return TransposedOperator(self, handle, n, (int(nsrc),), None)   # (the handle owns its sorted copy)

    def transpose_elem(self, elem, coeffs, nelem):
        """Group the GLL operator (elem int64[N], coeffs f64[N, P]) by source element: ``apply(values)`` ->
        f64[C, nelem, P], the sequential sums of ``coeffs[n] * values[n, c]`` per element; rows with elem -1 are skipped."""
        el = self.asdevice(elem, np.int64)
        co = self.asdevice(coeffs, np.float64)
        if len(el.shape) != 1 or len(co.shape) != 2 or co.shape[0] != el.shape[0]:
            raise ValueError("elem must be [N] and coeffs [N, P]")
        n, p = co.shape
        handle = self._create("mm_transpose_create_elem", el, co, n, p, int(nelem))
        return TransposedOperator(self, handle, n, (int(nelem), p), co)

    # ---- the GLL mass matrix and what it weights ----------------------------------------------
    def gll_mass(self, shape_order, gll_points, want_det=False):
        """The diagonal GLL mass matrix ``w_p |det J_e(xi_p)|`` of gll_points f64[E, (order+1)^dim, dim], orders 1, 2, 4
        (``mm_gll_mass``: bit for bit the NumPy statement of include/multimesh_hip.h).  Returns (mass f64[E, P], n_bad)
        or, with ``want_det``, (mass, n_bad, det f64[E, P]); ``n_bad`` counts the nodes whose determinant is not > 0."""
        deriv, weights = gll_derivative_matrix(shape_order), gll_weights_1d(shape_order)
        gp, nelem, P, dim = self._gll_points(shape_order, gll_points)
        mass = self.empty((nelem, P), np.float64)
        det = self._wanted(want_det, (nelem, P))
        d_d, w_d = self.to_device(deriv), self.to_device(weights)
        n_bad = self._call("mm_gll_mass", int(shape_order), dim, gp, nelem, d_d, w_d, mass, det)
        return (mass, int(n_bad), det) if want_det else (mass, int(n_bad))

    def weighted_sum(self, mass, fields=None):
        """``sum_i mass[i] * fields[c][i]`` -> f64[C] (NumPy), the volume integral of every field; ``fields=None``:
        f64[1], the sum of ``mass``.  mass f64[E, P] (any shape), fields f64[C, E, P] or the shape of ``mass`` (one
        field).  Deterministic, in the fixed order ``mm_weighted_sum`` states."""
        m = self.asdevice(mass, np.float64)
        f, ncomp = self._fields_over(m, fields)
        out = self.empty((ncomp,), np.float64)
        self._call("mm_weighted_sum", m, f, m.size, ncomp, out)
        return out.numpy()

    def multiply_rows(self, mass, values):
        """``mass[i] * values[c][i]`` for values f64[C, n] over the n values of mass (any shape): the plain product, one
        rounding (``mm_pcg_combine`` with ``tau = 0``).  Returns a new f64[C, n] on the device."""
        m = self.asdevice(mass, np.float64)
        v = self.asdevice(values, np.float64)
        if len(v.shape) != 2 or v.shape[1] != m.size:
            raise ValueError("values must be [C, n] over the n values of mass")
        out = self.empty(v.shape, np.float64)
        self._call("mm_pcg_combine", m, v, 0.0, None, m.size, v.shape[0], out)
        return out

    def divide_rows(self, num, den, out=None):
        """``num[c] / den`` for num f64[C, ...] over den's shape (or the shape of den); ``out`` may be ``num``."""
        a = self.asdevice(num, np.float64)
        d = self.asdevice(den, np.float64)
        if a.shape != d.shape and a.shape[1:] != d.shape:
            raise ValueError("num must be [C, ...] over the shape of den, or the shape of den")
        out = self._out(out, a.shape, "out must have the shape of num")
        self._call("mm_divide_rows", a, d, d.size, a.size // max(d.size, 1), out)
        return out

    # ---- radial 1-D profiles: bins, binned sums, a 1-D table on the nodes -----------------------------
    def radial_bins(self, points, edges, want_radius=False):
        """The radial bin of every point (``mm_radial_bins``): points f64[..., 3] (N points, read flat), edges
        f64[nbins + 1] strictly ascending and finite (``ValueError`` otherwise).  ``edges[b] <= |p| < edges[b + 1]``, the
        last edge belongs to the last bin, -1 outside the edges and for a NaN radius.  Returns (bin int32[N] on the device,
        number of -1 entries) or, with ``want_radius``, (bin, noutside, radius f64[N])."""
        pts, n = self._points3(points)
        e = self.asdevice(edges, np.float64)
        if len(e.shape) != 1 or e.shape[0] < 2:
            raise ValueError("edges must be 1-D with at least two entries")
        bins = self.empty((n,), np.int32)
        radius = self._wanted(want_radius, (n,))
        rc = self._call_args("mm_radial_bins", pts, n, e, e.shape[0] - 1, bins, radius)
        return (bins, int(rc), radius) if want_radius else (bins, int(rc))

    def binned_weighted_sum(self, mass, bins, nbins, fields=None, square=False, want_count=False):
        """``out[c][b] = sum over bins[i] == b of mass[i] * fields[c][i]`` (``square``: ``(mass * f) * f``) for all bins in
        one pass per component (``mm_binned_weighted_sum``): deterministic, in the fixed order include/multimesh_hip.h
        states.  mass f64[...] (any shape, N values), bins int32[N] (entries outside [0, nbins) belong to no bin), fields
        f64[C, ...] over the shape of mass, the shape of mass (one field), or None: the sum of the mass per bin.  Returns
        f64[C, nbins] (NumPy) or, with ``want_count``, (sums, count int64[nbins])."""
        m = self.asdevice(mass, np.float64)
        b = self.asdevice(bins, np.int32)
        if b.size != m.size:
            raise ValueError("bins must hold one entry per value of mass")
        nbins = int(nbins)
        if nbins < 1:
            raise ValueError("nbins must be at least 1")
        f, ncomp = self._fields_over(m, fields)
        out = self.empty((ncomp, nbins), np.float64)
        count = self._wanted(want_count, (nbins,), np.int64)
        self._call("mm_binned_weighted_sum", m, f, b, m.size, ncomp, nbins, bool(square), out, count)
        return (out.numpy(), count.numpy()) if want_count else out.numpy()

    def radial_model_apply(self, points, radius, values, mode=0, values_in=None, out=None):
        """A 1-D table evaluated on the nodes (``mm_radial_model_apply``): points f64[G, P, 3] (P nodes per element, at
        most 256; the element's centre picks the layer) or f64[N, 3] (P = 1), radius f64[m] ascending with a repeated
        radius at every discontinuity, values f64[C, m] (or f64[m]).  ``mode`` 0: the table's value ``ref``; with
        ``values_in`` f64[C, G * P] (any shape of that size): 1 ``in - ref``, 2 ``(in - ref) / ref``, 3 ``in + ref``,
        4 ``ref + in * ref``.  ``out`` may be ``values_in``.  Returns f64[C, G, P] (or [C, N]) on the device.  A table
        that is not a set of layers raises ``ValueError``."""
        pts, ngroups, P = self._node_groups(points)
        r = self.asdevice(radius, np.float64)
        v = self.asdevice(values, np.float64)
        if len(r.shape) != 1 or v.shape[-1:] != r.shape or len(v.shape) > 2:
            raise ValueError("radius must be [m] and values [C, m] (or [m])")
        ncomp = v.shape[0] if len(v.shape) == 2 else 1
        if mode not in (0, 1, 2, 3, 4):
            raise ValueError("mode must be 0 .. 4")
        n = ngroups * P
        src = None
        if mode != 0:
            if values_in is None:
                raise ValueError("modes 1 to 4 need values_in")
            src = self.asdevice(values_in, np.float64)
            if src.size != ncomp * n:
                raise ValueError("values_in must hold one value per component and node")
        out = self._out(out, (ncomp,) + pts.shape[:-1], "out must hold one value per component and node", size_only=True)
        self._call_args("mm_radial_model_apply", pts, ngroups, P, r, v, r.shape[0], ncomp, int(mode), src, out)
        return out

    # ---- kernel preconditioning: the cut-out weight, order statistics, clipping -------------------------
    def point_taper(self, points, centres, inner, outer, values_in=None, out=None, want_weight=False):
        """The cut-out around ``centres`` (``mm_point_taper``): per node the least, over the centres, of a smoothstep of the
        distance -- 0 within ``inner[k]``, 1 beyond ``outer[k]`` -- times the values.  points f64[G, P, 3] (P nodes per
        element, at most 256) or f64[N, 3]; centres f64[K, 3], inner and outer f64[K] (K may be 0); ``values_in``
        f64[C, G * P] (any shape of that size per component, or one component of the points' shape) or None; ``out`` may
        be ``values_in``: elements that no centre reaches are then not written at all.  Returns (values f64[C, G, P] or
        [C, N] on the device, or None without ``values_in``; the number of nodes with weight < 1) and, with
        ``want_weight``, the weight f64[G, P] / [N] as a third entry.  Centres or radii that are not finite, a negative
        inner, an outer below its inner raise ``ValueError`` and nothing is written."""
        pts, ngroups, P = self._node_groups(points)
        c = self.asdevice(centres, np.float64)
        ri, ro = self.asdevice(inner, np.float64), self.asdevice(outer, np.float64)
        if len(c.shape) != 2 or c.shape[1] != 3 or ri.shape != (c.shape[0],) or ro.shape != (c.shape[0],):
            raise ValueError("centres must be [K, 3], inner and outer [K]")
        n = ngroups * P
        src, ncomp = None, 0
        if values_in is not None:
            src = self.asdevice(values_in, np.float64)
            ncomp = 1 if src.shape == pts.shape[:-1] else src.shape[0]
            if src.size != ncomp * n:
                raise ValueError("values_in must hold one value per component and node")
            out = self._out(out, (ncomp,) + pts.shape[:-1], "out must hold one value per component and node", size_only=True)
        elif out is not None:
            raise ValueError("out without values_in")
        elif not want_weight:
            raise ValueError("ask for the weight or pass values_in")
        weight = self._wanted(want_weight, pts.shape[:-1])
        rc = self._call_args("mm_point_taper", pts, ngroups, P, c, ri, ro, c.shape[0], ncomp, src, out, weight)
        return (out, int(rc), weight) if want_weight else (out, int(rc))

    def order_statistics(self, values, q, absolute=False, method="lower"):
        """Exact order statistics (``mm_order_statistics``): values f64[C, ...] (every row read flat) or f64[n] (one row),
        q f64[m] in [0, 1], 1 <= m <= 16.  NaNs are left out; of the ``nvalid`` others (``absolute``: of their absolute
        values) the one of rank ``floor(q * (nvalid - 1))`` (``method="lower"``) or ``ceil`` (``"higher"``) in the numeric
        order, -0.0 before +0.0; NaN for a row without a valid value.  Returns (out f64[C, m], nvalid int64[C]), both on
        the device: nothing is read back."""
        v, ncomp, n = self._flat_rows(values, "values must be [C, ...] or [n]")
        if method not in ("lower", "higher"):
            raise ValueError('method must be "lower" or "higher"')
        if not isinstance(q, DeviceArray):
            q = np.atleast_1d(np.asarray(q, dtype=np.float64))
            if q.ndim != 1 or not 1 <= q.size <= 16 or not ((q >= 0.0) & (q <= 1.0)).all():
                raise ValueError("q must hold between 1 and 16 values in [0, 1]")
        qd = self.asdevice(q, np.float64)
        m = qd.size
        out = self.empty((ncomp, m), np.float64)
        nvalid = self.empty((ncomp,), np.int64)
        self._call_args("mm_order_statistics", v, n, ncomp, bool(absolute), qd, m, method != "lower", out, nvalid)
        return out, nvalid

    def clamp(self, values, lower=None, upper=None, symmetric=False, out=None, want_count=True):
        """``v < lo ? lo : (v > hi ? hi : v)`` (``mm_clamp``) for values f64[C, ...] (every row read flat) or f64[n] with
        bounds f64[C] that are on the device already (a :class:`DeviceArray`, such as a column of
        :meth:`order_statistics`) or are copied there; None: no bound on that side; ``symmetric``: ``lower`` must be None
        and is ``-upper``.  A NaN passes through, -0.0 is kept.  ``out`` may be ``values``.  Returns (out on the device,
        changed int64[C] on the device -- the number of values replaced -- or None without ``want_count``)."""
        v, ncomp, n = self._flat_rows(values, "values must be [C, ...] or [n]")
        if symmetric and (lower is not None or upper is None):
            raise ValueError("symmetric takes upper alone")
        lo = None if lower is None else self.asdevice(lower, np.float64)
        hi = None if upper is None else self.asdevice(upper, np.float64)
        for b in (lo, hi):
            if b is not None and b.size != ncomp:
                raise ValueError("a bound per component")
        out = self._out(out, v.shape, "out must hold one value per value", size_only=True)
        changed = self._wanted(want_count, (ncomp,), np.int64)
        self._call_args("mm_clamp", v, n, ncomp, lo, hi, bool(symmetric), out, changed)
        return out, changed

    # ---- boundaries: faces, their side and nodes, the distance to them, the taper and blend it drives ------
    def _faces(self, faces, nelem, side=None):
        """(faces int64[nb] on the device, side int32[nb] or None, nb), checked against ``nelem`` elements."""
        fd = self.asdevice(faces, np.int64)
        if len(fd.shape) != 1 or fd.shape[0] > 6 * nelem:
            raise ValueError("faces must be 1-D with at most 6 * nelem codes")
        sd = None if side is None else self.asdevice(side, np.int32)
        if sd is not None and sd.shape != fd.shape:
            raise ValueError("side must hold one entry per face")
        return fd, sd, fd.shape[0]

    def boundary_faces(self, corner_ids, nnodes):
        """The boundary faces of a hexahedral mesh (``mm_boundary_faces``): corner_ids int64[E, 8] in tensor order
        (corner ``i + 2 j + 4 k``), every id in [0, nnodes).  A face is a boundary face when its four sorted ids occur once
        among all 6 E faces.  Returns (codes ``6 e + f`` int64[nb] ascending, on the device; the number of faces whose ids
        occur more than twice -- not zero: the mesh is not a manifold).  An id out of range raises ``ValueError``."""
        ids = self.asdevice(corner_ids, np.int64)
        if len(ids.shape) != 2 or ids.shape[1] != 8:
            raise ValueError("corner_ids must be [E, 8]")
        nnodes = int(nnodes)
        if not 0 <= nnodes < 1 << 31 or ids.shape[0] >= 1 << 27:
            raise ValueError("nnodes must lie in [0, 2^31) and E below 2^27")
        faces = self.empty((6 * ids.shape[0],), np.int64)
        info = self.empty((1,), np.int64)
        rc = self._call_args("mm_boundary_faces", ids, ids.shape[0], nnodes, faces, info)
        return faces.rows(0, int(rc)), int(info.numpy()[0])

    def boundary_classify(self, corners, faces, up=None, cos_min=0.5):
        """Top (1), bottom (2) or lateral side (0) of every boundary face (``mm_boundary_classify``): corners f64[E, 8, 3]
        in tensor order, faces int64[nb] codes.  ``up=None``: radial, the direction of the face's centre in Earth-centred
        coordinates; else a vector (x, y, z).  A face is top when the cosine between its outward normal and up is at least
        ``cos_min`` (in (0, 1]), bottom when it is at most ``-cos_min``.  Returns int32[nb] on the device."""
        c = self.asdevice(corners, np.float64)
        if len(c.shape) != 3 or c.shape[1:] != (8, 3):
            raise ValueError("corners must be [E, 8, 3]")
        fd, _, nb = self._faces(faces, c.shape[0])
        if not 0.0 < float(cos_min) <= 1.0:
            raise ValueError("cos_min must lie in (0, 1]")
        u = (0.0, 0.0, 0.0)
        if up is not None:
            u = tuple(float(v) for v in np.asarray(up, dtype=np.float64).reshape(-1))
            if len(u) != 3 or not np.isfinite(u).all() or not any(u):
                raise ValueError("up must be three finite numbers, not all zero")
        side = self.empty((nb,), np.int32)
        self._call_args("mm_boundary_classify", c, c.shape[0], fd, nb, up is None, u[0], u[1], u[2], float(cos_min), side)
        return side

    def boundary_nodes(self, points, shape_order, faces, side=None, side_mask=7):
        """The nodes of the boundary faces whose side is in ``side_mask`` (bit ``1 << side``; ``mm_boundary_nodes``):
        points f64[E, (order+1)^3, 3], order 1, 2 or 4; faces int64[nb], side int32[nb] (None: every face).  Face by face in
        the order of ``faces``, ascending node index within a face; a node shared by two faces appears twice.  Returns
        f64[K, 3] on the device, K = (order+1)^2 per selected face."""
        pts = self.asdevice(points, np.float64)
        order = int(shape_order)
        if order not in (1, 2, 4):
            raise ValueError("shape_order must be 1, 2 or 4")
        if len(pts.shape) != 3 or pts.shape[1:] != ((order + 1) ** 3, 3):
            raise ValueError("points must be [E, (order+1)^3, 3]")
        fd, sd, nb = self._faces(faces, pts.shape[0], side)
        if not 0 <= int(side_mask) <= 7:
            raise ValueError("side_mask must lie in [0, 7]")
        out = self.empty((nb * (order + 1) ** 2, 3), np.float64)
        rc = self._call_args("mm_boundary_nodes", pts, pts.shape[0], order, fd, sd, nb, int(side_mask), out)
        return out.rows(0, int(rc))

    def cutoff_distance(self, points, sources, cutoff):
        """``min(cutoff, min over the sources of |x - s|)`` for points f64[..., 3] and sources f64[K, 3]
        (``mm_cutoff_distance``): bit for bit the brute-force minimum, by a cell grid whose edge is just above ``cutoff``;
        points far from every source cost O(1).  A point with a NaN coordinate keeps ``cutoff``.  Returns (distance f64 of
        the points' leading shape, on the device; the number of points with distance < cutoff).  A cutoff that is not
        positive and finite, or a source that is not finite, raises ``ValueError``."""
        pts, n = self._points3(points)
        s = self.asdevice(sources, np.float64)
        if len(s.shape) != 2 or s.shape[1] != 3:
            raise ValueError("sources must be [K, 3]")
        cutoff = float(cutoff)
        if not (np.isfinite(cutoff) and cutoff > 0.0):
            raise ValueError("cutoff must be positive and finite")
        dist = self.empty(pts.shape[:-1], np.float64)
        rc = self._call_args("mm_cutoff_distance", pts, n, s, s.shape[0], cutoff, dist)
        return dist, int(rc)

    def distance_taper(self, dist, inner, outer, a, b=None, elem=None, out=None, want_weight=False):
        """Taper or blend by a distance (``mm_distance_taper``): ``w`` = 0 for ``dist <= inner``, 1 for ``dist >= outer``,
        the smoothstep ``s*s*(3 - 2*s)`` between them, and 0 where ``elem`` (int64, one per node) is negative.  ``a``
        f64[C, ...] over the shape of ``dist`` (or that shape: one component), or None with ``want_weight``; ``b`` None:
        ``out = w * a``; else ``out = b`` where w == 0, ``a`` where w == 1, ``(w * a) + ((1 - w) * b)`` between.  ``out`` may be
        ``a`` or ``b``.  Returns (out on the device or None, the number of nodes with w < 1) and, with ``want_weight``, the
        weight as a third entry.  ``0 <= inner <= outer``, finite (``ValueError`` otherwise)."""
        d = self.asdevice(dist, np.float64)
        inner, outer = float(inner), float(outer)
        if not (np.isfinite(inner) and np.isfinite(outer) and 0.0 <= inner <= outer):
            raise ValueError("the radii need 0 <= inner <= outer, both finite")
        n = d.size
        av, bv, ncomp = None, None, 0
        if a is not None:
            av = self.asdevice(a, np.float64)
            ncomp = 1 if av.shape == d.shape else av.shape[0]
            if av.size != ncomp * n:
                raise ValueError("a must hold one value per component and node")
            if b is not None:
                bv = self.asdevice(b, np.float64)
                if bv.size != av.size:
                    raise ValueError("b must hold one value per value of a")
            out = self._out(out, (ncomp,) + d.shape, "out must hold one value per component and node", size_only=True)
        elif b is not None or out is not None:
            raise ValueError("b or out without a")
        elif not want_weight:
            raise ValueError("ask for the weight or pass a")
        ev = None if elem is None else self.asdevice(elem, np.int64)
        if ev is not None and ev.size != n:
            raise ValueError("elem must hold one entry per node")
        weight = self._wanted(want_weight, d.shape)
        rc = self._call_args("mm_distance_taper", d, n, inner, outer, ncomp, av, bv, ev, out, weight)
        return (out, int(rc), weight) if want_weight else (out, int(rc))

    # ---- scattered models: kNN rows -> inverse-distance values ------------------------------------------
    def idw_gather(self, fields, idx, dist, power=2, max_distance=np.inf, outside="fill", fill_value=np.nan, out=None,
                   point_major=False, want_nearest=False, want_count=False):
        """The rows of a kNN query turned into values (``mm_idw_gather``): ``fields`` f64[C, nsrc] (or [nsrc]), ``idx``
        int64[N, k] and ``dist`` f64[N, k] as :meth:`KnnIndex.query` gives them with ``want_dist`` (any contents are
        served).  An entry is valid when its index lies in [0, nsrc) and its distance is ``<= max_distance``; with ``d0``
        the first valid distance the weights are ``(d0 / d) ** power`` by repeated multiplication (``power`` an integer in
        1..8), the value is ``sum(w * v) / sum(w)`` summed in the row's order from 0.0, and a valid entry at distance 0.0
        (the first such) gives its sample's bits instead.  A target without a valid entry is outside: ``outside`` "fill"
        writes ``fill_value``, "keep" leaves the entries of ``out``, which is then required.  Returns (values f64[C, N] --
        [N, C] with ``point_major`` --, the number of outside targets) and then, as asked for, ``nearest`` f64[N] (``d0``,
        +inf outside) and ``nused`` int32[N] (the valid entries), all on the device.  include/multimesh_hip.h states the
        arithmetic, and the values are bit for bit that statement."""
        modes = {"fill": 0, "keep": 2}
        if outside not in modes:
            raise ValueError(f"outside must be one of {sorted(modes)}, got {outside!r}")
        if isinstance(power, bool) or not isinstance(power, (int, np.integer)) or not 1 <= power <= 8:
            raise ValueError(f"power must be an integer in 1..8, got {power!r}")
        max_distance = float(max_distance)
        if not max_distance >= 0.0:
            raise ValueError("max_distance must not be negative or a NaN (inf: no limit)")
        f = _components(self.asdevice(fields, np.float64), 1)
        idv, d, n, k = self._pairs(idx, dist)
        if len(f.shape) != 2:
            raise ValueError("fields must be [C, nsrc] (or [nsrc])")
        if not 1 <= k <= MM_KNN_MAX_K:
            raise ValueError(f"k must be in 1..{MM_KNN_MAX_K}")
        ncomp, nsrc = f.shape
        shape = _major(n, ncomp, point_major)
        if out is None and outside == "keep":
            raise ValueError('outside="keep" keeps the entries of out: pass out')
        out = self._out(out, shape, f"out must be {list(shape)}")
        nearest = self._wanted(want_nearest, (n,))
        nused = self._wanted(want_count, (n,), np.int32)
        rc = self._call_args("mm_idw_gather", f, nsrc, ncomp, idv, d, n, k, int(power), max_distance, modes[outside],
                             float(fill_value), out, bool(point_major), nearest, nused)
        return (out, int(rc)) + ((nearest,) if want_nearest else ()) + ((nused,) if want_count else ())

    # ---- resolution: node spacing, edge lengths, the time step and the resolved period of a model ------
    def gll_resolution(self, shape_order, gll_points, fast=None, slow=None, want_node_spacing=False):
        """The sizes of every element of gll_points f64[E, (order+1)^dim, dim], orders 1, 2, 4, and what a model makes of
        them (``mm_gll_resolution``: bit for bit the NumPy statement of include/multimesh_hip.h).  ``fast`` f64[nfast, E, P]
        (or [E, P]) and ``slow`` f64[nslow, E, P] are the velocities; ``slow`` needs ``fast``.  Returns (out, info), both on
        the device and nothing read back: out f64[5, E] = spacing, edge_min, edge_max, step, period -- f64[3, E] without
        ``fast`` --, info int64[2] = the geometry-invalid and the model-invalid elements, whose entries are NaN.  The edges
        are corner-to-corner chords, not arcs.  With ``want_node_spacing`` a third entry: h f64[E, P], every node's least
        distance to its tensor-line neighbours."""
        gp, nelem, P, dim = self._gll_points(shape_order, gll_points)
        f = None if fast is None else _element_nodal(self, fast, nelem, P, "fast")
        s = None if slow is None else _element_nodal(self, slow, nelem, P, "slow")
        out = self.empty((5 if f else 3, nelem), np.float64)
        info = self.empty((2,), np.int64)
        node_h = self._wanted(want_node_spacing, (nelem, P))
        self._call_args("mm_gll_resolution", int(shape_order), dim, gp, nelem, f, f.shape[0] if f else 0, s,
                        s.shape[0] if s else 0, node_h, out, info)
        return (out, info, node_h) if want_node_spacing else (out, info)

    def arg_extreme(self, values, want_max=False):
        """The least (``want_max``: greatest) value of every row of values f64[R, ...] (every row read flat) or f64[n] (one
        row) that is not a NaN, and its place (``mm_arg_extreme``): the lowest index among equal values, -0.0 equal to
        +0.0, NaN and -1 for a row without a valid value.  Returns (value f64[R], index int64[R], nvalid int64[R]), all on
        the device: nothing is read back.  Deterministic (integer atomics only)."""
        v, nrows, n = self._flat_rows(values, "values must be [R, ...] or [n]")
        value = self.empty((nrows,), np.float64)
        index, nvalid = self.empty((nrows,), np.int64), self.empty((nrows,), np.int64)
        self._call_args("mm_arg_extreme", v, nrows, n, bool(want_max), value, index, nvalid)
        return value, index, nvalid

    # ---- diffusion: the stiffness operator and the smoothing it gives -------------------------------
    def diffusion(self, shape_order, gll_points, kappa_h=1.0, kappa_r=None):
        """A :class:`Diffusion` over gll_points f64[E, (order+1)^dim, dim], orders 1, 2, 4: ``apply(u)`` is the bare
        ``K u``, ``smooth(values, ...)`` the diffusion steps.  ``kappa_h`` / ``kappa_r``: the lateral and the radial
        diffusivity, each a number or an element-nodal array f64[E, P]; ``kappa_r=None``: isotropic (``kappa_h`` in every
        direction; the only choice in 2-D).  A scalar is passed to the kernel as a scalar, never made an array."""
        deriv, weights = gll_derivative_matrix(shape_order), gll_weights_1d(shape_order)
        gp, _, _, dim = self._gll_points(shape_order, gll_points)
        if kappa_r is not None and dim != 3:
            raise ValueError("a radial diffusivity needs a 3-D mesh")

        def kappa(k, name):
            if isinstance(k, (DeviceArray,)) or (hasattr(k, "data_ptr") and hasattr(k, "shape")):
                arr = self.asdevice(k, np.float64)
                if arr.shape != gp.shape[:2]:
                    raise ValueError(f"{name} must be a number or an array [E, P]")
                return 1.0, arr
            k = np.asarray(k, dtype=np.float64)
            if not np.isfinite(k).all() or (k < 0).any():
                raise ValueError(f"{name} must be finite and >= 0")
            if k.ndim == 0:
                return float(k), None
            if k.shape != gp.shape[:2]:
                raise ValueError(f"{name} must be a number or an array [E, P]")
            return 1.0, self.to_device(k)

        return Diffusion(self, shape_order, gp, kappa(kappa_h, "kappa_h"),
                         None if kappa_r is None else kappa(kappa_r, "kappa_r"),
                         (self.to_device(deriv), self.to_device(weights)))

    # ---- the gradient of element-nodal fields ------------------------------------------------------
    def gll_gradient(self, shape_order, gll_points, u, grad=True, radial=False, lateral=False, norm=False):
        """The spatial gradient of u f64[C, E, P] (or [E, P]) over gll_points f64[E, (order+1)^dim, dim], orders 1, 2, 4,
        per element and not assembled (``mm_gll_gradient``: bit for bit the NumPy statement of include/multimesh_hip.h).
        Returns the requested device arrays in the order of the flags -- ``grad`` f64[C, dim, E, P], ``radial`` (the
        derivative along x / |x|), ``lateral`` (the norm of what is left of the gradient) and ``norm``, each f64[C, E, P] --
        as a tuple, or the array itself when one is asked for.  ``radial`` and ``lateral`` need a 3-D mesh."""
        deriv = gll_derivative_matrix(shape_order)
        gp, nelem, P, dim = self._gll_points(shape_order, gll_points)
        if not (grad or radial or lateral or norm):
            raise ValueError("ask for at least one of grad, radial, lateral and norm")
        if (radial or lateral) and dim != 3:
            raise ValueError("the radial / lateral split needs a 3-D mesh")
        v = _element_nodal(self, u, nelem, P, "u")
        ncomp = v.shape[0]
        outs = [self._wanted(want, (ncomp, dim, nelem, P) if full else (ncomp, nelem, P))
                for want, full in ((grad, True), (radial, False), (lateral, False), (norm, False))]
        d_d = self.to_device(deriv)
        self._call("mm_gll_gradient", int(shape_order), dim, gp, nelem, d_d, v, ncomp, *outs)
        got = tuple(o for o in outs if o is not None)
        return got[0] if len(got) == 1 else got

    # ---- the order of element-nodal values, changed on their own mesh ---------------------------------
    def gll_tensor_apply(self, order_in, order_out, dim, values, layout=0, transpose=False, scale_in=None, div_out=None,
                         out=None):
        """Element-nodal values from the GLL nodes of ``order_in`` to those of ``order_out`` on the same elements, orders 1,
        2, 4, different (``mm_gll_tensor_apply``: bit for bit the NumPy statement of include/multimesh_hip.h).  ``values``
        by ``layout``: 0 = f64[C, E, P_in] (or [E, P_in]), 1 = f64[E, P_in, C] (coordinates), 2 = f64[E, C, P_in]
        (``MODEL/data``); the result has the same layout with P_out.  The table is the interpolation
        :func:`multimesh_amd.synth.gll_order_table` or, with ``transpose``, the transpose of the interpolation
        ``order_out -> order_in``.  ``scale_in`` f64[E, P_in] multiplies the input, ``div_out`` f64[E, P_out] divides the
        output (both nullable, shared by the components)."""
        order_in, order_out, dim, layout = int(order_in), int(order_out), int(dim), int(layout)
        table = (np.ascontiguousarray(gll_order_table(order_out, order_in).T) if transpose
                 else gll_order_table(order_in, order_out))
        if order_in == order_out:
            raise ValueError("order_in equals order_out: nothing to resample")
        if dim not in (2, 3) or layout not in (0, 1, 2):
            raise ValueError("dim must be 2 or 3 and layout 0 ([C, E, P]), 1 ([E, P, C]) or 2 ([E, C, P])")
        pin, pout = (order_in + 1) ** dim, (order_out + 1) ** dim
        v = self.asdevice(values, np.float64)
        if layout == 0:
            v = _components(v, 2)
        if len(v.shape) != 3 or v.shape[(2, 1, 2)[layout]] != pin:
            raise ValueError(f"values must hold {pin} nodes per element in layout {layout}, got shape {v.shape}")
        ncomp, nelem = ((v.shape[0], v.shape[1]), (v.shape[2], v.shape[0]), (v.shape[1], v.shape[0]))[layout]
        shape = ((ncomp, nelem, pout), (nelem, pout, ncomp), (nelem, ncomp, pout))[layout]
        scale = div = None
        if scale_in is not None:
            scale = self.asdevice(scale_in, np.float64)
            if scale.shape != (nelem, pin):
                raise ValueError(f"scale_in must be [{nelem}, {pin}]")
        if div_out is not None:
            div = self.asdevice(div_out, np.float64)
            if div.shape != (nelem, pout):
                raise ValueError(f"div_out must be [{nelem}, {pout}]")
        out = self._out(out, shape, f"out must be {shape}")
        t_d = self.to_device(table)
        self._call("mm_gll_tensor_apply", dim, order_in, order_out, t_d, layout, v, out, nelem, ncomp, scale, div)
        return out

    def element_deviation(self, a, b):
        """Per element of two f64[E, P, dim] coordinate arrays of the same elements: (deviation f64[E], edge f64[E]) = the
        largest ``|a - b|`` of the element (NaN where a difference is) and the largest bounding-box edge of ``b``
        (``mm_element_deviation``, include/multimesh_hip.h)."""
        a, b = self.asdevice(a, np.float64), self.asdevice(b, np.float64)
        if len(a.shape) != 3 or a.shape[2] not in (2, 3) or a.shape[1] < 1 or b.shape != a.shape:
            raise ValueError(f"a and b must both be [nelem, P, dim] with dim 2 or 3, got {a.shape} and {b.shape}")
        nelem, npts, dim = a.shape
        deviation, edge = self.empty((nelem,), np.float64), self.empty((nelem,), np.float64)
        self._call("mm_element_deviation", dim, npts, a, b, nelem, deviation, edge)
        return deviation, edge

    # ---- fused ---------------------------------------------------------------------------
    def interpolate_gll(self, shape_order, gll_points, points, element_nodal_fields, nelem_to_search=20,
                        tolerance=1.05, snap_to_nearest=False, want_operator=False, out=None):
        """The GLL form of the whole path (reference interpolator.py:931-977) on resident arrays:
        gll_points f64[E, P, dim], points f64[N, dim], element_nodal_fields f64[C, E, P].
        Returns (values f64[N, C], nmissing) or (values, elem int64[N], coeffs f64[N, P], nmissing)."""
        gp = self.asdevice(gll_points, np.float64)
        pts = self.asdevice(points, np.float64)
        f = _components(self.asdevice(element_nodal_fields, np.float64), 2)
        nelem, P, dim = gp.shape
        if P != (shape_order + 1) ** dim or len(pts.shape) != 2 or pts.shape[1] != dim:
            raise ValueError("gll_points must be [nelem, (order+1)^dim, dim] and points [N, dim]")
        if f.shape[1:] != (nelem, P):
            raise ValueError("element_nodal_fields must be [C, nelem, P]")
        n, ncomp = pts.shape[0], f.shape[0]
        out = self._out(out, (n, ncomp), "out must be [N, C]")
        elem = self._wanted(want_operator, (n,), np.int64)
        coeffs = self._wanted(want_operator, (n, P))
        miss = self._call("mm_interpolate_gll", shape_order, dim, gp, nelem, pts, n, f, ncomp, nelem_to_search,
                          float(tolerance), bool(snap_to_nearest), out, elem, coeffs)
        return _with_operator(want_operator, out, elem, coeffs, miss)

    def sample_columns_gll(self, shape_order, gll_points, element_nodal_fields, lat_table, lon_table, radius,
                           paired=False, nelem_to_search=25, tolerance=1.05, fill_value=np.nan, chunk_points=None,
                           want_points=False, out=None):
        """A 3-D GLL model sampled on latitude x longitude x radius columns, the targets generated on the device
        (``mm_sample_columns_gll``).  ``lat_table`` f64[nlat, 2] = (sin colat, cos colat), ``lon_table`` f64[nlon, 2]
        = (cos lon, sin lon), ``radius`` f64[D]; columns are the nlat x nlon grid (latitude outer) or, with
        ``paired``, the path of latitude h with longitude h.  Every target's value is what :meth:`interpolate_gll`
        gives for the same point; targets without an element hold ``fill_value``.  ``chunk_points``: targets per
        chunk (None: the library's byte budget).
        Returns (values f64[C, D, H], nmissing) or, with ``want_points``, (values, nmissing, points f64[D, H, 3])."""
        gp = self.asdevice(gll_points, np.float64)
        f = _components(self.asdevice(element_nodal_fields, np.float64), 2)
        lat = self.asdevice(lat_table, np.float64)
        lon = self.asdevice(lon_table, np.float64)
        rad = self.asdevice(radius, np.float64)
        if len(gp.shape) != 3 or gp.shape[2] != 3 or gp.shape[1] != (shape_order + 1) ** 3:
            raise ValueError("gll_points must be [nelem, (order+1)^3, 3]")
        nelem, P, _ = gp.shape
        if f.shape[1:] != (nelem, P):
            raise ValueError("element_nodal_fields must be [C, nelem, P]")
        if len(lat.shape) != 2 or lat.shape[1] != 2 or len(lon.shape) != 2 or lon.shape[1] != 2 or len(rad.shape) != 1:
            raise ValueError("lat_table and lon_table must be [n, 2], radius [D]")
        nlat, nlon, nd = lat.shape[0], lon.shape[0], rad.shape[0]
        if paired and nlat != nlon:
            raise ValueError("a path pairs latitude h with longitude h: lat_table and lon_table need the same length")
        if chunk_points is not None and int(chunk_points) < 1:
            raise ValueError("chunk_points must be >= 1 (or None)")
        ncol = nlat if paired else nlat * nlon
        ncomp = f.shape[0]
        out = self._out(out, (ncomp, nd, ncol), "out must be [C, D, H]")
        pts = self._wanted(want_points, (nd, ncol, 3))
        miss = self._call("mm_sample_columns_gll", int(shape_order), gp, nelem, f, ncomp, lat, nlat, lon, nlon, bool(paired),
                          rad, nd, int(nelem_to_search), float(tolerance), float(fill_value), int(chunk_points or 0), out,
                          pts)
        return (out, int(miss), pts) if want_points else (out, int(miss))

    def sample_grid(self, points, grid_values, depth, lat, lon, outside="fill", fill_value=np.nan, lon_periodic=False,
                    out=None, want_latlondepth=False):
        """A regular grid sampled at points (``mm_sample_grid``): ``points`` f64[..., 3] (N points, read flat),
        ``grid_values`` f64[C, D, LA, LO] (or [D, LA, LO]) over the strictly ascending axes ``depth`` f64[D] (m below
        6371 km), ``lat`` f64[LA] (geocentric degrees) and ``lon`` f64[LO] (degrees; host axes are checked here, device
        axes are the caller's word).  Trilinear, every operation rounded as include/multimesh_hip.h states; a NaN
        corner makes the values of its cell NaN.  ``outside``: "fill" (``fill_value``), "clamp" (the edge value
        extends) or "keep" (``out``, which is then required, keeps its entries).  ``lon_periodic``: the longitude is
        wrapped into [lon[0], lon[0] + 360), and the axis must start in [-360, 180] and end at ``lon[0] + 360``.
        Returns (values f64[C, N], number of points outside the grid) or, with ``want_latlondepth``, (values,
        nmissing, latlondepth f64[N, 3]) -- the (lat, lon, depth) the device computed."""
        modes = {"fill": 0, "clamp": 1, "keep": 2}
        if outside not in modes:
            raise ValueError(f"outside must be one of {sorted(modes)}, got {outside!r}")
        pts, n = self._points3(points)
        g = _components(self.asdevice(grid_values, np.float64), 3)
        d, la, lo = self._grid_axes(depth, lat, lon, lon_periodic)
        if len(g.shape) != 4 or g.shape[1:] != (d.shape[0], la.shape[0], lo.shape[0]):
            raise ValueError(f"grid_values must be [C, {d.shape[0]}, {la.shape[0]}, {lo.shape[0]}] over the axes, got {g.shape}")
        ncomp = g.shape[0]
        if out is None:
            if outside == "keep":
                raise ValueError('outside="keep" keeps the entries of out: pass out')
            out = self.empty((ncomp, n), np.float64)
        else:
            out = self.asdevice(out, np.float64)
            if len(out.shape) < 2 or out.shape[0] != ncomp or out.size != ncomp * n:
                raise ValueError("out must be [C, N] (or [C, ...] over the leading shape of points)")
        lld = self._wanted(want_latlondepth, (n, 3))
        miss = self._call("mm_sample_grid", pts, n, d, d.shape[0], la, la.shape[0], lo, lo.shape[0], g, ncomp,
                          bool(lon_periodic), modes[outside], float(fill_value), out, lld)
        return (out, int(miss), lld) if want_latlondepth else (out, int(miss))

    def _grid_axes(self, depth, lat, lon, lon_periodic):
        """The three axes of a regular grid on the device.  Host axes are checked here (1-D, finite, strictly ascending; a
        periodic longitude axis starts in [-360, 180] and ends at ``lon[0] + 360``), device axes are the caller's word."""
        axes = []
        for name, a in (("depth", depth), ("lat", lat), ("lon", lon)):
            if isinstance(a, np.ndarray) or not hasattr(a, "data_ptr"):
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.ndim != 1 or a.size < 1 or not np.isfinite(a).all() or not (np.diff(a) > 0).all():
                    raise ValueError(f"the {name} axis must be 1-D, finite and strictly ascending")
                if name == "lon" and lon_periodic and (not -360.0 <= a[0] <= 180.0 or a[-1] != a[0] + 360.0):
                    raise ValueError("a periodic lon axis must start in [-360, 180] and end at lon[0] + 360")
            a = self.asdevice(a, np.float64)
            if len(a.shape) != 1 or a.shape[0] < 1:
                raise ValueError(f"the {name} axis must be 1-D with at least one node")
            axes.append(a)
        return axes

    def grid_operator(self, points, depth, lat, lon, clamp=False, lon_periodic=False, latlondepth=False, ids_out=None,
                      weights_out=None):
        """The grid import of :meth:`sample_grid` as an operator (``mm_grid_operator``): for ``points`` f64[..., 3] (N
        points, read flat) over the axes ``depth``, ``lat``, ``lon`` (checked as :meth:`sample_grid` checks them), the
        flat indices ``(k * LA + j) * LO + i`` of the eight corners of every point's cell and their trilinear weights,
        corner ``c = 4 a + 2 b + e`` over (depth, latitude, longitude), bit for bit the statement of
        include/multimesh_hip.h.  ``gather(cube.reshape(C, -1), ids, w)`` imports a cube, ``transpose_nodes(ids, w,
        D * LA * LO)`` is the way back.  ``clamp=False``: a point outside the grid gets ids 0 and weights +0.0 and is
        counted; ``clamp=True``: the edge extends and nothing is outside.  ``ids_out`` / ``weights_out``: the caller's
        i64[N, 8] / f64[N, 8] to write into.  Returns (ids i64[N, 8], w f64[N, 8], noutside) or, with ``latlondepth``,
        (ids, w, noutside, latlondepth f64[N, 3])."""
        pts, n = self._points3(points)
        d, la, lo = self._grid_axes(depth, lat, lon, lon_periodic)
        ids = self.empty((n, 8), np.int64) if ids_out is None else self.asdevice(ids_out, np.int64)
        w = self.empty((n, 8), np.float64) if weights_out is None else self._out(weights_out, (n, 8))
        if ids.shape != (n, 8) or w.shape != (n, 8):
            raise ValueError("ids_out must be i64[N, 8] and weights_out f64[N, 8]")
        lld = self._wanted(latlondepth, (n, 3))
        miss = self._call("mm_grid_operator", pts, n, d, d.shape[0], la, la.shape[0], lo, lo.shape[0], bool(lon_periodic),
                          bool(clamp), ids, w, lld)
        return (ids, w, int(miss), lld) if latlondepth else (ids, w, int(miss))

    def interpolate_hex8(self, nodes, connectivity, points, fields, nelem_to_search=20, want_operator=False,
                         out=None):
        """The whole hot path of reference scripts/cli.py:62-100 on resident arrays.
        connectivity is the mesh's own (exodus-order) hex8 connectivity.
        Returns (values f64[N,C], nfailed) or (values, enc, weights, nfailed)."""
        nod = self.asdevice(nodes, np.float64)
        conn = self.asdevice(connectivity, np.int64)
        pts, f, out, enc, w = _hex8_arrays(self, nod.shape[0], points, fields, want_operator, out)
        nf = self._call("mm_interpolate_hex8", nod, nod.shape[0], conn, conn.shape[0], pts, pts.shape[0], f, f.shape[0],
                        nelem_to_search, out, enc, w)
        return _with_operator(want_operator, out, enc, w, nf)

    def source(self, nodes, connectivity):
        """Keep a hex8 source mesh resident (centroids + search grid built once): :class:`Source`."""
        nod = self.asdevice(nodes, np.float64)
        conn = self.asdevice(connectivity, np.int64)
        return Source(self, self._create("mm_source_create", nod, nod.shape[0], conn, conn.shape[0]), nod, conn)

    def interpolate_hex8_host(self, nodes, connectivity, points, fields, nelem_to_search=20, want_operator=False,
                              out=None):
        """:meth:`interpolate_hex8` for NumPy arrays on the host (reference scripts/cli.py:62-100 holds
        nothing else): uploads overlapped with the kernels, device copies cached in the context.
        Returns NumPy arrays: (values f64[N,C], nfailed) or (values, enc, weights, nfailed)."""
        nod = np.ascontiguousarray(nodes, dtype=np.float64)
        conn = np.ascontiguousarray(connectivity, dtype=np.int64)
        pts = np.ascontiguousarray(points, dtype=np.float64)
        f = np.ascontiguousarray(fields, dtype=np.float64)
        if f.ndim == 1:
            f = f[None]
        if nod.ndim != 2 or nod.shape[1] != 3 or conn.ndim != 2 or conn.shape[1] != 8 or pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("need nodes[M,3], connectivity[E,8], points[N,3]")
        if f.shape[1] != nod.shape[0]:
            raise ValueError("fields must be [C, number of nodes]")
        n, ncomp = pts.shape[0], f.shape[0]
        if out is None:
            out = np.empty((n, ncomp), dtype=np.float64)
        elif out.shape != (n, ncomp) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous f64[N, C] array")
        enc = np.empty((n, 8), dtype=np.int64) if want_operator else None
        w = np.empty((n, 8), dtype=np.float64) if want_operator else None
        nf = self._call("mm_interpolate_hex8_host", nod.ctypes.data, nod.shape[0], conn.ctypes.data, conn.shape[0],
                        pts.ctypes.data, n, f.ctypes.data, ncomp, nelem_to_search, out.ctypes.data,
                        enc.ctypes.data if want_operator else None, w.ctypes.data if want_operator else None)
        return _with_operator(want_operator, out, enc, w, nf)

    # ---- section 8f-4: device passes of the layer-aware drivers ------------------------------------
    def scatter_elements(self, values, inverse, elem_ids, out):
        """``out[:, elem_ids] = values[inverse].reshape(len(elem_ids), P, C)`` transposed to the element-nodal
        layout (reference interpolator.py:1079-1081): values f64[U, C], inverse int64[len(elem_ids) * P],
        out f64[C, E, P] (updated in place on the device)."""
        v = self.asdevice(values, np.float64)
        inv = self.asdevice(inverse, np.int64)
        ids = self.asdevice(elem_ids, np.int64)
        o = self.asdevice(out, np.float64)
        ncomp, nelem_out, P = o.shape
        if v.shape[1] != ncomp or inv.size != ids.size * P:
            raise ValueError("need values[U, C], inverse[len(elem_ids) * P], out[C, E, P]")
        self._call("mm_scatter_elements", v, v.shape[0], ncomp, inv, ids, ids.size, P, nelem_out, o)
        return o

    def fluid_solid_fix(self, values, previous, solid, vs_index):
        """The fix-up of reference interpolator.py:829-841 on values f64[E, C, P] (in place on the device):
        fluid elements and solid elements with a zero shear velocity get ``previous`` back.  Returns the
        number of solid elements restored."""
        v = self.asdevice(values, np.float64)
        prev = self.asdevice(previous, np.float64)
        sol = self.asdevice(np.ascontiguousarray(solid, dtype=np.uint8), np.uint8)
        nelem, ncomp, P = v.shape
        if prev.shape != v.shape or sol.size != nelem:
            raise ValueError("need values[E, C, P], previous[E, C, P], solid[E]")
        return int(self._call("mm_fluid_solid_fix", v, prev, sol, nelem, ncomp, P, int(vs_index)))

    # ---- Earth meshes onto their 1-D sphere (reference interpolator.py:1085-1144) ------------------------------
    def _points3(self, points):
        pts = self.asdevice(points, np.float64)
        if len(pts.shape) < 2 or pts.shape[-1] != 3:
            raise ValueError("points must be [..., 3] (3-D meshes only)")
        return pts, pts.size // 3

    def first_occurrence(self, connectivity, nnodes):
        """``np.unique(connectivity, return_index=True)[1]`` as the node layout of ``map_to_sphere`` reads it:
        int64[nnodes] with the smallest flat index of every node.  Raises ``ValueError`` when a node is not
        referenced (the reference would fail there with an index error) or an entry lies outside [0, nnodes)."""
        conn = self.asdevice(connectivity, np.int64)
        first = self.empty((int(nnodes),), np.int64)
        unreferenced = self._call_args("mm_first_occurrence", conn, conn.size, int(nnodes), first)
        if unreferenced:
            raise ValueError(f"{unreferenced} nodes are not referenced by the connectivity: z_node_1D has no value "
                             "for them")
        return first

    def _radius_index(self, npoints, rad, connectivity, first):
        """(rad DeviceArray, first DeviceArray or None) for ``npoints`` points."""
        r = self.asdevice(rad, np.float64)
        if connectivity is None and first is None:
            if r.size != npoints:
                raise ValueError("element-nodal layout: rad (z_node_1D) needs one value per point")
            return r, None
        if first is None:
            conn = self.asdevice(connectivity, np.int64)
            if conn.size != r.size:
                raise ValueError("node layout: z_node_1D must be element-nodal, the shape of the connectivity")
            first = self.first_occurrence(conn, npoints)
        else:
            first = self.asdevice(first, np.int64)
            if first.size != npoints:
                raise ValueError("first must hold one index per point")
        return r, first

    def map_to_sphere(self, points, rad, connectivity=None, out=None, r_ref=6371000.0, first=None):
        """Every point rescaled radially onto the radius of its 1-D model, ``((p * r_ref) * rad) / |p|``
        (reference interpolator.py:1125-1144); points at the centre are left alone.

        Element-nodal layout: ``points`` f64[E, P, 3] (or [N, 3]) and ``rad`` (z_node_1D) f64[E, P] (or [N]).
        Node layout: ``points`` f64[N, 3], ``rad`` f64[E, P] element-nodal and ``connectivity`` int64[E, P]: node
        n takes the value of its first occurrence in the flattened connectivity (or pass ``first``, what
        :meth:`first_occurrence` returned).  ``out``: None -> a new device array; ``out`` may be ``points``
        itself for the in-place map (a DeviceArray, a device tensor, or a NumPy array, which then receives the
        result).  Returns the mapped points (``out`` when given)."""
        pts, n = self._points3(points)
        r, first = self._radius_index(n, rad, connectivity, first)
        host_out = out if isinstance(out, np.ndarray) else None
        if host_out is not None:
            if host_out.shape != pts.shape or host_out.dtype != np.float64 or not host_out.flags.c_contiguous:
                raise ValueError("out must be a C-contiguous f64 array of the shape of points")
            out = pts if host_out is points else None
        out = self._out(out, pts.shape, "out must have the shape of points", size_only=True)
        self._call("mm_map_to_sphere", pts, n, r, r.size, first, float(r_ref), out)
        if host_out is not None:      # a NumPy ``out`` (``points`` itself for the in-place map) receives the result
            self._call("mm_copy_d2h", host_out.ctypes.data, out, host_out.nbytes)
            return host_out
        return out

    def sphere_ratio(self, points, rad, connectivity=None, r_ref=6371000.0, first=None):
        """``(|p| / r_ref) / rad`` per point (reference interpolator.py:1093-1097), the radial stretch of an
        elliptic mesh over its sphere; layouts as :meth:`map_to_sphere`.  Returns f64 of the points' leading shape."""
        pts, n = self._points3(points)
        r, first = self._radius_index(n, rad, connectivity, first)
        out = self.empty(pts.shape[:-1], np.float64)
        self._call("mm_sphere_ratio", pts, n, r, r.size, first, float(r_ref), out)
        return out

    def scale_points(self, points, factor, out=None):
        """``factor[i] * p_i`` (reference interpolator.py:1121); ``out`` may be ``points`` (in place)."""
        pts, n = self._points3(points)
        f = self.asdevice(factor, np.float64)
        if f.size != n:
            raise ValueError("factor needs one value per point")
        out = self._out(out, pts.shape, "out must have the shape of points", size_only=True)
        self._call("mm_scale_points", pts, n, f, out)
        return out

    # ---- A11 ----------------------------------------------------------------------------
    def unique_points(self, points, unique_out=None, inverse_out=None, ordered=True):
        """``np.unique(points, axis=0, return_inverse=True)`` (reference utils.py:484-488) on the
        device: (unique f64[U, dim] in lexicographic order, inverse int64[N]).  ``unique_out`` f64[N, dim] /
        ``inverse_out`` int64[N]: caller-owned device buffers to write into (no allocation in the call).
        ``ordered=False``: the unique rows in the order of their first occurrence instead (a hash table, 2-3x
        faster) -- enough wherever the rows are only interpolated and scattered back through the inverse."""
        pts = self.asdevice(points, np.float64)
        n, dim = pts.shape
        uniq = self.empty((max(n, 1), dim), np.float64) if unique_out is None else self.asdevice(unique_out, np.float64)
        inv = self.empty((max(n, 1),), np.int64) if inverse_out is None else self.asdevice(inverse_out, np.int64)
        if uniq.size < n * dim or inv.size < n:
            raise ValueError("unique_out / inverse_out too small: need [N, dim] and [N]")
        nu = self._call("mm_unique_points" if ordered else "mm_unique_points_any_order", pts, n, dim, uniq, inv,
                        what="mm_unique_points")      # (a failure of either has always been reported under this name)
        return uniq.rows(0, int(nu)), inv.rows(0, n)

    def close(self):
        if self.handle:
            self.lib.mm_context_destroy(self.handle)
        self.handle = None


_default = {}


def default_context(device=0):
    """Process-wide context per device (created on first use; raises without a GPU)."""
    if device not in _default:
        _default[device] = Context(device)
    return _default[device]


__all__ = ["Context", "DeviceArray", "Diffusion", "KnnIndex", "Source", "TransposedOperator", "default_context",
           "MultiMeshHipError"]
