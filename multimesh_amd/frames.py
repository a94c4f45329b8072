"""Frames: meshes, points and vector fields rotated on the GPU, models imported in a rotated frame, and vector fields
expressed in the local up/north/east basis of every node (include/multimesh_frames.h: ``mm_rotate_points``,
``mm_rotate_vectors``, ``mm_local_components``; the header holds the statement, operation by operation, which the device
reproduces bit for bit).  Imported explicitly (``from multimesh_amd import frames``).

Every model tool of the package reads a model in the mesh's own geographic frame: ``z`` is the pole, latitude is
geocentric, longitude runs from ``x`` towards ``y``.  Two things break that: meshes built with the source under the north
pole and then rotated to the event (the reference's ``multi_mesh/utils.py``: ``get_rot_matrix``, ``rotate``,
``rotate_mesh``), and regional models that ship on a lat/lon/depth grid in a rotated frame.  :class:`Rotation` and
:func:`rotate_mesh` serve the first, :func:`in_frame` the second; :func:`local_components` and
:meth:`Rotation.apply_to_vectors` let vector fields (``gll_gradient``'s planes, displacement snapshots) follow.

There is NO file driver for Exodus meshes here: :class:`multimesh_amd.io.Exodus` has no coordinate writer, and adding one
is a separate change.  Read the coordinates, rotate them (:meth:`Rotation.apply`) and write them with the tool that owns
the file.

The symbols are an extension of the library's C ABI with a header of their own: this module keeps their signature table
and applies it to the handle of :func:`multimesh_amd.helpers.load_lib` on first use; the calls themselves go through
:func:`multimesh_amd.device._call` and the :class:`Context` checks like every other call of the package."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np

from . import device as _device
from .api._common import GllMesh, _mesh_points, is_mesh, named_fields
from .api.earth import _set_points
from .device import default_context
from .helpers import i32, i64, load_lib, vp
from .mesh import HexMesh

__all__ = ["Rotation", "rotate_mesh", "in_frame", "local_components", "rotate_points", "rotate_vectors_on_device",
           "local_components_on_device", "BASIS", "ORTHOGONALITY_TOL"]

MAX_P = 4096   # MM_PARAM_MAX_P: the nodes of one group of the field addressing
#: names -> their numbers in the C ABI (MM_FRAMES_BASIS_*): (radial, south, east) and (up, north, east)
BASIS = {"rtp": 0, "zne": 1}
#: what :class:`Rotation` allows of ``|R^T R - I|``, elementwise
ORTHOGONALITY_TOL = 1e-12

#: name -> (restype, argtypes) of the functions include/multimesh_frames.h declares (tests/test_frames.py compares it with
#: the header); they are not part of helpers.SIGNATURES, the table of include/multimesh_hip.h
SIGNATURES = {
    "mm_rotate_points": (i32, (vp, i64, vp, vp, vp, i32)),
    "mm_rotate_vectors": (i32, (vp, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, vp, i32)),
    "mm_local_components": (i32, (vp, i64, i64, vp, vp, i64, i64, vp, vp, i64, i64, vp, i32, i32)),
}


def bind(lib=None):
    """The library handle with :data:`SIGNATURES` applied (once)."""
    lib = lib or load_lib()
    if getattr(lib, "_frames_bound", False) is not True:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        lib._frames_bound = True
    return lib


# ------------------------------------------------------------------------------------------------------------ the calls
def _matrix9(matrix):
    m = np.ascontiguousarray(matrix, dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError(f"a rotation matrix is [3, 3], got {m.shape}")
    return (C.c_double * 9)(*m.ravel())


def _cols3(cols):
    cols = [int(c) for c in cols]
    if len(cols) != 3:
        raise ValueError(f"a vector has 3 components, got {len(cols)} columns")
    return (C.c_int * 3)(*cols)


def _is_device(ctx, x):
    return isinstance(x, _device.DeviceArray) or (hasattr(x, "data_ptr") and hasattr(x, "shape") and not ctx._on_host(x))


def rotate_points(ctx, points, matrix, transpose=False, out=None):
    """``mm_rotate_points`` on the context ``ctx``: ``points`` f64[..., 3] (a host array, a :class:`DeviceArray` or a
    torch-like tensor on the GPU) multiplied by ``matrix`` f64[3, 3] (``transpose``: by its transpose) into ``out`` -- a
    device array of as many values, which may be ``points`` itself, or None: a new one.  Returns the device array.  Runs
    on the context's stream and does not synchronise; ``ValueError`` with the library's message for what it refuses."""
    lib = bind(ctx.lib)
    pts, n = ctx._points3(points)
    out = ctx._out(out, pts.shape, "out must hold as many values as points", size_only=True)
    _device._call(lib, "mm_rotate_points", ctx.handle, n, pts, out, _matrix9(matrix), int(bool(transpose)), arg_error=True)
    return out


def _check_layouts(ngroups, P, **layouts):
    for what, layout in layouts.items():
        if ngroups > 0 and min(layout[3]) >= 0 and min(layout[1:3]) >= 0:     # (negative values are the library's to refuse)
            extent = (int(ngroups) - 1) * int(layout[1]) + max(layout[3]) * int(layout[2]) + int(P)
            if extent > layout[0].size:
                raise ValueError(f"{what}: the layout reaches element {extent - 1} of an array of {layout[0].size}")


def _layout_args(layout):
    return [layout[0], int(layout[1]), int(layout[2]), _cols3(layout[3])]


def rotate_vectors_on_device(ctx, matrix, ngroups, P, src, dst, transpose=False):
    """``mm_rotate_vectors`` for arrays that are on the device already, in any layout the addressing of
    include/multimesh_params.h reaches.  ``src`` and ``dst`` are ``(DeviceArray, group_stride, comp_stride, cols)``:
    component c of node p of group e is element ``e * group_stride + cols[c] * comp_stride + p``.  ``dst`` may be ``src``
    with the same strides (its columns may be permuted).  Does not synchronise; ``ValueError`` for what is refused."""
    lib = bind(ctx.lib)
    _check_layouts(ngroups, P, src=src, dst=dst)
    _device._call(lib, "mm_rotate_vectors", ctx.handle, int(ngroups), int(P), *_layout_args(src), *_layout_args(dst),
                  _matrix9(matrix), int(bool(transpose)), arg_error=True)


def local_components_on_device(ctx, points, ngroups, P, src, dst, inverse=False, basis="rtp"):
    """``mm_local_components`` for arrays that are on the device already: ``points`` f64[ngroups * P, 3] (any shape of that
    size), ``src`` and ``dst`` as :func:`rotate_vectors_on_device`.  ``inverse``: local -> Cartesian."""
    if basis not in BASIS:
        raise ValueError(f"basis must be one of {list(BASIS)}, got {basis!r}")
    lib = bind(ctx.lib)
    if points.size != 3 * int(ngroups) * int(P):
        raise ValueError(f"points must hold {int(ngroups) * int(P)} positions, got {points.shape}")
    _check_layouts(ngroups, P, src=src, dst=dst)
    _device._call(lib, "mm_local_components", ctx.handle, int(ngroups), int(P), points, *_layout_args(src), *_layout_args(dst),
                  int(bool(inverse)), BASIS[basis], arg_error=True)


def _planes(ctx, values, what):
    """(values f64[3, ...] on the device, ngroups, P, whether it was on the device) of three field planes: [3, E, P] with
    P within the addressing's limit keeps its groups, any other shape is one node per group."""
    on_device = _is_device(ctx, values)
    v = ctx.asdevice(values, np.float64)
    if len(v.shape) < 2 or v.shape[0] != 3:
        raise ValueError(f"{what} must be [3, ...]: the three components of a vector field, got {v.shape}")
    if len(v.shape) == 3 and 1 <= v.shape[2] <= MAX_P:
        return v, v.shape[1], v.shape[2], on_device
    return v, v.size // 3, 1, on_device


def _plane_layout(array, ngroups, P):
    return (array, P, ngroups * P, (0, 1, 2))


def _plane_out(ctx, out, v, on_device):
    """The device output of a call on planes ``v``: the caller's device ``out``, or a new array."""
    if out is not None and not on_device:
        raise ValueError("out goes with device arrays: host arrays give a new host array")
    return ctx._out(out, v.shape, "out must hold as many values as the fields", size_only=True)


# ----------------------------------------------------------------------------------------------------------- rotations
def _rodrigues(x, y, z, c, s):
    """Rodrigues' formula for the unit axis (x, y, z) and the cosine ``c`` and sine ``s`` of the angle (right-hand rule),
    with the operands in the order of the reference's ``get_rot_matrix``: NumPy scalars give its entries bit for bit."""
    m = np.empty((3, 3))
    m[0, 0] = c + (x**2) * (1 - c)
    m[1, 0] = z * s + x * y * (1 - c)
    m[2, 0] = (-1) * y * s + x * z * (1 - c)
    m[0, 1] = x * y * (1 - c) - z * s
    m[1, 1] = c + (y**2) * (1 - c)
    m[2, 1] = x * s + y * z * (1 - c)
    m[0, 2] = y * s + x * z * (1 - c)
    m[1, 2] = (-1) * x * s + y * z * (1 - c)
    m[2, 2] = c + (z * z) * (1 - c)
    return m


def _unit(axis):
    x, y, z = (np.float64(a) for a in np.asarray(axis, dtype=np.float64).reshape(3))
    norm = np.sqrt(x**2 + y**2 + z**2)
    if not (np.isfinite(norm) and norm > 0):
        raise ValueError(f"a rotation axis must be finite and not zero, got {axis}")
    return x / norm, y / norm, z / norm


class Rotation:
    """A rotation of 3-D space: ``matrix`` f64[3, 3], applied as ``p' = matrix @ p``.

    With ``check`` (default) ``ValueError`` unless ``|matrix^T matrix - I| <= 1e-12`` elementwise and ``det > 0``: a scaled
    matrix and a reflection are refused.  ``check=False`` takes any nine finite numbers -- the device applies what it is
    given.  ``.inverse()`` is the transpose, ``a @ b`` the rotation that applies ``b`` first (NumPy's matrix product, on
    the host)."""

    def __init__(self, matrix, check=True):
        m = np.array(matrix, dtype=np.float64)
        if m.shape != (3, 3):
            raise ValueError(f"a rotation matrix is [3, 3], got {m.shape}")
        if not np.isfinite(m).all():
            raise ValueError("a rotation matrix must be finite")
        if check:
            off = np.abs(m.T @ m - np.eye(3)).max()
            if not off <= ORTHOGONALITY_TOL:
                raise ValueError(f"not a rotation: |R^T R - I| reaches {off:.3g} (allowed: {ORTHOGONALITY_TOL:g})")
            if not np.linalg.det(m) > 0:
                raise ValueError("not a rotation: the determinant is negative (a reflection)")
        self.matrix = m

    @classmethod
    def identity(cls):
        return cls(np.eye(3), check=False)

    @classmethod
    def from_axis_angle(cls, axis, angle_deg):
        """The right-hand rotation about ``axis`` (three numbers, normalised here) by ``angle_deg`` degrees: Rodrigues'
        formula -- the axis normalised first, then the nine entries from ``cos``, ``sin`` and ``1 - cos`` -- in the operand
        order of the reference's ``get_rot_matrix``, whose matrix for ``np.deg2rad(angle_deg)`` this is bit for bit
        (tests/golden/rotation.npz)."""
        return cls.from_axis_angle_rad(axis, np.deg2rad(np.float64(angle_deg)))

    @classmethod
    def from_axis_angle_rad(cls, axis, angle):
        """:meth:`from_axis_angle` with the angle in radians."""
        angle = np.float64(angle)
        if not np.isfinite(angle):
            raise ValueError("the angle must be finite")
        return cls(_rodrigues(*_unit(axis), np.cos(angle), np.sin(angle)))

    @classmethod
    def to_north_pole(cls, lat_deg, lon_deg):
        """The rotation that takes the geocentric direction ``e`` of (``lat_deg``, ``lon_deg``) to the north pole
        ``n = (0, 0, 1)``: about ``e x n`` by ``arccos(e . n)``, the shortest way.  A mesh built with its source under the
        north pole is moved to an event at (lat, lon) by the INVERSE (``rotate_mesh(mesh, R, backwards=True)``); a model
        given around (lat, lon) is brought to the pole by the rotation itself.

        This is what the reference's ``rotate_mesh`` intends; that function takes the cosines of its location without a
        conversion from degrees and notes itself that its direction is unsettled, so the definition here is this
        package's own.  The axis is ``(sin lon, -cos lon, 0)`` and the cosine and sine of the angle are ``sin lat`` and
        ``cos lat``, used as they are (an ``arccos`` of ``e . n`` would lose half the digits near the poles).  ``e == n``
        (lat 90) gives the identity, ``e == -n`` (lat -90), where the axis is undefined, a half turn about ``y``."""
        lat, lon = np.float64(lat_deg), np.float64(lon_deg)
        if not (np.isfinite(lon) and -90.0 <= lat <= 90.0):
            raise ValueError(f"need -90 <= lat <= 90 and a finite lon, got ({lat_deg}, {lon_deg})")
        if lat == 90.0:
            return cls.identity()
        if lat == -90.0:
            return cls(np.diag([-1.0, 1.0, -1.0]))
        phi, lam = np.deg2rad(lat), np.deg2rad(lon)
        return cls(_rodrigues(*_unit((np.sin(lam), -np.cos(lam), 0.0)), np.sin(phi), np.cos(phi)))

    def inverse(self):
        return Rotation(self.matrix.T, check=False)

    def __matmul__(self, other):
        if not isinstance(other, Rotation):
            raise TypeError("a Rotation composes with a Rotation: wrap the matrix")
        return Rotation(self.matrix @ other.matrix, check=False)

    def __repr__(self):
        return f"Rotation({self.matrix.tolist()})"

    # ---- on the device
    def apply(self, points, out=None, backwards=False, context=None):
        """``matrix @ p`` (``backwards``: ``matrix^T @ p``) for every point of ``points`` f64[..., 3], on the GPU
        (``mm_rotate_points``: ``x' = (R00*x + R01*y) + R02*z`` ..., every operation rounded on its own).

        A NumPy array gives a new NumPy array, or fills ``out`` -- a C-contiguous f64 array of the same shape, which may
        be ``points`` itself.  A :class:`DeviceArray` or a device tensor gives a device array: a new one, or ``out``, which
        may be ``points`` itself (in place); the call runs on the context's stream and does not synchronise."""
        ctx = context or default_context()
        if _is_device(ctx, points):
            return rotate_points(ctx, points, self.matrix, transpose=backwards, out=out)
        host = np.ascontiguousarray(points, dtype=np.float64)
        if host.ndim < 1 or host.shape[-1] != 3:
            raise ValueError(f"points must be [..., 3] (3-D only), got {host.shape}")
        if out is not None and not (isinstance(out, np.ndarray) and out.shape == host.shape and out.dtype == np.float64
                                    and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("out must be a writable C-contiguous f64 array of the shape of points")
        pts = ctx.to_device(host.reshape(-1, 3))
        res = rotate_points(ctx, pts, self.matrix, transpose=backwards, out=pts).numpy().reshape(host.shape)
        if out is None:
            return res
        out[...] = res
        return out

    def apply_to_vectors(self, fields, columns=None, out=None, backwards=False, context=None):
        """``v' = matrix @ v`` (``backwards``: the transpose) for the vector at every node (``mm_rotate_vectors``).

        Without ``columns``, ``fields`` holds field planes f64[3, ...] (``gll_gradient``'s ``[dim, E, P]`` of one
        component, three stacked fields of a mesh): the result has the same shape.  With ``columns`` -- three column
        indices --, ``fields`` is f64[E, C_total, P], the layout of ``MODEL/data``: those three columns are rotated,
        every other column is carried over.  Host arrays give a new host array; device arrays give a device array,
        ``out`` when given (it may be ``fields`` itself), else a new one for planes and ``fields`` itself, in place, for
        columns."""
        ctx = context or default_context()
        if columns is None:
            v, ngroups, P, on_device = _planes(ctx, fields, "fields")
            dst = _plane_out(ctx, out, v, on_device)
            rotate_vectors_on_device(ctx, self.matrix, ngroups, P, _plane_layout(v, ngroups, P), _plane_layout(dst, ngroups, P),
                                     transpose=backwards)
            return dst if on_device else dst.numpy()
        on_device = _is_device(ctx, fields)
        rows = ctx.asdevice(fields, np.float64)            # (a host array: a copy, which carries the other columns)
        if len(rows.shape) != 3 or not 1 <= rows.shape[2] <= MAX_P:
            raise ValueError(f"with columns, fields must be [E, C_total, P] with P <= {MAX_P}, got {rows.shape}")
        nelem, ncol, P = rows.shape
        if len(list(columns)) != 3 or not all(0 <= int(c) < ncol for c in columns):
            raise ValueError(f"columns must be three indices into the {ncol} columns, got {list(columns)}")
        dst = rows if out is None else _plane_out(ctx, out, rows, on_device)
        layout = lambda a: (a, ncol * P, P, tuple(columns))
        rotate_vectors_on_device(ctx, self.matrix, nelem, P, layout(rows), layout(dst), transpose=backwards)
        return dst if on_device else dst.numpy()


# ------------------------------------------------------------------------------------------------------------- meshes
def _points3d(mesh, who):
    pts = np.asarray(_mesh_points(mesh))
    if pts.ndim not in (2, 3) or pts.shape[-1] != 3:
        raise ValueError(f"{who} rotates 3-D meshes only (points of shape {pts.shape})")
    return np.ascontiguousarray(pts, dtype=np.float64)


def rotate_mesh(mesh, rotation, backwards=False, context=None):
    """Rotates the points of ``mesh`` IN PLACE on the GPU: every point becomes ``rotation.matrix @ p`` (``backwards``: the
    transpose, as the reference's ``rotate_mesh``).  ``mesh``: a :class:`GllMesh`, a :class:`HexMesh` or a Salvus mesh
    object (``points``); its fields are untouched -- vector fields follow through :meth:`Rotation.apply_to_vectors`.
    ``ValueError`` for a 2-D mesh.  Returns the mesh."""
    pts = _points3d(mesh, "rotate_mesh")
    _set_points(mesh, rotation.apply(pts, backwards=backwards, context=context))
    return mesh


def in_frame(mesh, rotation, context=None):
    """``mesh`` seen from the frame ``rotation`` leads to: a mesh of the same class (:class:`GllMesh` or :class:`HexMesh`)
    whose points are ``rotation.matrix @ p``, computed on the device into a NEW array, and whose field store IS the
    original's.  The caller's coordinates never change.

    This is how a model given in a rotated frame is imported: with ``R`` the rotation that takes the mesh's geographic
    frame to the model's, ``api.import_regular_grid(grid, frames.in_frame(mesh, R), ...)`` samples the model at the rotated
    positions and binds the fields to ``mesh``; :func:`multimesh_amd.harmonics.import_harmonic_model` and
    :func:`multimesh_amd.layered.import_layered_model` likewise.

    Preferred to rotating the mesh there and back: ``R^T (R p)`` is not ``p`` bit for bit -- each product and sum rounds,
    so a mesh that made the round trip no longer shares its points with the meshes it was built beside, and exact
    coincidences (shared faces, points on interfaces) are lost.

    The view composes with :func:`multimesh_amd.geodesy.as_geographic`, the view of a mesh in geographic (geodetic)
    coordinates: ``in_frame(as_geographic(mesh, ellipsoid), R)`` is the geographic view seen from the rotated frame."""
    if not isinstance(mesh, (GllMesh, HexMesh)):
        raise ValueError("in_frame takes a GllMesh or a HexMesh")
    pts = _points3d(mesh, "in_frame")
    view = copy.copy(mesh)              # (shallow: the same field store, the same connectivity)
    rotated = rotation.apply(pts, context=context)
    if isinstance(mesh, GllMesh):
        view.gll_points = rotated
    else:
        view.points = rotated
    return view


def local_components(mesh_or_points, vectors, basis="rtp", inverse=False, out=None, context=None):
    """The components of a vector field in the local basis at every node (``mm_local_components``), or back.

    ``mesh_or_points``: a mesh, or the positions f64[..., 3] of the nodes (host or device).  ``vectors``: f64[3, ...] over
    the leading shape of the positions -- Cartesian ``(vx, vy, vz)`` --, or three names of fields of the mesh.  ``basis``:
    "rtp" gives (radial, south, east), "zne" (up, north, east): the second component negated, exactly.  A node on the
    polar axis takes longitude 0; a node at the centre gives NaN.  ``inverse``: ``vectors`` holds the local components and
    the result is Cartesian.  Host arrays (and names) give a new host array f64[3, ...]; device arrays a device array,
    ``out`` when given (it may be ``vectors`` itself)."""
    if basis not in BASIS:
        raise ValueError(f"basis must be one of {list(BASIS)}, got {basis!r}")
    ctx = context or default_context()
    mesh = mesh_or_points if is_mesh(mesh_or_points) else None
    if isinstance(vectors, (list, tuple)) and all(isinstance(p, str) for p in vectors):
        if mesh is None or len(vectors) != 3:
            raise ValueError("named vectors are three fields of a mesh")
        vectors = named_fields(mesh, list(vectors))[1]
    pts = ctx.asdevice(_mesh_points(mesh) if mesh is not None else mesh_or_points, np.float64)
    if len(pts.shape) < 1 or pts.shape[-1] != 3:
        raise ValueError(f"positions must be [..., 3] (3-D only), got {pts.shape}")
    v, ngroups, P, on_device = _planes(ctx, vectors, "vectors")
    if v.shape[1:] != pts.shape[:-1]:
        raise ValueError(f"vectors {v.shape} must be [3, ...] over the positions {pts.shape}")
    dst = _plane_out(ctx, out, v, on_device)
    local_components_on_device(ctx, pts, ngroups, P, _plane_layout(v, ngroups, P), _plane_layout(dst, ngroups, P),
                               inverse=inverse, basis=basis)
    return dst if on_device else dst.numpy()
