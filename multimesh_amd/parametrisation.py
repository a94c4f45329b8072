"""Parametrisations: models and sensitivity kernels converted between ``iso_velocity``, ``iso_lame``, ``iso_bulk``,
``vti_velocity`` and ``vti_love`` on the GPU, node by node, on arrays that need not leave HBM (include/multimesh_params.h:
``mm_convert_parameters``, ``mm_convert_kernels``; the header holds the statement, formula by formula, which the device
reproduces bit for bit).  Imported explicitly (``from multimesh_amd import parametrisation``); the reference has no
counterpart.

The two symbols are an extension of the library's C ABI with a header of their own: this module keeps their signature
table and applies it to the handle of :func:`multimesh_amd.helpers.load_lib` on first use; the calls themselves go through
:func:`multimesh_amd.device._call` like every other call of the package."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import device as _device
from . import io as mio
from .api._common import field_store, named_fields, require_fields
from .device import default_context
from .helpers import i32, i64, load_lib, vp
from .mesh import HexMesh

__all__ = ["PARAMETRISATIONS", "STEPS", "route", "detect", "convert_values", "convert_kernels", "convert_on_device",
           "convert_model", "convert_model_file"]

#: name -> components, in the order of the arrays; the position of a name is its number in the C ABI
PARAMETRISATIONS = {
    "iso_velocity": ("VP", "VS", "RHO"),
    "iso_lame": ("LAMBDA", "MU", "RHO"),
    "iso_bulk": ("KAPPA", "MU", "RHO"),
    "vti_velocity": ("VPV", "VPH", "VSV", "VSH", "ETA", "RHO"),
    "vti_love": ("A", "C", "L", "N", "F", "RHO"),
}

#: the eight directed steps (from, to), numbered from 1 as in the header; the last two go one way only
STEPS = (
    ("iso_velocity", "iso_lame"),
    ("iso_lame", "iso_velocity"),
    ("iso_lame", "iso_bulk"),
    ("iso_bulk", "iso_lame"),
    ("vti_velocity", "vti_love"),
    ("vti_love", "vti_velocity"),
    ("iso_velocity", "vti_velocity"),
    ("vti_love", "iso_bulk"),
)

MAX_P = 4096   # MM_PARAM_MAX_P

#: name -> (restype, argtypes) of the functions include/multimesh_params.h declares (tests/test_parametrisation.py compares
#: it with the header); they are not part of helpers.SIGNATURES, the table of include/multimesh_hip.h
SIGNATURES = {
    "mm_convert_parameters": (i32, (vp, i32, i32, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, vp)),
    "mm_convert_kernels": (i32, (vp, i32, i32, i64, i64, vp, i64, i64, vp, vp, i64, i64, vp, vp, i64, i64, vp, vp)),
}


def bind(lib=None):
    """The library handle with :data:`SIGNATURES` applied (once)."""
    lib = lib or load_lib()
    if getattr(lib, "_parametrisation_bound", False) is not True:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        lib._parametrisation_bound = True
    return lib


def step_name(step):
    return f"{step[0]}->{step[1]}"


def _check_name(name):
    if name not in PARAMETRISATIONS:
        raise ValueError(f"unknown parametrisation {name!r}: one of {list(PARAMETRISATIONS)}")
    return name


def route(frm, to):
    """The steps of the conversion ``frm`` -> ``to`` as a tuple of names ``"a->b"``: the legal route with the fewest
    steps around the ring ``iso_velocity -- iso_lame -- iso_bulk <- vti_love -- vti_velocity <- iso_velocity`` (five edges:
    two routes never tie; at most four steps).  ``frm == to`` is the empty route."""
    _check_name(frm), _check_name(to)
    paths = {frm: ()}
    frontier = [frm]
    while frontier and to not in paths:
        nxt = []
        for a in frontier:
            for s in STEPS:
                if s[0] == a and s[1] not in paths:
                    paths[s[1]] = paths[a] + (step_name(s),)
                    nxt.append(s[1])
        frontier = nxt
    return paths[to]


def detect(names):
    """The one parametrisation whose components are all among ``names`` (``QKAPPA``, ``QMU`` and unknown names are
    ignored); ``ValueError`` naming the candidates when none or several match."""
    names = set(names)
    found = [p for p, comps in PARAMETRISATIONS.items() if set(comps) <= names]
    if len(found) == 1:
        return found[0]
    if not found:
        raise ValueError(f"the names {sorted(names)} hold no complete parametrisation; candidates: "
                         + ", ".join(f"{p} {list(c)}" for p, c in PARAMETRISATIONS.items()))
    raise ValueError(f"the names {sorted(names)} hold several parametrisations, {found}: pass frm")


def _number(name):
    return list(PARAMETRISATIONS).index(_check_name(name))


def _cols(cols, name):
    cols = [int(c) for c in cols]
    if len(cols) != len(PARAMETRISATIONS[name]):
        raise ValueError(f"{name} has {len(PARAMETRISATIONS[name])} components, got {len(cols)} columns")
    return (C.c_int * len(cols))(*cols)


def convert_on_device(ctx, frm, to, ngroups, P, src, dst, kernels=None, nbad=None):
    """The call itself, for arrays that are on the device already, in any layout the header's addressing reaches.  ``src``,
    ``dst`` and ``kernels`` are ``(DeviceArray, group_stride, comp_stride, cols)``: component c of node p of group e is
    element ``e * group_stride + cols[c] * comp_stride + p``.  Without ``kernels``: ``dst`` (in ``to``) = the converted
    ``src`` (in ``frm``).  With ``kernels`` (in ``to``): ``dst`` (in ``frm``) = J^T kernels at the model ``src``.  ``dst``
    may be an input with the same strides.  ``nbad``: int64[1] on the device, to which the number of nodes with a
    non-finite output is added, or None.  Runs on the context's stream and does not synchronise; ``ValueError`` with the
    library's message for what it refuses."""
    lib = bind(ctx.lib)
    f, t = _number(frm), _number(to)
    for what, layout in (("src", src), ("dst", dst), ("kernels", kernels)):
        if layout is not None and ngroups > 0 and min(layout[3]) >= 0 and min(layout[1:3]) >= 0:
            extent = (int(ngroups) - 1) * int(layout[1]) + max(layout[3]) * int(layout[2]) + int(P)
            if extent > layout[0].size:     # (negative values are the library's to refuse)
                raise ValueError(f"{what}: the layout reaches element {extent - 1} of an array of {layout[0].size}")
    args = [ctx.handle, f, t, int(ngroups), int(P), src[0], int(src[1]), int(src[2]), _cols(src[3], frm)]
    if kernels is None:
        symbol = "mm_convert_parameters"
        args += [dst[0], int(dst[1]), int(dst[2]), _cols(dst[3], to)]
    else:
        symbol = "mm_convert_kernels"
        args += [kernels[0], int(kernels[1]), int(kernels[2]), _cols(kernels[3], to),
                 dst[0], int(dst[1]), int(dst[2]), _cols(dst[3], frm)]
    _device._call(lib, symbol, *args, nbad, arg_error=True)


def _planes(ctx, values, name, what):
    """(values f64[C, ...] on the device, ngroups, P, whether it came from the host) of field planes in ``name``."""
    on_device = isinstance(values, _device.DeviceArray) or (hasattr(values, "data_ptr") and not ctx._on_host(values))
    v = ctx.asdevice(values, np.float64)
    ncomp = len(PARAMETRISATIONS[name])
    if len(v.shape) < 2 or v.shape[0] != ncomp:
        raise ValueError(f"{what} must be [{ncomp}, ...]: the components {list(PARAMETRISATIONS[name])} of {name}")
    n = v.size // ncomp
    if len(v.shape) == 3 and 1 <= v.shape[2] <= MAX_P:
        return v, v.shape[1], v.shape[2], on_device
    return v, n, 1, on_device


def _plane_layout(array, ngroups, P):
    return (array, P, ngroups * P, range(array.shape[0]))


def _finish(ctx, out, nbad, on_device):
    count = int(nbad.numpy()[0])   # (the copy waits for the stream)
    return (out if on_device else out.numpy()), count


def convert_values(values, frm, to, context=None):
    """A model ``values`` f64[C_frm, ...] in the parametrisation ``frm`` converted to ``to``: ``(f64[C_to, ...], nbad)``,
    the components in the order of :data:`PARAMETRISATIONS`, ``nbad`` the number of nodes with a component that is not
    finite (a fluid node, ``VS = 0``, is finite in every parametrisation; ``RHO = 0`` is not in the velocities).  ``values``
    may be a host array, a :class:`DeviceArray` or a torch-like tensor on the GPU; a device input gives a device output.
    Bit for bit the composition of the statements of :func:`route`'s steps (include/multimesh_params.h); nothing is
    special-cased."""
    ctx = context or default_context()
    v, ngroups, P, on_device = _planes(ctx, values, frm, "values")
    out = ctx.empty((len(PARAMETRISATIONS[_check_name(to)]),) + v.shape[1:], np.float64)
    nbad = ctx.zeros((1,), np.int64)
    convert_on_device(ctx, frm, to, ngroups, P, _plane_layout(v, ngroups, P), _plane_layout(out, ngroups, P), nbad=nbad)
    return _finish(ctx, out, nbad, on_device)


def convert_kernels(kernels, model, frm, to, context=None):
    """Sensitivity kernels ``kernels`` f64[C_to, ...] with respect to the components of ``to`` turned into kernels with
    respect to those of ``frm`` at the model ``model`` f64[C_frm, ...] (in ``frm``): ``(f64[C_frm, ...], nbad)`` with
    ``K_frm = J^T K_to``, ``J = d to / d frm`` along :func:`route` -- the chain rule, step by step in reverse.  Kernels
    are ABSOLUTE (d misfit / d p); relative kernels (``p * d misfit / d p``) are out of scope: divide by the parameter
    before and multiply after.  Arrays and ``nbad`` as :func:`convert_values`."""
    ctx = context or default_context()
    m, ngroups, P, on_device = _planes(ctx, model, frm, "model")
    k, kgroups, kP, k_on_device = _planes(ctx, kernels, _check_name(to), "kernels")
    if k.shape[1:] != m.shape[1:]:
        raise ValueError(f"kernels {k.shape} and model {m.shape} must cover the same nodes")
    out = ctx.empty(m.shape, np.float64)
    nbad = ctx.zeros((1,), np.int64)
    convert_on_device(ctx, frm, to, ngroups, P, _plane_layout(m, ngroups, P), _plane_layout(out, ngroups, P),
                      kernels=_plane_layout(k, ngroups, P), nbad=nbad)
    return _finish(ctx, out, nbad, on_device or k_on_device)


def convert_model(mesh, to, frm=None, context=None):
    """The model on ``mesh`` -- a :class:`GllMesh`, a :class:`HexMesh` or a Salvus mesh with its fields in memory --
    converted to ``to`` in the mesh's field store: the components of ``frm`` (detected from the field names when None,
    :func:`detect`) are replaced by those of ``to``; every other field (``QKAPPA``, ``QMU``, ...) is left alone.  Returns
    ``nbad`` as :func:`convert_values`."""
    store = field_store(mesh)
    frm = detect(store) if frm is None else _check_name(frm)
    require_fields(mesh, PARAMETRISATIONS[frm])
    names, fields = named_fields(mesh, list(PARAMETRISATIONS[frm]))
    out, nbad = convert_values(fields, frm, to, context=context)
    for name in names:
        del store[name]
    for name, v in zip(PARAMETRISATIONS[to], out):
        if isinstance(mesh, HexMesh):
            mesh.attach_field(name, v)
        else:
            store[name] = np.ascontiguousarray(v)
    return nbad


def convert_model_file(gll_model, to, frm=None, model_path="MODEL/data", context=None):
    """``MODEL/data`` of a Salvus model -- a path, or an open writable h5py-like object -- converted to ``to``.  The
    dataset f64[E, C, P] is uploaded as it is and converted through the column addressing (no transpose); it is rewritten
    (:func:`multimesh_amd.io.remove_and_create_empty_dataset`, so ``DIMENSION_LABELS`` follows) with the components of
    ``to`` first, in their order, and then the columns outside ``frm`` in their old order, carried over bit for bit.
    ``frm`` is detected from the labels when None.  Returns ``nbad``."""
    ctx = context or default_context()
    with mio.open_h5(gll_model, "r+") as f:
        labels = mio.dimension_labels(f[model_path], 1)
        frm = detect(labels) if frm is None else _check_name(frm)
        comps, new = PARAMETRISATIONS[frm], PARAMETRISATIONS[_check_name(to)]
        if missing := [p for p in comps if p not in labels]:
            raise ValueError(f"parameters {missing} are not in {model_path} (it holds {labels})")
        data = np.ascontiguousarray(f[model_path][()], dtype=np.float64)
        if data.ndim != 3:
            raise ValueError(f"{model_path} must be [nelem, nparam, P], got {data.shape}")
        carried = [p for p in labels if p not in comps]
        nelem, ncol, P = data.shape
        width = len(new) + len(carried)
        src = ctx.to_device(data)
        dst = ctx.empty((nelem, width, P), np.float64)
        nbad = ctx.zeros((1,), np.int64)
        convert_on_device(ctx, frm, to, nelem, P, (src, ncol * P, P, [labels.index(p) for p in comps]),
                          (dst, width * P, P, range(len(new))), nbad=nbad)
        out, count = _finish(ctx, dst, nbad, False)
        for j, p in enumerate(carried):
            out[:, len(new) + j, :] = data[:, labels.index(p), :]
        ds = mio.remove_and_create_empty_dataset(f, list(new) + carried, model=model_path)
        ds[:, :, :] = out
    return count
