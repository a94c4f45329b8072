"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/multimesh_hip.h declares, and fails loudly (no CPU fallback) when there is no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from multimesh_amd import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multimesh_hip.h")


def _header_code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))


def _declared_functions():
    names = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", _header_code())
    return sorted(set(n for n in names if n not in ("defined",)))


_SCALARS = {"int": "int", "int64_t": "int64", "long long": "int64", "size_t": "size_t", "double": "double", "void": "void"}


def _c_class(decl, is_return=False):
    """The class of one C parameter (with its name) or return type: "pointer", "char*" or a scalar of _SCALARS."""
    decl = " ".join(decl.replace("*", " * ").split())
    if "*" in decl:
        return "char*" if is_return and decl == "const char *" else "pointer"
    words = [w for w in decl.split() if w != "const"]
    if not is_return and " ".join(words) not in _SCALARS:
        words = words[:-1]                                   # the parameter's name
    return _SCALARS[" ".join(words)]


def _declared_prototypes():
    """name -> (class of the return type, [class of every parameter]) from the text of the header."""
    protos = {}
    for statement in _header_code().split(";"):
        m = re.fullmatch(r"\s*([^()]*?)\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^()]*)\)\s*", re.split(r"[{}]", statement)[-1])
        if not m:
            continue                                         # a typedef, a struct, a linkage brace
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        protos[name] = (_c_class(ret, is_return=True), [_c_class(p) for p in params])
    return protos


def _ctypes_class(t):
    if t is None:
        return "void"
    if t is C.c_char_p:
        return "char*"
    if t is C.c_void_p or issubclass(t, C._Pointer) or hasattr(t, "_dtype_"):   # (_dtype_: an ndpointer class)
        return "pointer"
    if t in (C.c_int64, C.c_longlong):
        return "int64"
    return {C.c_int: "int", C.c_size_t: "size_t", C.c_double: "double"}[t]


def test_header_and_loader_agree():
    declared = _declared_functions()
    assert sorted(helpers.EXPORTED_SYMBOLS) == declared


def test_declared_signatures_match_the_header():
    """Every prototype of the header against what load_lib declares, argument by argument: the count and the class of
    each argument and of the return value (a c_int where the header says int64_t only works by accident of the calling
    convention).  The expectation comes from the header's text alone."""
    protos = _declared_prototypes()
    assert sorted(protos) == _declared_functions() and len(protos) == len(helpers.EXPORTED_SYMBOLS)
    assert list(helpers.EXPORTED_SYMBOLS) == list(protos)           # the table keeps the header's order
    lib = helpers.load_lib()
    wrong = []
    for name, (ret, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None, f"helpers.load_lib does not declare {name}"
        got = (_ctypes_class(fn.restype), [_ctypes_class(t) for t in fn.argtypes])
        if got != (ret, params):
            wrong.append((name, got, (ret, params)))
    assert not wrong, wrong
    # the two legacy symbols take NumPy arrays directly
    assert all(hasattr(t, "_dtype_") for t in lib.centroid.argtypes[3:] + lib.triLinearInterpolator.argtypes[2:])


def test_device_array_reshape_is_a_checked_view():
    import gc
    import types
    import weakref

    from multimesh_amd.device import DeviceArray

    ctx = types.SimpleNamespace(handle=None, lib=None)              # a view needs no GPU and no library call
    parent = DeviceArray(ctx, 4096, (2, 3, 4), np.float64, owner=False)
    for shape in ((5,), (2, 3, 5), (1, 23), ()):
        with pytest.raises(ValueError):
            parent.reshape(*shape)
    view = parent.reshape(1, 2, 12)
    assert (view.ptr, view.shape, view.dtype, view.size) == (4096, (1, 2, 12), np.dtype(np.float64), 24)
    assert view._owner is False and view._keepalive is parent
    assert parent.reshape(24).shape == (24,) and parent.reshape(6, 4).reshape(2, 3, 4).shape == parent.shape
    alive = weakref.ref(parent)
    del parent
    gc.collect()
    assert alive() is not None and alive().ptr == 4096               # the view holds its parent ...
    view.free()
    assert view.ptr == 0 and alive().ptr == 4096                    # ... and does not own its bytes
    del view
    gc.collect()
    assert alive() is None
    empty = DeviceArray(ctx, 0, (0, 3), np.int64, owner=False)
    assert empty.reshape(3, 0).shape == (3, 0) and empty.reshape(0).dtype == np.dtype(np.int64)


def test_library_exports_every_declared_symbol():
    lib = helpers.load_lib()
    assert os.path.basename(lib._filename).startswith("multi_mesh")
    for name in _declared_functions():
        assert hasattr(lib, name), f"{name} missing from {lib._filename}"
    assert helpers.load_lib() is lib  # cached handle, like the reference loader


def test_no_silent_cpu_fallback_without_gpu():
    lib = helpers.load_lib()
    if lib.mm_device_count() > 0:
        pytest.skip("a GPU is present")
    from multimesh_amd.device import Context

    with pytest.raises(helpers.MultiMeshHipError):
        Context(0)
    # the legacy symbol reports failure through its return code, never computes on the CPU
    nn = np.zeros((4, 2), np.int64)
    conn = np.arange(8, dtype=np.int64)[None, :].copy()
    enc = np.zeros((4, 8), np.int64)
    w = np.zeros((4, 8))
    nodes = np.random.default_rng(0).uniform(size=(8, 3))
    pts = np.full((4, 3), 0.5)
    rc = lib.triLinearInterpolator(2, 4, nn, conn, enc, nodes, w, pts)
    assert rc < 0 and lib.mm_last_status() < 0
    assert not w.any() and not enc.any()
    with pytest.raises(helpers.MultiMeshHipError):
        helpers.check(rc, "triLinearInterpolator")


def test_argument_validation_needs_no_gpu():
    lib = helpers.load_lib()
    h = C.c_void_p()
    assert lib.mm_context_create(0, None, None) < 0      # null out pointer
    assert lib.mm_gather(None, None, 0, 0, None, None, 0, 8, None, 1) < 0   # null ctx
    assert b"null" in lib.mm_last_error()
