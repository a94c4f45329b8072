"""Library loading helper -- the drop-in for reference ``multi_mesh/helpers.py:22-84``.

Same contract as the reference's ``load_lib()``: glob ``<package>/lib/multi_mesh*.so``, open it
with ``ctypes.CDLL``, declare the argument types of the two legacy symbols (``centroid``,
``triLinearInterpolator``), cache the handle in a module-level list, and raise ``ValueError``
when no library is found.  Differences, on purpose:

* scalar arguments are declared ``c_int64`` (the C signature is ``long long``; the reference's
  ``c_int`` only works by accident of the x86-64 calling convention);
* the ``mm_*`` device-pointer entry points of ``include/multimesh_hip.h`` are declared too;
* there is NO CPU fallback: the library is HIP code for gfx950 and every compute call fails
  (``MultiMeshHipError``) when no GPU is usable.
"""
from __future__ import annotations

import ctypes as C
import glob
import os

import numpy as np

#: where the built library lives: <this package>/lib (same place the reference looks, helpers.py:22-27)
LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
#: the opened library, kept for the life of the process (the reference keeps its handle the same way)
cache = []

MM_OK = 0
MM_KNN_MAX_K = 64
MM_FP_EXACT = 0
MM_FP_TOL = 1
MM_SAMPLE_CHUNK_BYTES = 1 << 34   # include/multimesh_hip.h: per-target scratch of one automatic chunk of mm_sample_columns_gll
MM_SAMPLE_STAGE_BYTES = 96
# include/multimesh_hip.h: slots of the PCG state block (8 doubles per system) and the phases of mm_pcg_scalars
MM_PCG_STATE = 8
MM_PCG_RZ, MM_PCG_RZ_OLD, MM_PCG_PAP, MM_PCG_BB, MM_PCG_ALPHA, MM_PCG_BETA, MM_PCG_ACTIVE = range(7)
MM_PCG_PHASE_START, MM_PCG_PHASE_BETA, MM_PCG_PHASE_ALPHA = range(3)
STAGES = ("centroid", "knn_build", "knn_query", "locate", "gather", "knn_cell", "locate_pass0")


class MultiMeshHipError(RuntimeError):
    """A negative MM_ERR_* code came back from multi_mesh_hip.so."""


i32, i64, usize, f64, vp = C.c_int, C.c_int64, C.c_size_t, C.c_double, C.c_void_p
# the two legacy symbols take NumPy arrays (reference helpers.py:43-81); their scalars are long long
_I64_2D = np.ctypeslib.ndpointer(dtype=np.int64, ndim=2, flags=["C_CONTIGUOUS"])
_F64_2D = np.ctypeslib.ndpointer(dtype=np.float64, ndim=2, flags=["C_CONTIGUOUS"])

#: name -> (restype, argtypes) of every function include/multimesh_hip.h declares, in the header's order; load_lib applies
#: it and tests/test_abi.py compares it with the header argument by argument.  vp stands for any pointer.
SIGNATURES = {
    "centroid": (None, (i64, i64, i64, _I64_2D, _F64_2D, _F64_2D)),
    "triLinearInterpolator": (i64, (i64, i64, _I64_2D, _I64_2D, _I64_2D, _F64_2D, _F64_2D, _F64_2D)),
    "mm_device_count": (i32, ()),
    "mm_last_error": (C.c_char_p, ()),
    "mm_last_status": (i32, ()),
    "mm_context_create": (i32, (i32, vp, C.POINTER(vp))),
    "mm_context_destroy": (None, (vp,)),
    "mm_synchronize": (i32, (vp,)),
    "mm_device_alloc": (i32, (vp, usize, C.POINTER(vp))),
    "mm_device_free": (i32, (vp, vp)),
    "mm_copy_h2d": (i32, (vp, vp, vp, usize)),
    "mm_copy_d2h": (i32, (vp, vp, vp, usize)),
    "mm_memset": (i32, (vp, vp, i32, usize)),
    "mm_centroid": (i32, (vp, i64, i64, i64, vp, vp, vp)),
    "mm_knn_build": (i32, (vp, vp, i64, i64, C.POINTER(vp))),
    "mm_knn_query": (i32, (vp, vp, vp, i64, i64, vp, vp)),
    "mm_knn_destroy": (None, (vp, vp)),
    "mm_locate_hex8": (i64, (vp, i64, i64, vp, vp, i64, i32, vp, vp, vp, vp)),
    "mm_gather": (i32, (vp, vp, i64, i64, vp, vp, i64, i64, vp, i32)),
    "mm_locate_gll": (i64, (vp, i32, i32, i64, i64, vp, vp, i64, vp, f64, i32, vp, vp)),
    "mm_locate_gll_bbox": (i64, (vp, i32, i32, i64, i64, vp, vp, i64, vp, vp, vp)),
    "mm_gather_elem": (i32, (vp, vp, i64, i64, vp, vp, i64, i64, vp, i32)),
    "mm_interpolate_gll": (i64, (vp, i32, i32, vp, i64, vp, i64, vp, i64, i64, f64, i32, vp, vp, vp)),
    "mm_sample_columns_gll": (i64, (vp, i32, vp, i64, vp, i64, vp, i64, vp, i64, i32, vp, i64, i64, f64, f64, i64, vp,
                                  vp)),
    "mm_sample_grid": (i64, (vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, f64, vp, vp)),
    "mm_grid_operator": (i64, (vp, vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, vp, vp, vp)),
    "mm_transpose_create_nodes": (i32, (vp, vp, vp, i64, i64, i64, C.POINTER(vp))),
    "mm_transpose_create_elem": (i32, (vp, vp, vp, i64, i64, i64, C.POINTER(vp))),
    "mm_transpose_apply": (i32, (vp, vp, vp, i64, i32, vp)),
    "mm_transpose_destroy": (None, (vp, vp)),
    "mm_gll_mass": (i64, (vp, i32, i32, vp, i64, vp, vp, vp, vp)),
    "mm_weighted_sum": (i32, (vp, vp, vp, i64, i64, vp)),
    "mm_divide_rows": (i32, (vp, vp, vp, i64, i64, vp)),
    "mm_gll_diffusion_apply": (i32, (vp, i32, i32, vp, i64, vp, vp, vp, i64, f64, vp, i32, f64, vp, vp)),
    "mm_gll_gradient": (i32, (vp, i32, i32, vp, i64, vp, vp, i64, vp, vp, vp, vp)),
    "mm_gll_tensor_apply": (i32, (vp, i32, i32, i32, vp, i32, vp, vp, i64, i64, vp, vp)),
    "mm_element_deviation": (i32, (vp, i32, i64, vp, vp, i64, vp, vp)),
    "mm_radial_bins": (i64, (vp, vp, i64, vp, i64, vp, vp)),
    "mm_binned_weighted_sum": (i32, (vp, vp, vp, vp, i64, i64, i64, i32, vp, vp)),
    "mm_radial_model_apply": (i32, (vp, vp, i64, i64, vp, vp, i64, i64, i32, vp, vp)),
    "mm_point_taper": (i64, (vp, vp, i64, i64, vp, vp, vp, i64, i64, vp, vp, vp)),
    "mm_order_statistics": (i32, (vp, vp, i64, i64, i32, vp, i64, i32, vp, vp)),
    "mm_clamp": (i32, (vp, vp, i64, i64, vp, vp, i32, vp, vp)),
    "mm_boundary_faces": (i64, (vp, vp, i64, i64, vp, vp)),
    "mm_boundary_classify": (i32, (vp, vp, i64, vp, i64, i32, f64, f64, f64, f64, vp)),
    "mm_boundary_nodes": (i64, (vp, vp, i64, i32, vp, vp, i64, i32, vp)),
    "mm_cutoff_distance": (i64, (vp, vp, i64, vp, i64, f64, vp)),
    "mm_distance_taper": (i64, (vp, vp, i64, f64, f64, i64, vp, vp, vp, vp, vp)),
    "mm_gll_resolution": (i32, (vp, i32, i32, vp, i64, vp, i64, vp, i64, vp, vp, vp)),
    "mm_arg_extreme": (i32, (vp, vp, i64, i64, i32, vp, vp, vp)),
    "mm_idw_gather": (i64, (vp, vp, i64, i64, vp, vp, i64, i64, i32, f64, i32, f64, vp, i32, vp, vp)),
    "mm_pcg_combine": (i32, (vp, vp, vp, f64, vp, i64, i64, vp)),
    "mm_pcg_scalars": (i32, (vp, vp, i64, i32, f64, vp)),
    "mm_pcg_direction": (i32, (vp, vp, vp, i64, i64, vp)),
    "mm_pcg_advance": (i32, (vp, vp, vp, vp, i64, i64, vp, vp)),
    "mm_unique_points": (i64, (vp, vp, i64, i64, vp, vp)),
    "mm_unique_points_any_order": (i64, (vp, vp, i64, i64, vp, vp)),
    "mm_scatter_elements": (i32, (vp, vp, i64, i64, vp, vp, i64, i64, i64, vp)),
    "mm_map_to_sphere": (i32, (vp, vp, i64, vp, i64, vp, f64, vp)),
    "mm_first_occurrence": (i64, (vp, vp, i64, i64, vp)),
    "mm_sphere_ratio": (i32, (vp, vp, i64, vp, i64, vp, f64, vp)),
    "mm_scale_points": (i32, (vp, vp, i64, vp, vp)),
    "mm_points_to_elements": (i32, (vp, vp, i64, i64)),
    "mm_fluid_solid_fix": (i64, (vp, vp, vp, vp, i64, i64, i64, i64)),
    "mm_interpolate_hex8": (i64, (vp, vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, vp, vp)),
    "mm_source_create": (i32, (vp, vp, i64, vp, i64, C.POINTER(vp))),
    "mm_source_destroy": (None, (vp, vp)),
    "mm_interpolate_hex8_on": (i64, (vp, vp, vp, i64, vp, i64, i64, vp, vp, vp)),
    "mm_interpolate_hex8_host": (i64, (vp, vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, vp, vp)),
    "mm_set_lazy_lists": (i32, (vp, i32)),
    "mm_set_fp_mode": (i32, (vp, i32)),
    "mm_get_fp_mode": (i32, (vp,)),
    "mm_last_locate_stats": (i32, (vp, C.POINTER(C.c_longlong))),
    "mm_last_knn_kernels": (i32, (vp, C.POINTER(i32))),
    "mm_set_profiling": (i32, (vp, i32)),
    "mm_last_timings": (i32, (vp, C.POINTER(f64), i32)),
}

#: every symbol include/multimesh_hip.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = tuple(SIGNATURES)


def load_lib():
    if cache:
        return cache[0]
    # any file called multi_mesh*.so in lib/ qualifies, the first in sorted order wins (the contract of
    # the reference loader: same glob, same exception type when nothing is there)
    candidates = sorted(glob.glob(os.path.join(LIB_DIR, "multi_mesh*.so")))
    if not candidates:
        raise ValueError(
            f"no multi_mesh*.so under {LIB_DIR}: build multi_mesh_hip.so with `make -C multimesh_amd/csrc` "
            "or `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    lib = C.CDLL(candidates[0])
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    lib._filename = candidates[0]
    cache.append(lib)
    return lib


def check(rc, what="multi_mesh_hip call"):
    """Raise on a negative return code; pass non-negative values (counts) through."""
    if rc < 0:
        msg = load_lib().mm_last_error().decode(errors="replace")
        raise MultiMeshHipError(f"{what} failed with code {rc}: {msg}")
    return rc
