"""The sweep of tests/test_scratch_fill_gpu.py, stated once: which case names which entry points (read without a GPU by the
file's CPU companion) and how a case runs (in the child processes, which alone use the GPU).

A case is ``(run, check)``: ``run(ctx)`` -> the call's results as a list of NumPy arrays and numbers, ``check(results)``
holds them to the CPU statement exactly as the case's own test does.  :func:`sweep` runs a case twice on each of three
contexts created under MM_SCRATCH_FILL = 0x00, 0x5A and 0xFF, checks the first result and demands of the other five the
bits of the first (NaN in the same places, as every table here compares doubles).  The inputs are those of the existing
tests: the tables of test_caller_stream_gpu.py and test_caller_views_gpu.py, the scenarios of test_pool_reuse_gpu.py and
the units' ``*_cases.py`` / guarded_cases.py."""
import os

FILLS = ("0x00", "0x5A", "0xFF")

# ------------------------------------------------------------------------------------------- what names which entry point
_STREAM = {
    "centroid": ("mm_centroid",),
    "knn_k8": ("mm_knn_build", "mm_knn_query"),
    "knn_k64": ("mm_knn_build", "mm_knn_query"),
    "locate_hex8_gather": ("mm_locate_hex8", "mm_gather"),
    "interpolate_hex8": ("mm_interpolate_hex8",),
    "interpolate_hex8_operator": ("mm_interpolate_hex8",),
    "source_interpolate_twice": ("mm_source_create", "mm_interpolate_hex8_on"),
    "first_occurrence": ("mm_first_occurrence",),
    "locate_gll_gather_elem_3d": ("mm_locate_gll", "mm_gather_elem"),
    "locate_gll_gather_elem_2d": ("mm_locate_gll", "mm_gather_elem"),
    "locate_gll_bbox_3d": ("mm_locate_gll_bbox",),
    "locate_gll_bbox_2d": ("mm_locate_gll_bbox",),
    "interpolate_gll_3d": ("mm_interpolate_gll",),
    "interpolate_gll_2d": ("mm_interpolate_gll",),
    "sample_columns_gll": ("mm_sample_columns_gll",),
    "sample_grid": ("mm_sample_grid",),
    "transpose_nodes_apply": ("mm_transpose_create_nodes", "mm_transpose_apply"),
    "transpose_elem_apply": ("mm_transpose_create_elem", "mm_transpose_apply"),
    "gll_mass": ("mm_gll_mass",),
    "weighted_sum": ("mm_weighted_sum",),                    # n = 4097: a chunked sum with a level in scratch
    "divide_rows": ("mm_divide_rows",),
    "diffusion_apply": ("mm_gll_diffusion_apply",),
    "smooth_two_steps": ("mm_gll_diffusion_apply", "mm_pcg_combine", "mm_pcg_scalars", "mm_pcg_direction", "mm_pcg_advance"),
    "gll_gradient": ("mm_gll_gradient",),
    "gll_tensor_apply": ("mm_gll_tensor_apply",),
    "element_deviation": ("mm_element_deviation",),
    "radial_bins": ("mm_radial_bins",),
    "binned_weighted_sum": ("mm_binned_weighted_sum",),      # n = 3 * 4096 + 5: likewise
    "radial_model_apply": ("mm_radial_model_apply",),
    "point_taper": ("mm_point_taper",),
    "order_statistics": ("mm_order_statistics",),
    "clamp": ("mm_clamp",),
    "unique_points_ordered": ("mm_unique_points",),
    "unique_points_any_order": ("mm_unique_points_any_order",),
    "scatter_elements": ("mm_scatter_elements",),
    "fluid_solid_fix_P125": ("mm_fluid_solid_fix",),
    "fluid_solid_fix_P27": ("mm_fluid_solid_fix",),
    "map_to_sphere": ("mm_map_to_sphere",),
    "sphere_ratio": ("mm_sphere_ratio",),
    "scale_points": ("mm_scale_points",),
}
_OWN = {
    "boundary_faces": ("mm_boundary_faces",),
    "boundary_classify": ("mm_boundary_classify",),
    "boundary_nodes": ("mm_boundary_nodes",),
    "cutoff_distance": ("mm_cutoff_distance",),
    "distance_taper": ("mm_distance_taper",),
    "gll_resolution_node_h": ("mm_gll_resolution",),
    "gll_resolution": ("mm_gll_resolution",),
    "arg_extreme_min": ("mm_arg_extreme",),
    "arg_extreme_max": ("mm_arg_extreme",),
    "pcg_combine": ("mm_pcg_combine",),
    "pcg_combine_mass_alone": ("mm_pcg_combine",),
    "pcg_combine_kp_alone": ("mm_pcg_combine",),
    "pcg_scalars_start": ("mm_pcg_scalars",),
    "pcg_scalars_beta": ("mm_pcg_scalars",),
    "pcg_scalars_beta_later": ("mm_pcg_scalars",),
    "pcg_scalars_alpha": ("mm_pcg_scalars",),
    "pcg_direction": ("mm_pcg_direction",),
    "pcg_advance": ("mm_pcg_advance",),
}


def _pick(table, *prefixes):
    return {k: v for k, v in table.items() if k.startswith(prefixes)}


#: group (one child process each) -> case -> the entry points the case calls
GROUPS = {
    "hex8_search": dict(_pick(_STREAM, "centroid", "knn_", "locate_hex8", "interpolate_hex8", "source_", "first_occurrence"),
                        interpolate_hex8_host=("mm_interpolate_hex8_host",)),
    "gll_search": _pick(_STREAM, "locate_gll", "interpolate_gll", "sample_"),
    "gll_tools": _pick(_STREAM, "transpose_", "gll_", "weighted_sum", "divide_rows", "diffusion_apply", "smooth_",
                       "element_deviation"),
    "streaming_tools": _pick(_STREAM, "radial_", "binned_", "point_taper", "order_statistics", "clamp", "unique_", "scatter_",
                             "fluid_solid", "map_to_sphere", "sphere_ratio", "scale_points"),
    "boundary_resolution_pcg": _OWN,
    "refusals": {                                             # the text of a refusal that a kernel's count goes into
        "radial_bins_refused": ("mm_radial_bins",),
        "transpose_nodes_refused": ("mm_transpose_create_nodes",),
    },
    "pool_reuse": {
        "knn_uniform": ("mm_knn_build", "mm_knn_query"),
        "gll_snap": ("mm_locate_gll",),
        "unique": ("mm_unique_points",),
        "knn_graded_tree": ("mm_knn_build", "mm_knn_query"),
        "hex8_lazy": ("mm_interpolate_hex8",),
    },
    "imports": {
        "idw_gather": ("mm_idw_gather",),
        "grid_operator": ("mm_grid_operator",),
        "points_to_elements": ("mm_points_to_elements",),
        "parametrisation": ("mm_convert_parameters", "mm_convert_kernels"),
        "surface": ("mm_boundary_triangles", "mm_surface_distance"),
        "layered": ("mm_layered_model_apply",),
    },
    "earth_models": {
        "harmonics": ("mm_harmonic_model_apply",),
        "harmonic_adjoint": ("mm_harmonic_model_transpose",),
        "harmonic_fit": ("mm_harmonic_model_apply", "mm_harmonic_model_transpose"),
        "frames": ("mm_rotate_points", "mm_rotate_vectors", "mm_local_components"),
        "topography": ("mm_radial_stretch",),
        "regions": ("mm_region_distance",),
        "geodesy": ("mm_geographic_points",),
    },
}
assert set().union(*(set(g) for k, g in GROUPS.items() if k != "pool_reuse")) >= set(_STREAM) | set(_OWN)

#: entry point -> why no sweep case names it
EXCLUDED = {
    "mm_device_count": "takes no context",
    "mm_last_error": "takes no context: the text of the thread's last refusal",
    "mm_last_status": "takes no context",
    "mm_context_create": "creates the context; every sweep case runs on three of them",
    "mm_context_destroy": "destroys the context",
    "mm_synchronize": "a wait, no kernel",
    "mm_device_alloc": "an allocation: the positive control reads its fill back",
    "mm_device_free": "a release",
    "mm_copy_h2d": "a copy of the runtime's, no scratch",
    "mm_copy_d2h": "a copy of the runtime's, no scratch",
    "mm_memset": "a fill of the runtime's, no scratch",
    "mm_knn_destroy": "a release",
    "mm_transpose_destroy": "a release",
    "mm_source_destroy": "a release",
    "mm_set_lazy_lists": "a setter of a host field",
    "mm_set_fp_mode": "a setter of a host field",
    "mm_get_fp_mode": "a getter of a host field",
    "mm_set_profiling": "a setter of a host field",
    "mm_last_locate_stats": "reads the counters of the last locate stage",
    "mm_last_knn_kernels": "a getter of a host field",
    "mm_last_timings": "reads the stage timers",
    "centroid": "legacy host symbol: wraps mm_centroid on the process's default context",
    "triLinearInterpolator": "legacy host symbol: wraps mm_locate_hex8 on the process's default context",
}


def signature_tables():
    """name -> module of every entry point the binding layer declares (helpers.SIGNATURES and the units' own tables)."""
    import importlib

    out = {}
    for module in ("helpers", "parametrisation", "geodesy", "surface", "topography", "frames", "layered", "harmonic_adjoint",
                   "harmonics", "regions"):
        for name in importlib.import_module("multimesh_amd." + module).SIGNATURES:
            out[name] = module
    return out


def swept_symbols(groups=None):
    return {s for cases in (groups or GROUPS).values() for symbols in cases.values() for s in symbols}


# ------------------------------------------------------------------------------------------------------ the child's side
def debug_scratch(ctx):
    """[fill byte or -1, pool base, bytes of the current reservation, fills queued] of mm_debug_scratch"""
    import ctypes as C

    fn = ctx.lib.mm_debug_scratch
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 4)()
    assert fn(ctx.handle, out) == 0
    return list(out)


def context_with_fill(fill):
    """A context created under MM_SCRATCH_FILL=fill (None: unset); the variable is read at creation and not after."""
    from multimesh_amd.device import Context

    if fill is None:
        os.environ.pop("MM_SCRATCH_FILL", None)
    else:
        os.environ["MM_SCRATCH_FILL"] = fill
    try:
        return Context(0)
    finally:
        os.environ.pop("MM_SCRATCH_FILL", None)


class _Env:
    """setenv / delenv of pytest's monkeypatch, for the scenarios of test_pool_reuse_gpu.py"""

    @staticmethod
    def setenv(name, value):
        os.environ[name] = value

    @staticmethod
    def delenv(name, raising=True):
        os.environ.pop(name, None)


def _same(got, want, what):
    from test_caller_stream_gpu import _bits, _same_as

    _same_as(got, want, _bits, what)


def sweep(name, run, check):
    print(name, flush=True)
    first = None
    for fill in FILLS:
        ctx = context_with_fill(fill)
        try:
            before = debug_scratch(ctx)
            assert before[0] == int(fill, 16), (name, before)
            for rep in range(2):
                got = run(ctx)
                if first is None:
                    first = got
                    check(first)
                else:
                    _same(got, first, (name, "fill", fill, "run", rep, "against the first run of fill 0x00"))
        finally:
            ctx.close()


def _numpy(x):
    return x.numpy() if hasattr(x, "numpy") else x


def _table_case(name, make):
    from test_caller_stream_gpu import _bits, _run_reference, _same_as

    case = make()
    return (lambda ctx: _run_reference(ctx, case)[0],
            lambda ref: _same_as(ref, case.expect(ref), case.compare or _bits, (name, "against the CPU")))


def _pool_case(name):
    import test_pool_reuse_gpu as PR

    call = getattr(PR, name)
    kernels = []

    def run(ctx):
        out, ran = call(ctx, _Env)                       # (asserts the kNN kernels the scenario is meant for)
        kernels.append(ran)
        assert ran == kernels[0], (name, ran, kernels[0])
        return list(out)

    return run, lambda ref: None                         # (each scenario's statement is its own file's: here the bits alone)


def _hex8_host():
    import numpy as np
    from test_caller_stream_gpu import _hex8

    d = _hex8()

    def check(ref):
        assert ref[3] == d.nf and all(np.array_equal(a, b) for a, b in zip(ref[:3], (d.vals, d.enc, d.w)))

    return (lambda ctx: list(ctx.interpolate_hex8_host(d.pa, d.ca, d.pb, d.fields, nelem_to_search=20, want_operator=True)), check)


# ---- the units the two tables lack: the inputs and statements of their guarded children, smallest cases first
def _idw_gather():
    import numpy as np
    import guarded_cases as G
    import scattered_cases as SC

    cases = G.scattered_cases()
    todo = [(c, cut, power) for c in cases for cut, power in ((np.inf, 2), (c["cut"], 3))]

    def run(ctx):
        out = []
        for c, cut, power in todo:
            for point_major in (False, True):
                o, nout, near, used = ctx.idw_gather(c["fields"], c["idx"], c["dist"], power=power, max_distance=cut, fill_value=-5.0,
                                                     point_major=point_major, want_nearest=True, want_count=True)
                out += [o.numpy().T if point_major else o.numpy(), nout, near.numpy(), used.numpy()]
        return out

    def check(ref):
        it = iter(ref)
        for c, cut, power in todo:
            want, want_out, want_near, want_used = SC.idw(c["fields"], c["idx"], c["dist"], G.NSRC, power=power, max_distance=cut,
                                                          fill=-5.0)
            for _ in range(2):
                o, nout, near, used = (next(it) for _ in range(4))
                assert nout == want_out and SC.same_bits(o, want) and SC.same_bits(near, want_near), c["name"]
                assert np.array_equal(used, want_used), c["name"]

    return run, check


def _grid_operator():
    import numpy as np
    import guarded_cases as G
    import grid_adjoint_cases as GA
    import grid_import_cases as GI

    cases = G.grid_operator_cases()[:4]                   # n = 8 and 101, a plain box and a global map each

    def run(ctx):
        out = []
        for c in cases:
            depth, lat, lon = c["axes"]
            for clamp in (False, True):
                ids, w, nout, lld = ctx.grid_operator(c["points"], depth, lat, lon, clamp=clamp, lon_periodic=c["periodic"],
                                                      latlondepth=True)
                out += [ids.numpy(), w.numpy(), nout, lld.numpy()]
        return out

    def check(ref):
        it = iter(ref)
        for c in cases:
            depth, lat, lon = c["axes"]
            for clamp in (False, True):
                ids, w, nout, lld = (next(it) for _ in range(4))
                want_ids, want_w, want_out, _ = GA.operator(depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1], clamp, c["periodic"])
                assert nout == want_out and np.array_equal(ids, want_ids) and GI.same_bits(w, want_w), (c["name"], clamp)

    return run, check


def _points_to_elements():
    import numpy as np

    idx = np.random.default_rng(5).integers(0, 27 * 300, 4097)
    return (lambda ctx: [ctx.points_to_elements(ctx.to_device(idx), 27).numpy()],
            lambda ref: np.testing.assert_array_equal(ref[0], idx // 27))


def _parametrisation():
    import parametrisation_cases as PC
    from multimesh_amd import parametrisation as P

    todo = []
    for a, b in PC.PAIRS:
        m = PC.special_rows(a, PC.models(a, 257, 5))
        todo.append((a, b, m, PC.special_rows(b, PC.models(b, 257, 6))))

    def run(ctx):
        out = []
        for a, b, m, k in todo:
            o, count = P.convert_values(m, a, b, context=ctx)
            ko, kcount = P.convert_kernels(k, m, a, b, context=ctx)
            out += [o, count, ko, kcount]
        return out

    def check(ref):
        it = iter(ref)
        for a, b, m, k in todo:
            o, count, ko, kcount = (next(it) for _ in range(4))
            want, kwant = PC.convert(m, a, b), PC.convert_kernels(k, m, a, b)
            assert PC.same_bits(o, want) and count == PC.n_bad(want), (a, b)
            assert PC.same_bits(ko, kwant) and kcount == PC.n_bad(kwant), (a, b)

    return run, check


def _surface():
    import numpy as np
    import boundary_cases as BC
    import surface_cases as SC
    from multimesh_amd import device, surface, synth

    todo = []
    for order, nelem in ((1, 2), (2, 64), (2, 101), (4, 1)):
        gp = np.ascontiguousarray(synth.gll_mesh(9, order, seed=3)[:nelem])
        corners = np.ascontiguousarray(gp[:, BC.corner_nodes(order)])
        faces, _ = BC.boundary_faces(BC.corner_ids(corners)[0])
        side = BC.classify(corners, faces, up=(0.0, 0.0, 1.0))
        todo.append((order, gp, faces, side, gp.reshape(-1, 3)[::3] if nelem > 2 else gp))

    def run(ctx):
        lib = surface.bind(ctx.lib)
        out = []
        for order, gp, faces, side, targets in todo:
            for mask in (0b010, 0b111):
                tri = ctx.empty((len(faces) * 2 * order * order, 3, 3), np.float64)
                T = device._call(lib, "mm_boundary_triangles", ctx.handle, ctx.to_device(gp), len(gp), order, ctx.to_device(faces),
                                 ctx.to_device(side), len(faces), mask, tri, arg_error=True)
                tri = tri.rows(0, T)
                out.append(tri.numpy())
            for cutoff in (0.04, np.inf):                 # (on the triangles of every face)
                d, count = surface.distance_to_triangles(targets, tri, cutoff, context=ctx)
                out += [d.numpy().reshape(-1), count]
        return out

    def check(ref):
        it = iter(ref)
        for order, gp, faces, side, targets in todo:
            for mask in (0b010, 0b111):
                want_tri = SC.boundary_triangles(gp, order, faces, side, mask)
                assert SC.same_bits(next(it), want_tri), (order, len(gp), mask)
            least, _ = SC.surface_distance(targets, want_tri, np.inf)
            for cutoff in (0.04, np.inf):
                want, want_count = SC.with_cutoff(least, cutoff)
                d, count = next(it), next(it)
                assert count == want_count and SC.same_bits(d, want), (order, len(gp), cutoff)

    return run, check


def _layered():
    import numpy as np
    import guarded_cases as G
    import layered_cases as LC
    from multimesh_amd import layered as LY

    cases = [c for c in G.layered_cases() if c["points"].size // 3 <= 101 * 27][:5]
    todo = [(c, lateral, pick) for c in cases for lateral in ("cell", "bilinear")
            for pick in (("node", "element") if c["points"].ndim == 3 else ("node",))]

    def run(ctx):
        out = []
        for c, lateral, pick in todo:
            count = ctx.to_device(np.array([3], dtype=np.int64))
            res = LY.layered_model_apply(ctx, c["points"], c["lat"], c["lon"], c["bounds"], c["values"], lon_periodic=c["periodic"],
                                         lateral=lateral, pick=pick, outside="fill", fill_value=-1.5, want_layers=True,
                                         want_span=True, want_latlondepth=True, noutside=count)
            out += [res[k].numpy() for k in ("latlondepth", "layer", "span", "out")] + [int(count.numpy()[0])]
        return out

    def check(ref):
        it = iter(ref)
        for c, lateral, pick in todo:
            lld, layer, span, o, count = (next(it) for _ in range(5))
            n = c["points"].size // 3
            dp = LC.element_depth(c["points"]) if c["points"].ndim == 3 else None
            want, wlayer, wspan, nout = LC.model_apply(lld.reshape(n, 3), dp, c["lat"], c["lon"], c["bounds"], c["values"],
                                                       getattr(LC, lateral.upper()), getattr(LC, pick.upper()), LC.FILL, -1.5)
            what = (c["name"], lateral, pick)
            assert np.array_equal(layer.reshape(n), wlayer) and count == 3 + nout, what
            assert LC.same_bits_nan(span.reshape(n, 2), wspan) and LC.same_bits_nan(o.reshape(want.shape), want), what

    return run, check


def _harmonics():
    import numpy as np
    import guarded_cases as G
    import harmonic_cases as HC
    from multimesh_amd import harmonics as H

    todo = [(c, extend, mode) for c in G.harmonic_cases() for extend in (False, True) for mode in (0, 2)]

    def run(ctx):
        out = []
        for c, extend, mode in todo:
            vin = ctx.to_device(c["values_in"]) if mode else None
            count = ctx.to_device(np.array([3], dtype=np.int64))
            got = H.harmonic_model_apply(ctx, c["points"], c["radius"], c["coef"], c["lmax"], mode=mode, extend=extend, values_in=vin,
                                         noutside=count)
            out += [got.numpy(), int(count.numpy()[0])]
        return out

    def check(ref):
        it = iter(ref)
        for c, extend, mode in todo:
            want, nout = HC.model_apply(c["points"], c["radius"], c["coef"], c["lmax"], mode=mode, extend=extend,
                                        values_in=c["values_in"] if mode else None)
            got, count = next(it), next(it)
            assert HC.same_bits_nan(got.reshape(want.shape), want) and count == 3 + nout, (c["name"], extend, mode)

    return run, check


def _harmonic_adjoint():
    import numpy as np
    import guarded_cases as G
    import harmonic_adjoint_cases as AC
    import harmonic_cases as HC
    from multimesh_amd import harmonic_adjoint as A

    todo = [(c, weighted, limit) for c in G.harmonic_adjoint_cases() for weighted in (False, True) for limit in c["limits"]]

    def run(ctx):
        out = []
        for c, weighted, limit in todo:
            want_shape = (len(c["values"]), len(c["radius"]), 2, (c["lmax"] + 1) * (c["lmax"] + 2) // 2)
            count = ctx.to_device(np.array([3], dtype=np.int64))
            got = A.harmonic_model_transpose(ctx, c["points"], c["radius"], c["lmax"], c["values"],
                                             weight=c["weight"] if weighted else None, extend=True,
                                             out=ctx.to_device(np.full(want_shape, -7.0)), noutside=count, scratch_limit=limit)
            out += [got.numpy(), int(count.numpy()[0])]
        return out

    def check(ref):
        it = iter(ref)
        for c, weighted, limit in todo:
            want, nout = AC.model_transpose(c["points"], c["radius"], c["lmax"], c["values"],
                                            weight=c["weight"] if weighted else None, extend=True)
            got, count = next(it), next(it)
            assert got.shape == want.shape and HC.same_bits_nan(got, want) and count == 3 + nout, (c["name"], weighted, limit)

    return run, check


def _harmonic_fit():
    import numpy as np
    import harmonic_adjoint_cases as AC
    from multimesh_amd import harmonic_adjoint as A
    from multimesh_amd import harmonics as H
    from test_harmonic_adjoint import FIT_TOLERANCE, fit_case

    import torch

    torch.cuda.init()        # the fit runs on torch tensors: torch finds the device only if it opens it before the library does
    pts, R, f, w = fit_case()

    def run(ctx):
        model, iterations, residual, untouched = A.fit_harmonic_model(pts, f, R, 3, mass=w, damping=50.0, rtol=1e-12, extend=True,
                                                                      context=ctx)
        return [H.pack_coefficients(model.cos["0"], model.sin["0"], 3).reshape(-1), iterations, np.float64(residual),
                np.asarray(untouched)]

    def check(ref):                                       # tests/test_harmonic_adjoint_gpu.py::test_fit_against_lstsq
        got, iterations, residual, untouched = ref
        Hd = AC.dense_matrix(pts, R, 3, extend=True)
        rows, rhs = [np.sqrt(w)[:, None] * Hd, np.sqrt(50.0) * np.eye(60)], [np.sqrt(w) * f, np.zeros(60)]
        want = np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0]
        assert residual <= 1e-12 and iterations < 200 and not untouched.any()
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= FIT_TOLERANCE

    return run, check


def _frames():
    import numpy as np
    import guarded_cases as G
    import frames_cases as FC
    from multimesh_amd import frames as F

    cases = G.frames_cases()

    def run(ctx):
        out = []
        for c in cases:
            R = c["matrix"]
            if "points" in c:
                out += [F.rotate_points(ctx, ctx.to_device(c["points"]), R, transpose=t).numpy() for t in (False, True)]
                continue
            v, pos = c["planes"], c["positions"]
            _, E, P = v.shape
            plane = lambda a: (a, P, E * P, (0, 1, 2))    # noqa: E731
            for transpose in (False, True):
                dst = ctx.to_device(np.full(v.shape, -7.0))
                F.rotate_vectors_on_device(ctx, R, E, P, plane(ctx.to_device(v)), plane(dst), transpose=transpose)
                out.append(dst.numpy())
            for inverse in (False, True):
                dst = ctx.to_device(np.full(v.shape, -7.0))
                F.local_components_on_device(ctx, ctx.to_device(pos), E, P, plane(ctx.to_device(v)), plane(dst), inverse=inverse,
                                             basis="rtp")
                out.append(dst.numpy())
        return out

    def check(ref):
        it = iter(ref)
        for c in cases:
            R = c["matrix"]
            if "points" in c:
                for t in (False, True):
                    assert FC.same_bits_nan(next(it), FC.rotate_points(R, c["points"], t)), c["name"]
                continue
            for t in (False, True):
                assert FC.same_bits_nan(next(it), FC.rotate_vectors(R, c["planes"], t)), c["name"]
            for inverse in (False, True):
                want = FC.local_components(c["positions"], c["planes"], FC.TO_CARTESIAN if inverse else FC.TO_LOCAL, F.BASIS["rtp"])
                assert FC.same_bits_nan(next(it), want), (c["name"], inverse)

    return run, check


def _topography():
    import numpy as np
    import topography_cases as TC
    from multimesh_amd import topography as TP

    todo = [(c, direction, lateral) for c in TC.guarded_cases() for direction in ("apply", "flatten") for lateral in ("cell", "bilinear")]

    def run(ctx):
        out = []
        for c, direction, lateral in todo:
            count = ctx.to_device(np.array([3], dtype=np.int64))
            res = TP.radial_stretch(ctx, ctx.to_device(c["points"]), c["lat"], c["lon"], c["anchors"], c["shifts"],
                                    lon_periodic=c["periodic"], direction=direction, ref_radius=c["ref"] if direction == "apply" else None,
                                    lateral=lateral, outside="keep", want_radius=True, want_latlondepth=True, noutside=count)
            out += [res[k].numpy() for k in ("latlondepth", "points", "radius")] + [int(count.numpy()[0])]
        return out

    def check(ref):
        it = iter(ref)
        for c, direction, lateral in todo:
            lld, points, radius, count = (next(it) for _ in range(4))
            _, r = TC.device_view(c["points"], c["lon"], c["periodic"])
            want, wradius, nout = TC.stretch(lld, r, c["points"], c["ref"] if direction == "apply" else None, c["lat"], c["lon"],
                                             c["anchors"], c["shifts"], getattr(TC, direction.upper()), getattr(TC, lateral.upper()),
                                             TC.KEEP)
            what = (c["name"], direction, lateral)
            assert TC.same_bits_nan(points, want) and TC.same_bits_nan(radius, wradius) and count == 3 + nout, what

    return run, check


def _regions():
    import numpy as np
    import regions_cases as RC
    from multimesh_amd import regions as RG

    cases = RC.guarded_cases()

    def run(ctx):
        out = []
        for c in cases:
            res, n = RG.region_distance_call(ctx, c["points"], c["edges"], c["anchor"], c["anchor_inside"], c["cutoff"], c["scale"],
                                             want_signed=True, want_inside=True, want_info=True)
            out += [res["signed"].numpy().reshape(-1), res["inside"].numpy().reshape(-1), res["info"].numpy(), n]
        return out

    def check(ref):
        it = iter(ref)
        for c in cases:
            signed, inside, info, n = (next(it) for _ in range(4))
            s, want_inside, ni, nhit, ninvalid = RC.region_distance(c["points"], c["edges"], c["anchor"], c["anchor_inside"], c["cutoff"],
                                                                    c["scale"])
            assert n == ni and info.tolist() == [nhit, ninvalid] and RC.same_bits(signed, s), c["name"]
            assert np.array_equal(inside, want_inside), c["name"]

    return run, check


def _geodesy():
    import numpy as np
    import geodesy_cases as GC
    from multimesh_amd import geodesy as G

    ell = GC.constants()
    cases = GC.guarded_cases()

    def run(ctx):
        out = []
        for c in cases:
            src = ctx.to_device(c["points"])
            heights = ctx.to_device(np.full(len(c["points"]), -7.0))
            out.append(G.geographic_points_on_device(ctx, src, ell, radius=ctx.to_device(c["radius"]), height_out=heights).numpy())
            out.append(heights.numpy())
            out.append(G.geographic_points_on_device(ctx, src, ell, G.TO_CARTESIAN).numpy())
        return out

    def check(ref):
        it = iter(ref)
        for c in cases:
            want_r, _ = GC.to_geographic(ell, c["points"], radius=c["radius"])
            _, want_h = GC.to_geographic(ell, c["points"])
            assert GC.same_bits_nan(next(it), want_r) and GC.same_bits_nan(next(it), want_h), c["name"]
            assert GC.same_bits_nan(next(it), GC.from_geographic(ell, c["points"])), c["name"]

    return run, check


def _refused(call):
    """run -> [the text of the exception the call raises]"""
    def run(ctx):
        try:
            call(ctx)
        except Exception as exc:   # noqa: BLE001 -- the text is the result
            return [type(exc).__name__ + ": " + str(exc)]
        raise AssertionError("the call was not refused")

    return run


def _radial_bins_refused():
    import numpy as np
    from test_caller_stream_gpu import _shell_points

    pts, edges = _shell_points(4099, 31), np.linspace(3.0e6, 6.4e6, 8)
    edges[[2, 5]] = edges[[5, 2]]

    def check(ref):
        assert "mm_radial_bins: the edges are not finite and strictly ascending" in ref[0], ref

    return _refused(lambda ctx: ctx.radial_bins(pts, edges)), check


def _transpose_nodes_refused():
    import numpy as np

    rng = np.random.default_rng(21)
    ids, w = rng.integers(0, 1000, (5003, 8)), rng.uniform(0.0, 1.0, (5003, 8))
    ids[[7, 4098, 5002], [0, 3, 7]] = (1000, -1, 1 << 40)

    def check(ref):
        assert "mm_transpose_create_nodes: 3 ids outside [0, 1000)" in ref[0], ref

    return _refused(lambda ctx: ctx.transpose_nodes(ids, w, 1000)), check


_UNIT_CASES = {
    "radial_bins_refused": _radial_bins_refused, "transpose_nodes_refused": _transpose_nodes_refused,
    "interpolate_hex8_host": _hex8_host, "idw_gather": _idw_gather, "grid_operator": _grid_operator,
    "points_to_elements": _points_to_elements, "parametrisation": _parametrisation, "surface": _surface, "layered": _layered,
    "harmonics": _harmonics, "harmonic_adjoint": _harmonic_adjoint, "harmonic_fit": _harmonic_fit, "frames": _frames,
    "topography": _topography, "regions": _regions, "geodesy": _geodesy,
}


def case_of(group, name):
    if group == "pool_reuse":
        return _pool_case(name)
    if name in _UNIT_CASES:
        return _UNIT_CASES[name]()
    from test_caller_views_gpu import ALL_CASES

    return _table_case(name, ALL_CASES[name])


def run_group(group):
    """The child process of one group: every case of GROUPS[group], by name and in the table's order."""
    os.environ.pop("MM_KNN_FORCE_LIST", None)
    cases = {name: case_of(group, name) for name in GROUPS[group]}   # (built before the first context: see _harmonic_fit)
    for name, (run, check) in cases.items():
        sweep(name, run, check)
    print("ok")
