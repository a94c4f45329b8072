"""Kernel preconditioning on the CPU: properties of the NumPy statements of tests/precondition_cases.py, the argument
checks of the three entry points that need no device, the surface of multimesh_amd.precondition and the ValueErrors its
functions raise before they ask for a device."""
import ctypes as C
import inspect

import numpy as np
import pytest

import precondition_cases as PC
from multimesh_amd import api, helpers, precondition, synth
from multimesh_amd.api import GllMesh


# ------------------------------------------------------------------------------------------------------- the taper
def test_smoothstep_stays_in_the_unit_interval():
    """(s*s)*(3.0 - 2.0*s) for s in (0, 1): a product of two non-negative rounded factors, so >= 0; that its roundings never
    carry it above 1 is checked where they could -- next to 1 -- and next to 0, over the denormals and on a dense grid."""
    s = np.concatenate([
        np.linspace(0.0, 1.0, 200001)[1:-1],
        [np.nextafter(1.0, 0.0), np.nextafter(np.nextafter(1.0, 0.0), 0.0), np.nextafter(0.0, 1.0), 5e-324 * 3, 2.0 ** -1022,
         2.0 ** -1023, 2.0 ** -540, 2.0 ** -537, 0.5, np.nextafter(0.5, 1.0)],
        1.0 - 2.0 ** -np.arange(1, 54), 2.0 ** -np.arange(1, 1075).astype(np.float64)])
    s = s[(s > 0) & (s < 1)]
    with np.errstate(under="ignore"):
        t = PC.smoothstep(s)
    assert (t >= 0.0).all() and (t <= 1.0).all()
    assert PC.smoothstep(np.nextafter(1.0, 0.0)) <= 1.0 and PC.smoothstep(5e-324) == 0.0


def test_taper_weight_properties():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1, 1, (4000, 3))
    centres = rng.uniform(-1, 1, (7, 3))
    inner = rng.uniform(0.0, 0.2, 7)
    outer = inner + rng.uniform(0.0, 0.4, 7)
    w, count = PC.taper_weight(pts, centres, inner, outer)
    assert (w >= 0).all() and (w <= 1).all() and 0 < count == np.count_nonzero(w < 1) < len(pts)
    d = np.linalg.norm(pts[:, None, :] - centres[None], axis=2)
    assert (w[(d < inner * (1 - 1e-12)).any(axis=1)] == 0).all()
    assert (w[(d > outer * (1 + 1e-12)).all(axis=1)] == 1).all()
    # the order of the centres does not show
    perm = rng.permutation(7)
    assert PC.same_bits(PC.taper_weight(pts, centres[perm], inner[perm], outer[perm])[0], w)
    # K = 0: all ones
    assert (PC.taper_weight(pts, np.zeros((0, 3)), [], [])[0] == 1).all()


def test_taper_hard_cut_and_nan():
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [np.nextafter(1.0, 0), 0, 0], [np.nextafter(1.0, 2), 0, 0], [np.nan, 0, 0],
                    [0.5, np.nan, 0]])
    w, count = PC.taper_weight(pts, [[0.0, 0, 0]], 1.0, 1.0)     # outer == inner: no division decides anything
    assert w.tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0] and count == 3
    w, _ = PC.taper_weight(pts, [[0.0, 0, 0]], 0.0, 0.0)         # a centre on a node with inner = outer = 0 cuts that node
    assert w.tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    out, w, _ = PC.taper_apply(pts, [[0.0, 0, 0]], 0.5, 2.0, np.arange(12.0).reshape(2, 6))
    assert w[0] == 0 and 0 < w[1] < 1 and w[4] == 1 and w[5] == 1 and PC.same_bits(out[1], w * np.arange(6.0, 12.0))


# ------------------------------------------------------------------------------------------------------ the select
def _wild(rng, n):
    v = np.concatenate([rng.normal(size=n) * 10.0 ** rng.uniform(-300, 300, n),
                        [0.0, -0.0, 0.0, -0.0, np.inf, -np.inf, np.inf, 5e-324, -5e-324, 2.0 ** -1040, -(2.0 ** -1060),
                         2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308]])
    return rng.permutation(v)


def test_key_order_is_the_numeric_order():
    rng = np.random.default_rng(11)
    v = _wild(rng, 5000)
    k = PC.keys(v)
    order = np.argsort(k, kind="stable")
    s = v[order]
    assert np.array_equal(s, np.sort(v))                          # (== : -0.0 and +0.0 compare equal there)
    zeros = s[s == 0]
    assert np.signbit(zeros[:2]).all() and not np.signbit(zeros[2:]).any()      # -0.0 ahead of +0.0
    assert PC.same_bits(PC.values_of_keys(k), v)
    ka = PC.keys(v, absolute=True)
    assert np.array_equal(PC.values_of_keys(np.sort(ka)), np.sort(np.abs(v)))
    assert (np.diff(np.sort(k).astype(object)) >= 0).all()


@pytest.mark.parametrize("method", ["lower", "higher"])
def test_order_statistics_statement_against_numpy(method):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(2, 1001))
    v[1, ::7] = np.nan
    q = [0.0, 0.25, 0.5, 0.999, 1.0]
    out, nvalid = PC.order_statistics(v, q, method=method)
    assert nvalid.tolist() == [1001, 1001 - 143]
    for c in range(2):
        valid = v[c][~np.isnan(v[c])]
        assert np.array_equal(out[c], np.quantile(valid, q, method=method))
    out, _ = PC.order_statistics(v, q, absolute=True, method=method)
    assert np.array_equal(out[0], np.quantile(np.abs(v[0]), q, method=method))
    out, nvalid = PC.order_statistics(np.full((1, 5), np.nan), [0.5])
    assert np.isnan(out).all() and nvalid[0] == 0


def test_clamp_statement():
    v = np.array([[-3.0, -0.0, 0.0, np.nan, 2.0, 5.0, -np.inf]])
    out, n = PC.clamp(v, upper=[2.0], symmetric=True)
    assert PC.same_bits_nan(out, [[-2.0, -0.0, 0.0, np.nan, 2.0, 2.0, -2.0]]) and n.tolist() == [3]
    out, n = PC.clamp(v, lower=[0.0])
    assert PC.same_bits_nan(out, [[0.0, -0.0, 0.0, np.nan, 2.0, 5.0, 0.0]]) and np.signbit(out[0, 1]) and n.tolist() == [2]


# --------------------------------------------------------------------------- argument checks that need no device
def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = helpers.load_lib()
    fake = C.create_string_buffer(1 << 16)                        # a non-null context that is never looked into
    ctx = C.cast(fake, C.c_void_p)
    buf = C.cast(C.create_string_buffer(4096), C.c_void_p)
    assert lib.mm_point_taper(None, buf, 1, 1, buf, buf, buf, 1, 0, None, None, buf) == -1
    assert b"mm_point_taper" in lib.mm_last_error() and b"null" in lib.mm_last_error()
    assert lib.mm_order_statistics(None, buf, 1, 1, 0, buf, 1, 0, buf, buf) == -1
    assert b"mm_order_statistics" in lib.mm_last_error()
    assert lib.mm_clamp(None, buf, 1, 1, None, buf, 0, buf, None) == -1
    assert b"mm_clamp" in lib.mm_last_error()
    for P in (0, 257, -1):
        assert lib.mm_point_taper(ctx, buf, 1, P, buf, buf, buf, 1, 0, None, None, buf) == -1
        assert b"P must lie" in lib.mm_last_error()
    assert lib.mm_point_taper(ctx, buf, -1, 1, buf, buf, buf, 1, 0, None, None, buf) == -1
    assert lib.mm_point_taper(ctx, buf, 1, 1, buf, buf, buf, (1 << 20) + 1, 0, None, None, buf) == -1
    for m in (0, 17, -3):
        assert lib.mm_order_statistics(ctx, buf, 1, 1, 0, buf, m, 0, buf, buf) == -1
        assert b"m must lie" in lib.mm_last_error()
    for method in (-1, 2):
        assert lib.mm_order_statistics(ctx, buf, 1, 1, 0, buf, 1, method, buf, buf) == -1
        assert b"method" in lib.mm_last_error()
    assert lib.mm_order_statistics(ctx, buf, -1, 1, 0, buf, 1, 0, buf, buf) == -1
    assert lib.mm_clamp(ctx, buf, 1, 1, buf, buf, 1, buf, None) == -1        # symmetric with a lower bound
    assert b"symmetric" in lib.mm_last_error()
    assert lib.mm_clamp(ctx, buf, -1, 1, None, buf, 0, buf, None) == -1


# ------------------------------------------------------------------------------------------------------ the surface
SURFACE = {
    "taper_around_points": "(mesh_or_points, centres, inner, outer, geocentric=False, context=None)",
    "cut_around_points": "(mesh, params, centres, inner, outer, geocentric=False, context=None)",
    "field_quantiles": "(values_or_mesh, q, params=None, method='linear', absolute=False, context=None)",
    "clip_fields": "(values_or_mesh, params=None, quantile=None, lower=None, upper=None, symmetric=True, context=None)",
    "precondition_kernel": "(mesh, params, sources=None, receivers=None, source_cut=None, receiver_cut=None, "
                           "clip_quantile=None, geocentric=True, context=None)",
}


def test_the_modules_surface():
    assert sorted(precondition.__all__) == sorted(SURFACE)
    for name, signature in SURFACE.items():
        fn = getattr(precondition, name)
        assert str(inspect.signature(fn)) == signature, name
        assert (fn.__doc__ or "").strip(), name
    assert len(api.__all__) == 71 and not set(SURFACE) & set(api.__all__)     # the api package is as it was
    for name in ("point_taper", "order_statistics", "clamp"):
        assert (getattr(helpers, "SIGNATURES")["mm_" + name] and getattr(__import__("multimesh_amd.device").device.Context,
                                                                       name).__doc__)


def _mesh():
    gp = synth.gll_mesh(3, 2, seed=1)
    return GllMesh(gp, 2, {"K": np.ones(gp.shape[:2])})


@pytest.mark.parametrize("inner, outer", [(-1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.inf), ([0.0, 0.0], 1.0),
                                          (None, 1.0), (0.0, None)])
def test_bad_radii_raise_before_any_device_work(inner, outer):
    mesh = _mesh()
    with pytest.raises(ValueError):
        precondition.taper_around_points(mesh, [[0.5, 0.5, 0.5]], inner, outer)
    with pytest.raises(ValueError):
        precondition.cut_around_points(mesh, ["K"], [[0.5, 0.5, 0.5]], inner, outer)


def test_other_value_errors_before_any_device_work():
    mesh = _mesh()
    with pytest.raises(ValueError):
        precondition.taper_around_points(mesh, [[0.5, np.nan, 0.5]], 0.0, 1.0)
    with pytest.raises(ValueError):
        precondition.taper_around_points(mesh, [[0.5, 0.5]], 0.0, 1.0)
    with pytest.raises(ValueError):
        precondition.cut_around_points(mesh, ["VS"], [[0.5, 0.5, 0.5]], 0.0, 1.0)
    for q in (-0.1, 1.5, np.nan, [0.5] * 17, []):
        with pytest.raises(ValueError):
            precondition.field_quantiles(np.ones(10), q)
        with pytest.raises(ValueError):
            precondition.clip_fields(np.ones(10), quantile=q)
    with pytest.raises(ValueError):
        precondition.field_quantiles(np.ones(10), 0.5, method="nearest")
    with pytest.raises(ValueError):
        precondition.clip_fields(np.ones(10))                                  # no bound at all
    with pytest.raises(ValueError):
        precondition.clip_fields(np.ones(10), quantile=0.5, upper=1.0)
    with pytest.raises(ValueError):
        precondition.clip_fields(np.ones(10), lower=-1.0, upper=1.0)           # symmetric (the default) takes upper alone
    with pytest.raises(ValueError):
        precondition.clip_fields(np.ones((2, 10)), upper=[1.0, 2.0, 3.0])
    # a cut list without its radii, radii without their list
    src = [[0.0, 0.0, 1000.0]]
    with pytest.raises(ValueError):
        precondition.precondition_kernel(mesh, ["K"], sources=src)
    with pytest.raises(ValueError):
        precondition.precondition_kernel(mesh, ["K"], receivers=src, source_cut=(1.0, 2.0))
    with pytest.raises(ValueError):
        precondition.precondition_kernel(mesh, ["K"], source_cut=(1.0, 2.0))
    with pytest.raises(ValueError):
        precondition.precondition_kernel(mesh, ["K"], sources=src, source_cut=(2.0, 1.0))
    with pytest.raises(ValueError):
        precondition.precondition_kernel(mesh, ["K"], sources=src, source_cut=(1.0, 2.0), clip_quantile=1.5)
