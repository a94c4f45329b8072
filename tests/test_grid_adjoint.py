"""The grid-import operator and its adjoint, the parts that need no GPU: the NumPy statement of tests/grid_adjoint_cases.py
against a dense matrix, the host's fold and flip helpers against a dense periodic example, and the declarations."""
import ctypes as C
import os

import numpy as np
import pytest

import grid_adjoint_cases as GA
import grid_import_cases as G
from multimesh_amd import api, helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small():
    depth, lat, lon = np.array([0.0, 30_000.0, 100_000.0]), np.linspace(-3.0, 3.0, 4), np.linspace(-4.0, 4.0, 5)
    pts = GA.random_points(50, depth, lat, lon, 0.075, seed=3)
    lld = G.latlondepth(pts)
    return depth, lat, lon, lld


@pytest.mark.parametrize("clamp", [False, True])
def test_statement_transpose_is_the_transpose_of_the_dense_matrix(clamp):
    depth, lat, lon, lld = _small()
    nsrc = 3 * 4 * 5
    ids, w, nout, inside = GA.operator(depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1], clamp=clamp)
    assert (nout == 0 and inside.all()) if clamp else 0 < nout < 50
    A = GA.dense(ids, w, nsrc)
    rng = np.random.default_rng(0)
    v = rng.normal(size=(2, 50))
    want = np.zeros((2, nsrc))
    for n in range(50):                                      # column sums in ascending n, every product rounded on its own
        want = want + A[n][None, :] * v[:, n, None]
    assert G.same_bits(GA.transpose(ids, w, v, nsrc), want)
    assert np.abs(GA.transpose(ids, w, v, nsrc) - v @ A).max() <= 50 * GA.EPS * np.abs(v).max()
    # and the gather is the matrix itself
    m = rng.normal(size=(1, nsrc))
    assert np.abs(GA.gather(m, ids, w) - m @ A.T).max() <= 16 * GA.EPS * np.abs(m).max()
    # <G m, g> = <m, G^T g>
    g = rng.normal(size=50)
    lhs, rhs = np.dot(GA.gather(m, ids, w)[0], g), np.dot(m[0], GA.transpose(ids, w, g, nsrc)[0])
    assert abs(lhs - rhs) <= 2 * (8 * 50 + 2) * GA.EPS * np.abs(w * m[0][ids] * g[:, None]).sum()


def test_rows_inside_sum_to_one_and_rows_outside_are_zero():
    pts = GA.mixed_points()
    lld = G.latlondepth(pts)
    ids, w, nout, inside = GA.operator(G.DEPTH, G.LAT, G.LON, lld[:, 2], lld[:, 0], lld[:, 1])
    assert 1900 <= len(pts) <= 2100 and 0.1 * len(pts) < nout < 0.4 * len(pts) and not inside[-1]
    assert np.abs(w[inside].sum(axis=1) - 1.0).max() <= 4 * GA.EPS
    assert (w[inside] >= 0.0).all() and ids.min() == 0 and ids.max() == 7 * 9 * 11 - 1
    assert not w[~inside].any() and not np.signbit(w[~inside]).any() and not ids[~inside].any()
    # an axis of length 1: two corners share an id, with the weights 1 * ... and 0 * ...
    ids1, w1, _, in1 = GA.operator(G.DEPTH[3:4], G.LAT, G.LON, lld[:, 2], lld[:, 0], lld[:, 1])
    assert np.array_equal(ids1[:, :4], ids1[:, 4:]) and not w1[:, 4:].any() and in1.sum() > inside.sum()
    assert np.abs(w1[in1].sum(axis=1) - 1.0).max() <= 4 * GA.EPS


def test_fold_and_flips_against_a_dense_periodic_example():
    """A global grid with a descending latitude axis and longitudes 0 ... 300: prepare_regular_grid flips the latitudes
    and appends the column 360.  With P the 0/1 matrix of that layout change, the import in the caller's layout is
    G_prepared P, so its transpose is P^T G_prepared^T: the fold."""
    depth, lat, lon = np.array([0.0, 50_000.0]), np.array([60.0, 20.0, -20.0, -60.0]), np.arange(0.0, 360.0, 60.0)
    shape = (2, 4, 6)
    rng = np.random.default_rng(5)
    field = rng.normal(size=shape)
    d, la, lo, data, _, periodic = api.prepare_regular_grid(api.RegularGrid(depth, lat, lon, {"v": field}))
    d0, la0, lo0, data0, names, periodic0 = api.prepare_regular_grid(api.RegularGrid(depth, lat, lon, {"v": field}), [])
    assert periodic and periodic0 and names == [] and data0.shape == (0, 2, 4, 7)
    assert np.array_equal(lo, lo0) and np.array_equal(la, la0) and np.array_equal(d, d0) and lo[-1] == 360.0
    flipped, appended = (False, True, False), True
    assert G.same_bits(data[0], GA.to_prepared(field, flipped, appended))
    assert G.same_bits(api.to_prepared_layout(field, flipped, appended), data[0])
    ncaller, nprep = field.size, data[0].size
    index = GA.to_prepared(np.arange(ncaller).reshape(shape), flipped, appended).reshape(-1)
    P = np.zeros((nprep, ncaller))
    P[np.arange(nprep), index] = 1.0
    assert np.array_equal(P @ field.reshape(-1), data[0].reshape(-1))
    x = rng.normal(size=(3, 2, 4, 7))
    want = (x.reshape(3, nprep) @ P).reshape((3,) + shape)
    assert G.same_bits(api.fold_to_caller_layout(x, flipped, appended), want)
    assert G.same_bits(GA.fold(x, flipped, appended), want)
    # points all round the globe: G^T in the caller's layout is the transpose of the dense G_prepared P
    pts = G.sphere_points(60, seed=4, rmin=G.R_EARTH - 50_000.0, rmax=G.R_EARTH)
    lld = G.latlondepth(pts)
    ids, w, nout, _ = GA.operator(d, la, lo, lld[:, 2], lld[:, 0], lld[:, 1], periodic=True)
    assert 0 < nout < 30                                     # (beyond +-60 degrees of latitude)
    A = GA.dense(ids, w, nprep) @ P
    v = rng.normal(size=(1, 60))
    got = api.fold_to_caller_layout(GA.transpose(ids, w, v, nprep).reshape(1, 2, 4, 7), flipped, appended)
    assert np.abs(got.reshape(-1) - v[0] @ A).max() <= 64 * GA.EPS * np.abs(v).max()
    # every flip on its own, and none
    for flips in ((True, False, False), (False, False, True), (True, True, True), (False, False, False)):
        for app in (False, True):
            y = rng.normal(size=(2, 3, 4, 5 + app))
            a = rng.normal(size=(2, 3, 4, 5))
            assert G.same_bits(api.fold_to_caller_layout(y, flips, app), GA.fold(y, flips, app))
            assert G.same_bits(api.to_prepared_layout(a, flips, app), GA.to_prepared(a, flips, app))
            lhs, rhs = np.sum(GA.to_prepared(a, flips, app) * y), np.sum(a * GA.fold(y, flips, app))
            assert abs(lhs - rhs) <= 256 * GA.EPS * np.abs(a).max() * np.abs(y).max()


def test_chunk_rule_of_the_statement():
    depth, lat, lon, lld = _small()
    ids, w, _, _ = GA.operator(depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1])
    v = np.random.default_rng(1).normal(size=(2, 50)) * 10.0 ** np.random.default_rng(2).uniform(-6, 6, size=(2, 50))
    whole = GA.transpose(ids, w, v, 60)
    assert G.same_bits(GA.chunked_transpose(ids, w, v, 60, 50), whole)
    assert G.same_bits(GA.chunked_transpose(ids, w, v, 60, 1000), whole)
    for chunk in (1, 7, 49):
        got = GA.chunked_transpose(ids, w, v, 60, chunk)
        assert np.abs(got - whole).max() <= 50 * GA.EPS * np.abs(w[:, :, None] * v.T[:, None, :]).max() * 50


def test_refusals_need_no_device():
    grid = api.RegularGrid(G.DEPTH, G.LAT, G.LON, {})
    pts = G.AXIS_POINTS * 6.3e6
    with pytest.raises(ValueError, match="keep"):
        api.grid_import_operator(grid, pts, outside="keep")
    with pytest.raises(ValueError, match="outside"):
        api.grid_import_operator(grid, pts, outside="nearest")
    with pytest.raises(ValueError, match="keep"):
        api.regular_grid_adjoint(grid, api.GllMesh(np.zeros((1, 8, 3)), 1), [], outside="keep")
    bad = api.RegularGrid(G.DEPTH, G.LAT, G.LON, {})
    bad.coords["latitude"] = np.where(np.arange(9) == 2, 7.0, G.LAT)
    with pytest.raises(ValueError, match="monotone"):
        api.grid_import_operator(bad, pts)


def test_a_two_dimensional_mesh_is_refused_before_a_device_is_asked_for():
    grid = api.RegularGrid(G.DEPTH, G.LAT, G.LON, {})
    flat = api.GllMesh(np.zeros((2, 4, 2)), 1, {"K": np.zeros((2, 4))})
    with pytest.raises(ValueError, match="3-D"):
        api.regular_grid_adjoint(grid, flat, ["K"])


def test_periodicity_is_detected_as_the_import_detects_it():
    """A -180 ... 180 axis wraps when the end columns of the grid's variables agree, as prepare_regular_grid decides for
    the import of that grid; a grid without variables has only its axes to go by."""
    from multimesh_amd.api.grids import _operator_grid

    lat, depth, lon = np.linspace(-90.0, 90.0, 37), np.array([0.0, 1.0e6]), np.linspace(-180.0, 180.0, 73)
    same = G.periodic_field(lat, lon, depth)
    differ = same + lon[None, None, :]
    for data_vars in ({"v": same}, {"v": differ}, {"a": same, "b": differ}, {"v": differ[::-1, :, ::-1]}):
        grid = api.RegularGrid(depth, lat, lon, data_vars)
        want = api.prepare_regular_grid(grid)[5]
        _, axes, periodic, flipped, appended, clamp = _operator_grid(grid, "fill", None)
        assert periodic == want == (list(data_vars) == ["v"] and data_vars["v"] is same) and not appended and not clamp
        assert np.array_equal(axes[2], api.prepare_regular_grid(grid)[2])
        assert _operator_grid(grid, "fill", True)[2] and not _operator_grid(grid, "clamp", False)[2]
    assert _operator_grid(api.RegularGrid(depth, lat, lon, {}), "fill", None)[2]
    # a descending 0 ... 357.5 axis: flipped, detected, closed
    lon_d = np.arange(0.0, 360.0, 2.5)[::-1]
    grid = api.RegularGrid(depth, lat, lon_d, {"v": G.periodic_field(lat, lon_d, depth)})
    _, axes, periodic, flipped, appended, _ = _operator_grid(grid, "fill", None)
    assert periodic and appended and flipped == (False, False, True) and axes[2][-1] == 360.0


def test_header_declares_and_the_signature_table_holds_mm_grid_operator():
    with open(os.path.join(ROOT, "include", "multimesh_hip.h")) as f:
        header = f.read()
    assert "int64_t mm_grid_operator(mm_context *ctx, const double *points_d, int64_t npoints," in header
    restype, argtypes = helpers.SIGNATURES["mm_grid_operator"]
    assert restype is C.c_int64 and len(argtypes) == 14 and "mm_grid_operator" in helpers.EXPORTED_SYMBOLS
    assert argtypes[9] is C.c_int and argtypes[10] is C.c_int and argtypes[2] is C.c_int64
    order = list(helpers.EXPORTED_SYMBOLS)
    assert order.index("mm_grid_operator") == order.index("mm_sample_grid") + 1
    assert hasattr(helpers.load_lib(), "mm_grid_operator")
    assert callable(api.grid_import_operator) and callable(api.regular_grid_adjoint)
    assert "grid_operator" in dir(__import__("multimesh_amd.device").device.Context)
