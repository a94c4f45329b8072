"""Scattered import, the parts that need no GPU: properties of the NumPy statement of mm_idw_gather
(tests/scattered_cases.py), PointCloud, the chunk planner, the argument checks of multimesh_amd.scattered (every one raises
before a device is asked for) and the binding table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scattered_cases as SC
from multimesh_amd import helpers, scattered
from multimesh_amd.api import GllMesh, latlondepth_to_xyz
from multimesh_amd.scattered import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rows():
    """a cloud of 200 samples, 3 fields, and the brute-force rows of 60 targets at k = 8"""
    src, fields = SC.cloud(200, seed=3)
    tgt = SC.targets(60, seed=4)
    idx, dist = SC.knn(src, tgt, 8)
    return src, fields, tgt, idx, dist


# ------------------------------------------------------------------------------------------- the statement's properties
def test_knn_rows_of_the_cases_are_sorted_and_exact(rows):
    src, _, tgt, idx, dist = rows
    assert (np.diff(dist, axis=1) >= 0).all()
    brute = np.sqrt(((tgt[:, None, :] - src[None]) ** 2).sum(axis=2))
    assert np.allclose(np.sort(brute, axis=1)[:, :8], dist, rtol=1e-14)


@pytest.mark.parametrize("power", [1, 2, 3, 8])
def test_k1_returns_the_sample_bits(rows, power):
    _, fields, _, idx, dist = rows
    out, noutside, nearest, nused = SC.idw(fields, idx[:, :1], dist[:, :1], 200, power=power)
    assert noutside == 0 and (nused == 1).all() and SC.same_bits(nearest, dist[:, 0])
    assert SC.same_bits(out, fields[:, idx[:, 0]])


def test_exact_hit_among_duplicates_takes_the_lowest_index():
    src = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    fields = np.array([[10.0, 11.0, 12.0, 13.0, 14.0]])
    idx, dist = SC.knn(src, src[[2, 3, 1]], 4)
    assert idx[:, :3].tolist() == [[1, 2, 3]] * 3 and (dist[:, :3] == 0.0).all()
    out, noutside, nearest, nused = SC.idw(fields, idx, dist, 5)
    assert noutside == 0 and out.tolist() == [[11.0, 11.0, 11.0]] and (nearest == 0.0).all() and (nused == 4).all()
    # a zero that is not the row's first valid entry (a hand-made row) is still an exact hit, the lowest such j
    out, _, nearest, _ = SC.idw(fields, [[4, 3, 2, 0]], [[0.5, 0.0, 0.0, 1.0]], 5)
    assert out.tolist() == [[13.0]] and nearest.tolist() == [0.5]
    # ... unless it is cut: an index out of range is no hit
    out, _, _, nused = SC.idw(fields, [[4, 5, 2, 0]], [[0.5, 0.0, 0.0, 1.0]], 5)
    assert out.tolist() == [[12.0]] and nused.tolist() == [3]


@pytest.mark.parametrize("power", [1, 2, 8])
def test_a_constant_field_is_reproduced_to_a_few_ulp(rows, power):
    _, _, _, idx, dist = rows
    for value in (1.0, -3.7e5, 1e-200):
        out, _, _, _ = SC.idw(np.full((1, 200), value), idx, dist, 200, power=power)
        # k products of relative error u, k - 1 sums of non-negative terms on either side, one quotient
        assert (np.abs(out - value) <= 2 * 8 * np.finfo(float).eps * abs(value)).all()


@pytest.mark.parametrize("power", [1, 2, 3, 8])
def test_weights_lie_in_the_unit_interval_on_sorted_rows(rows, power):
    _, _, _, idx, dist = rows
    valid, w, m, _, _ = SC.weights(idx, dist, 200, power, np.inf)
    assert valid.all() and (m == 8).all() and (w[:, 0] == 1.0).all()
    assert ((w >= 0.0) & (w <= 1.0)).all() and (np.diff(w, axis=1) <= 0).all()


@pytest.mark.parametrize("scale", [1e-300, 1e300])
@pytest.mark.parametrize("power", [2, 8])
def test_no_overflow_at_tiny_and_huge_distances(rows, scale, power):
    """1 / d^p would be inf at 1e-300 and 0 (an all-zero sum) at 1e+300; the relative weights do not care"""
    _, fields, _, idx, dist = rows
    scaled = dist / dist.max() * scale
    out, noutside, _, _ = SC.idw(fields, idx, scaled, 200, power=power)
    assert noutside == 0 and np.isfinite(out).all()
    ref, _, _, _ = SC.idw(fields, idx, dist, 200, power=power)
    assert np.allclose(out, ref, rtol=1e-12, atol=0)
    assert (np.abs(out) <= np.abs(fields).max() * (1 + 1e-12)).all()


def test_cuts_padding_and_outside_modes_of_the_statement(rows):
    _, fields, _, idx, dist = rows
    cut = float(np.sort(dist[:, 0])[45])                       # the 14 targets farthest from the cloud lose every neighbour
    prior = np.full((3, 60), 7.0)
    out, noutside, nearest, nused = SC.idw(fields, idx, dist, 200, max_distance=cut, outside=SC.KEEP, prior=prior)
    gone = dist[:, 0] > cut
    assert noutside == gone.sum() == 14 and np.array_equal(nused, (dist <= cut).sum(axis=1))
    assert (out[:, gone] == 7.0).all() and np.isinf(nearest[gone]).all() and SC.same_bits(nearest[~gone], dist[~gone, 0])
    filled, _, _, _ = SC.idw(fields, idx, dist, 200, max_distance=cut, fill=-1.0)
    assert (filled[:, gone] == -1.0).all() and SC.same_bits(filled[:, ~gone], out[:, ~gone])
    # the padding index nsrc and a NaN distance are not valid; a NaN field under weight 0 gives NaN, under a cut none
    f = np.array([[1.0, np.nan, 3.0]])
    assert SC.idw(f, [[0, 3, 2]], [[1.0, np.inf, 2.0]], 3)[3].tolist() == [2]
    assert SC.idw(f, [[0, 1, 2]], [[1.0, np.nan, 2.0]], 3)[0].tolist() == [[(1.0 + 0.25 * 3.0) / 1.25]]
    assert np.isnan(SC.idw(f, [[0, 1, 2]], [[1e-200, 1e200, 2e-200]], 3)[0]).all()      # (1e-400)^2 is 0.0: 0 * NaN
    assert SC.idw(f, [[0, 1, 2]], [[1.0, 5.0, 2.0]], 3, max_distance=4.0)[0].tolist() == [[(1.0 + 0.25 * 3.0) / 1.25]]


# ------------------------------------------------------------------------------------------------------- the host layer
def test_point_cloud_validation():
    pts = np.random.default_rng(0).random((10, 3))
    c = PointCloud(pts, {"VP": np.arange(10.0), "VS": np.ones(10)})
    assert len(c) == 10 and c.ndim == 3 and c.names == ["VP", "VS"] and c.fields().shape == (2, 10)
    assert c.fields("VS").shape == (1, 10) and c.fields(["VS", "VP"])[1].tolist() == list(range(10))
    c2 = PointCloud(pts, np.stack([np.arange(10.0), np.ones(10)], axis=1), ["VP", "VS"])
    assert np.array_equal(c2.fields(), c.fields()) and c2.points.flags.c_contiguous
    assert PointCloud(pts[:, :2], np.ones(10), "H").ndim == 2 and PointCloud(pts[:, 0], np.ones(10), ["H"]).ndim == 1
    for bad in (lambda: PointCloud(pts, np.ones(9), ["A"]),                   # a column of another length
                lambda: PointCloud(pts, np.ones((10, 2)), ["A"]),             # names and columns disagree
                lambda: PointCloud(pts, np.ones((10, 2)), ["A", "A"]),        # a name twice
                lambda: PointCloud(pts, np.ones(10)),                         # an array without names
                lambda: PointCloud(np.ones((10, 4)), np.ones(10), ["A"]),     # four dimensions
                lambda: PointCloud(np.ones((0, 3)), np.ones(0), ["A"]),       # no points
                lambda: PointCloud(pts, {"A": np.ones((10, 1))}),             # a column that is not 1-D
                lambda: PointCloud(pts[:, :2], np.ones(10), ["A"], geocentric=True),
                lambda: c.fields("RHO"),
                lambda: c.pick(["VP", "Q"])):
        with pytest.raises(ValueError):
            bad()


def test_geocentric_points_go_through_latlondepth_to_xyz():
    lld = np.array([[10.0, 20.0, 0.0], [-45.0, 170.0, 30000.0], [89.0, -120.0, 6371000.0 / 2]])
    c = PointCloud(lld, {"H": np.ones(3)}, geocentric=True)
    assert SC.same_bits(c.points, latlondepth_to_xyz(lld))
    assert SC.same_bits(PointCloud(lld, {"H": np.ones(3)}).points, lld)


def test_chunk_planner():
    assert scattered.chunk_size(1000, 8) == 1000                                    # everything fits
    assert scattered.chunk_size(10 ** 9, 8, 1 << 30) == (1 << 30) // 128
    assert scattered.chunk_size(10 ** 9, 20, 1 << 30) * 16 * 20 <= 1 << 30 < (scattered.chunk_size(10 ** 9, 20, 1 << 30) + 1) * 320
    assert scattered.chunk_size(5, 64, 100) == 1 and scattered.chunk_size(0, 8) == 1   # at least one target per chunk
    assert scattered.SCRATCH_BYTES == 1 << 30
    with pytest.raises(ValueError):
        scattered.chunk_size(10, 0)


def _no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device was asked for before the arguments were checked")
    monkeypatch.setattr(scattered, "default_context", refuse)
    monkeypatch.setattr(PointCloud, "index", refuse)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    _no_device(monkeypatch)
    pts, fields = SC.cloud(20, seed=1)
    c = PointCloud(pts, {"A": fields[0], "B": fields[1]})
    tgt = SC.targets(5)
    mesh = GllMesh(np.zeros((2, 27, 3)), 2, {"A": np.zeros((2, 27))})
    for kwargs in (dict(k=0), dict(k=65), dict(k=2.0), dict(k=True), dict(power=0), dict(power=9), dict(power=2.0),
                   dict(max_distance=-1.0), dict(max_distance=np.nan), dict(outside="clamp"), dict(outside="keep"),
                   dict(params="C"), dict(params=["A", "C"]), dict(chunk_points=0)):
        with pytest.raises(ValueError):
            scattered.interpolate_scattered(c, tgt, **kwargs)
    with pytest.raises(ValueError):
        scattered.interpolate_scattered(c, tgt[:, :2])                              # 2-D targets of a 3-D cloud
    with pytest.raises(ValueError):
        scattered.interpolate_scattered((pts, fields), tgt)                         # not a PointCloud
    for kwargs in (dict(k=0), dict(power=9), dict(max_distance=-1.0), dict(outside="clamp"), dict(params="C"),
                   dict(blend=(2.0, 1.0)), dict(blend=(-1.0, 1.0)), dict(blend=(0.0, np.inf)),
                   dict(params=["A", "B"]),                                         # keep, and the mesh has no B
                   dict(params="B", outside="fill", blend=(0.0, 1.0))):             # blend needs the mesh's B too
        with pytest.raises(ValueError):
            scattered.import_point_cloud(c, mesh, **{"params": "A", **kwargs})
    with pytest.raises(ValueError):
        scattered.import_point_cloud(PointCloud(pts[:, :2], {"A": fields[0]}), mesh)   # a 2-D cloud onto a 3-D mesh


def test_the_binding_layer_knows_the_symbol():
    name = "mm_idw_gather"
    restype, argtypes = helpers.SIGNATURES[name]
    assert restype is C.c_int64 and len(argtypes) == 16 and name in helpers.EXPORTED_SYMBOLS
    order = list(helpers.EXPORTED_SYMBOLS)
    assert order.index("mm_arg_extreme") + 1 == order.index(name)
    header = open(os.path.join(ROOT, "include", "multimesh_hip.h")).read()
    assert re.search(r"\bint64_t %s\s*\(" % name, header)
    lib = helpers.load_lib()
    assert hasattr(lib, name) and lib.mm_idw_gather.restype is C.c_int64
    from multimesh_amd.device import Context
    assert Context.idw_gather.__doc__ and set(scattered.__all__) == {"PointCloud", "chunk_size", "interpolate_scattered",
                                                                     "import_point_cloud"}


def test_null_context_is_refused_without_a_gpu():
    lib = helpers.load_lib()
    buf = np.zeros(8)
    p = buf.ctypes.data
    assert lib.mm_idw_gather(None, p, 1, 1, p, p, 1, 1, 2, np.inf, 0, 0.0, p, 0, None, None) == -1
    assert b"ctx is null" in lib.mm_last_error()
