"""The integer counts and the chunked sums of the model tools at the sizes where a wave sum, a block boundary or the
grid-stride loop can go wrong.  Every count a call returns (or carries in the text of its refusal), and the one output array
it comes with, against the NumPy statements of tests/*_cases.py -- or a one-line expression where there is none.

SMALL brackets a wave (64 lanes) and a workgroup (256).  A launch with at most `cap` workgroups strides from
cap * 256 + 1 items on: STRIDE_2048 for the calls that launch at most 2048 workgroups, STRIDE_8192 for mm_first_occurrence's
8192, and 2048 tiles of 32 order-1 elements plus one element for mm_gll_mass.

The sums at three levels (more than 4096 * 4096 values) are asserted bit for bit by
test_mass_gpu.py::test_weighted_sum_bit_for_bit[16777221] and test_radial_gpu.py::test_binned_sum_three_levels; they are not
repeated here."""

import numpy as np
import pytest

import grid_import_cases as G
import mass_cases as M
import precondition_cases as PC
import radial_cases as RC
from multimesh_amd import api, helpers, synth
from multimesh_amd.device import Context

pytestmark = pytest.mark.gpu

SMALL = [1, 63, 64, 65, 255, 256, 257]
STRIDE_2048 = 2048 * 256 + 1
STRIDE_8192 = 8192 * 256 + 1
CHUNK_SIZES = [4095, 4096, 4097]


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


# ------------------------------------------------------------------------------------------------------ mm_radial_bins
@pytest.mark.parametrize("n", SMALL + [STRIDE_2048])
def test_radial_bins_outside_count(ctx, n):
    edges = np.linspace(3.0e6, 6.4e6, 8)
    pts = np.zeros((n, 3))
    pts[:, 0] = np.random.default_rng(n).uniform(edges[0], edges[-1], n)
    pts[::5, 0] = 7.0e6                          # every 5th point outside: every wave carries a count of its own
    ref, ref_out, _ = RC.bins(pts, edges)
    b, nout = ctx.radial_bins(pts, edges)
    assert ref_out == (n + 4) // 5 and nout == ref_out
    assert np.array_equal(b.numpy(), ref)


# ------------------------------------------------------------------------------------------------------------ mm_clamp
@pytest.mark.parametrize("n", SMALL + [STRIDE_2048])
def test_clamp_changed_count_per_component(ctx, n):
    v = np.random.default_rng(n).normal(size=(2, n))
    lower, upper = [-0.5, -2.0], [1.0, 1.5]
    ref, ref_changed = PC.clamp(v, lower, upper)
    out, changed = ctx.clamp(v, lower=lower, upper=upper)
    assert np.array_equal(changed.numpy(), ref_changed)
    assert n < 64 or (ref_changed[0] != ref_changed[1] and ref_changed.min() > 0)
    assert M.same_bits(out.numpy(), ref)


# ------------------------------------------------------------------------------------------------------ mm_point_taper
def _cloud(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))


@pytest.mark.parametrize("n", SMALL + [STRIDE_2048])
def test_point_taper_count_of_one_centre(ctx, n):
    pts = _cloud(n, n)
    centre, inner, outer = [[0.1, -0.2, 0.3]], [0.3], [0.9]
    ref_w, ref_count = PC.taper_weight(pts, centre, inner, outer)
    _, count, w = ctx.point_taper(pts, centre, inner, outer, want_weight=True)
    assert count == ref_count and (n < 64 or 0 < ref_count < n)
    assert M.same_bits(w.numpy(), ref_w)


@pytest.mark.parametrize("groups", [1, 9, 10, 19])             # 9 elements of 27 nodes are a tile
def test_point_taper_count_on_whole_elements(ctx, groups):
    pts = _cloud(groups * 27, groups).reshape(groups, 27, 3)
    centre, inner, outer = [[0.1, -0.2, 0.3]], [0.3], [0.9]
    ref_w, ref_count = PC.taper_weight(pts, centre, inner, outer)
    _, count, w = ctx.point_taper(pts, centre, inner, outer, want_weight=True)
    assert count == ref_count
    assert M.same_bits(w.numpy().reshape(-1), ref_w)


def test_point_taper_refusal_carries_the_count(ctx):
    centres = np.array([[0.0, 0.0, 0.0], [0.5, np.nan, 0.0], [0.2, 0.2, 0.2]])
    with pytest.raises(ValueError, match="mm_point_taper: 1 centres are not finite"):
        ctx.point_taper(_cloud(300, 0), centres, [0.1] * 3, [0.5] * 3, want_weight=True)


# --------------------------------------------------------------------------------------------------------- mm_gll_mass
@pytest.fixture(scope="module")
def order1_mesh():
    """65 537 order-1 3-D elements (2048 tiles of 32 and one more), every 7th mirrored in x about its centroid"""
    gp = np.ascontiguousarray(synth.gll_mesh(42, 1, seed=5)[:2048 * 32 + 1])
    gp[::7, :, 0] = 2.0 * gp[::7, :, 0].mean(axis=1, keepdims=True) - gp[::7, :, 0]
    return gp


@pytest.mark.parametrize("nelem", [1, 2, 31, 32, 33, 65, 2048 * 32 + 1])
def test_gll_mass_bad_jacobian_count(ctx, order1_mesh, nelem):
    gp = order1_mesh[:nelem]
    _, w, D = api.gll_quadrature(1)
    ref_mass, ref_det = M.mass(gp, 1, w, D)
    mass, n_bad = ctx.gll_mass(1, gp)
    assert n_bad == M.n_bad(ref_det) == 8 * ((nelem + 6) // 7)          # all eight nodes of every 7th element
    assert M.same_bits(mass.numpy(), ref_mass)


# ------------------------------------------------------------------------------------------------- mm_first_occurrence
@pytest.mark.parametrize("n", SMALL + [STRIDE_8192])
def test_first_occurrence_unreferenced_count(ctx, n):
    conn = np.random.default_rng(n).integers(0, n, n)                   # n entries over n nodes: about a third is not named
    ref = np.full(n, -1, dtype=np.int64)
    nodes, index = np.unique(conn, return_index=True)
    ref[nodes] = index
    conn_d, first_d = ctx.to_device(conn), ctx.empty((n,), np.int64)
    rc = ctx.lib.mm_first_occurrence(ctx.handle, conn_d.ptr, n, n, first_d.ptr)
    assert rc == n - len(nodes) and (n < 64 or rc > 0)
    assert np.array_equal(first_d.numpy(), ref)


@pytest.mark.parametrize("n", [257, STRIDE_8192])
def test_first_occurrence_refusal_carries_the_count(ctx, n):
    conn = np.random.default_rng(n).integers(0, n, n)
    conn[::100] = n + 5
    conn[50::100] = -1
    nbad = len(conn[::100]) + len(conn[50::100])
    with pytest.raises(ValueError, match=rf"mm_first_occurrence: {nbad} connectivity entries outside \[0, {n}\)"):
        ctx.first_occurrence(conn, n)


# ------------------------------------------------------------------------------------------------------ mm_sample_grid
@pytest.mark.parametrize("n", SMALL + [STRIDE_2048])
def test_sample_grid_outside_count(ctx, n):
    rng = np.random.default_rng(n)
    lat, lon = np.radians(rng.uniform(-9.0, 9.0, n)), np.radians(rng.uniform(-8.0, 9.0, n))
    r = G.R_EARTH - rng.uniform(-2.0e4, 3.5e5, n)
    pts = np.stack([r * np.cos(lat) * np.cos(lon), r * np.cos(lat) * np.sin(lon), r * np.sin(lat)], axis=1)
    grid = G.grid_values(1)
    out, nmissing, lld = ctx.sample_grid(pts, grid, G.DEPTH, G.LAT, G.LON, want_latlondepth=True)
    lld = lld.numpy()
    want, ref_missing, inside = G.sample(grid, G.DEPTH, G.LAT, G.LON, lld[:, 2], lld[:, 0], lld[:, 1])
    assert nmissing == ref_missing == int((~inside).sum()) and (n < 64 or 0 < nmissing < n)
    assert G.same_bits(out.numpy(), want)


# ------------------------------------------------------------------------------------------- mm_transpose_create_nodes
def test_transpose_nodes_refusal_carries_the_count(ctx):
    nsrc = 50
    ids = np.random.default_rng(1).integers(0, nsrc, (75, 4))           # 300 entries: five waves
    w = np.ones(ids.shape)
    ctx.transpose_nodes(ids, w, nsrc).free()
    for flat, bad in ((5, nsrc), (70, -1), (200, nsrc + 7)):            # three bad ids in three different waves
        ids.reshape(-1)[flat] = bad
    with pytest.raises(helpers.MultiMeshHipError, match=rf"mm_transpose_create_nodes: 3 ids outside \[0, {nsrc}\)"):
        ctx.transpose_nodes(ids, w, nsrc)


# -------------------------------------------------------------------------------------------------- mm_fluid_solid_fix
@pytest.mark.parametrize("nelem", [1, 63, 64, 65, 257])
def test_fluid_solid_fix_restored_count(ctx, nelem):
    rng = np.random.default_rng(nelem)
    values, previous = rng.uniform(1.0, 2.0, (nelem, 3, 27)), rng.uniform(5.0, 6.0, (nelem, 3, 27))
    solid = np.arange(nelem) % 4 != 1
    values[::3, 1, rng.integers(0, 27)] = 0.0                           # a zero shear velocity in every 3rd element
    zero_vs = (values[:, 1, :] == 0.0).any(axis=1)
    want = np.where((~solid | zero_vs)[:, None, None], previous, values)
    fixed = ctx.to_device(values)
    assert ctx.fluid_solid_fix(fixed, previous, solid, 1) == int((solid & zero_vs).sum())
    assert np.array_equal(fixed.numpy(), want)


# ---------------------------------------------------------------------------------------------------- the chunked sums
@pytest.mark.parametrize("n", CHUNK_SIZES)
def test_weighted_sum_around_a_chunk(ctx, n):
    rng = np.random.default_rng(n)
    mass, f = rng.uniform(0.5, 1.5, n), rng.normal(size=(2, n))
    f[:, 0] = -0.0                                                      # the sum starts from its first term
    assert M.same_bits(ctx.weighted_sum(mass, f), M.weighted_sum(mass, f))
    assert M.same_bits(ctx.weighted_sum(mass), M.weighted_sum(mass))


@pytest.mark.parametrize("n", CHUNK_SIZES + [4096 * 2 + 1])             # 8193: a level of binned_level_kernel on top
def test_binned_weighted_sum_around_a_chunk(ctx, n):
    rng = np.random.default_rng(n)
    mass, f = rng.uniform(0.5, 2.0, n), rng.normal(size=(2, n))
    bins = rng.integers(-1, 3, n).astype(np.int32)                      # -1: in no bin
    ref = RC.binned_weighted_sum(mass, f, bins, 3)
    out, count = ctx.binned_weighted_sum(mass, bins, 3, f, want_count=True)
    assert RC.same_bits_nan(out, ref)
    assert np.array_equal(count, RC.bin_counts(bins, 3))
