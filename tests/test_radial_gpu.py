"""mm_radial_bins, mm_binned_weighted_sum and mm_radial_model_apply on the GPU, BIT for bit against their NumPy statements
(tests/radial_cases.py) unless a bound is derived where it is asserted.  NaN results are compared by position
(radial_cases.same_bits_nan): the payload of a NaN is not part of the statement.

WINDOW is the kernel's window of bins (kWindow of multimesh_amd/csrc/mm_radial.hip), TILE the elements a 256-thread block
of the table evaluation takes (256 // P)."""

import numpy as np
import pytest

import mass_cases as M
import radial_cases as RC
from multimesh_amd import api, synth
from multimesh_amd.api import GllMesh, RadialModel
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

EPS = M.EPS
MM_ERR_ARG = -1
WINDOW = 8
SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097]
TWO_LEVELS = 4096 * 5 + 17
RADII3 = (5_771_000.0, 5_971_000.0, 6_171_000.0, synth.R_EARTH)


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


# ------------------------------------------------------------------------------------------------------ mm_radial_bins
def _bin_points(n, edges, seed):
    """n points with radii from below edges[0] to above edges[-1]; when there is room, rows exactly on edges[0], on an
    inner edge (where there is one) and on edges[-1], one below, one above and a NaN row."""
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 3))
    span = edges[-1] - edges[0]
    pts *= (rng.uniform(edges[0] - 0.1 * span, edges[-1] + 0.1 * span, n) / np.linalg.norm(pts, axis=1))[:, None]
    special = [edges[0], edges[len(edges) // 2], edges[-1], edges[0] * 0.5, edges[-1] * 2.0, np.nan]
    for k, v in enumerate(special[:n]):
        pts[k] = 0.0
        pts[k, k % 3] = v                       # sqrt(v * v) is v exactly: the point lies ON the edge
    return pts


@pytest.mark.parametrize("nbins", [1, 7, 3000])            # 3000: 3001 edges do not fit the 2048 doubles of the LDS path
def test_bins_bit_for_bit(ctx, nbins):
    edges = np.linspace(3.0e6, 6.4e6, nbins + 1)
    for n in SIZES + [3 * 4096 + 5]:
        pts = _bin_points(n, edges, n + nbins)
        ref, ref_out, ref_r = RC.bins(pts, edges)
        b, nout, r = ctx.radial_bins(pts, edges, want_radius=True)
        assert b.shape == (n,) and b.dtype == np.int32
        assert np.array_equal(b.numpy(), ref), (nbins, n)
        assert nout == ref_out, (nbins, n)
        assert RC.same_bits_nan(r.numpy(), ref_r), (nbins, n)
        if n >= 6:
            assert b.numpy()[0] == 0 and b.numpy()[2] == nbins - 1 and (b.numpy()[3:6] == -1).all()
        b2, nout2 = ctx.radial_bins(pts, edges)
        assert np.array_equal(b2.numpy(), ref) and nout2 == ref_out


@pytest.mark.parametrize("edges", [[1.0, 2.0, 2.0, 3.0], [1.0, 3.0, 2.0, 4.0], [1.0, 2.0, np.nan, 4.0], [1.0, 2.0, 3.0, np.inf]])
def test_bins_refuse_edges_that_do_not_ascend(ctx, edges):
    pts = np.random.default_rng(0).uniform(0.5, 2.0, (300, 3))
    with pytest.raises(ValueError):
        ctx.radial_bins(pts, edges)
    pts_d, edges_d = ctx.to_device(pts), ctx.to_device(np.asarray(edges))
    bins_d = ctx.to_device(np.full(300, 77, dtype=np.int32))
    rad_d = ctx.to_device(np.full(300, -5.0))
    rc = ctx.lib.mm_radial_bins(ctx.handle, pts_d.ptr, 300, edges_d.ptr, 3, bins_d.ptr, rad_d.ptr)
    assert rc == MM_ERR_ARG
    assert (bins_d.numpy() == 77).all() and (rad_d.numpy() == -5.0).all()          # nothing is written
    assert ctx.lib.mm_radial_bins(ctx.handle, pts_d.ptr, 300, edges_d.ptr, 0, bins_d.ptr, None) == MM_ERR_ARG


# ---------------------------------------------------------------------------------------------- mm_binned_weighted_sum
def _shuffled(n, nbins, ncomp, seed):
    """A cloud in no order: every chunk spans every bin and a lane comes back to a bin it left; some entries in no bin."""
    rng = np.random.default_rng(seed)
    mass = rng.uniform(0.5, 2.0, n)
    fields = rng.normal(size=(ncomp, n))
    bins = rng.integers(0, nbins, n).astype(np.int32)
    if n > 10:
        bins[rng.integers(0, n, max(n // 50, 2))] = -1
        bins[rng.integers(0, n, 2)] = nbins
        bins[rng.integers(0, n, 2)] = -7
    return mass, fields, bins


def _check_sum(ctx, mass, fields, bins, nbins, square=False, what=""):
    ref = RC.binned_weighted_sum(mass, fields, bins, nbins, square)
    out, count = ctx.binned_weighted_sum(mass, bins, nbins, fields, square=square, want_count=True)
    assert out.shape == ref.shape, what
    assert RC.same_bits_nan(out, ref), (what, np.argwhere(out != ref)[:5])
    assert not np.signbit(out[~np.isnan(out) & (out == 0.0)]).any(), what          # no -0.0
    assert np.array_equal(count, RC.bin_counts(bins, nbins)), what
    out2 = ctx.binned_weighted_sum(mass, bins, nbins, fields, square=square)       # without the counts, and once more
    assert RC.same_bits_nan(out2, out), what
    return out


@pytest.mark.parametrize("n", SIZES + [TWO_LEVELS])
def test_binned_sum_sizes(ctx, n):
    mass, fields, bins = _shuffled(n, 3, 1, n)
    _check_sum(ctx, mass, fields, bins, 3, what=n)
    _check_sum(ctx, mass, None, bins, 3, what=(n, "volume"))


@pytest.mark.parametrize("nbins", [1, 2, WINDOW, WINDOW + 1, 300])
@pytest.mark.parametrize("ncomp", [1, 3, 5])
def test_binned_sum_on_a_shuffled_cloud(ctx, nbins, ncomp):
    n = 2 * 4096 + 100 if nbins == 300 or ncomp == 5 else TWO_LEVELS
    mass, fields, bins = _shuffled(n, nbins, ncomp, nbins * 10 + ncomp)
    out = _check_sum(ctx, mass, fields, bins, nbins, what=(nbins, ncomp))
    _check_sum(ctx, mass, fields, bins, nbins, square=True, what=(nbins, ncomp, "square"))
    # sum over the bins against the plain weighted sum of the members: other orders of the same terms
    inside = (bins >= 0) & (bins < nbins)
    total = ctx.weighted_sum(np.where(inside, mass, 0.0), fields)
    for c in range(ncomp):
        assert abs(out[c].sum() - total[c]) <= 2 * M.term_bound(mass[inside] * fields[c][inside]) \
            + nbins * EPS * np.abs(out[c]).sum()


def test_binned_sum_three_levels(ctx):
    n = 4096 * 4096 + 1
    rng = np.random.default_rng(9)
    mass = rng.uniform(0.5, 2.0, n)
    field = rng.normal(size=(1, n))
    bins = (rng.random(n) < 0.3).astype(np.int32)
    bins[-1] = 1                                  # the value that opens the last chunk of the first level
    _check_sum(ctx, mass, field, bins, 2, what="three levels")


@pytest.mark.parametrize("nbins_per_element", [None, 0.5, 3.0])
def test_binned_sum_on_an_earth_chunk(ctx, nbins_per_element):
    """Bins equal to the layers, bins wider and bins thinner than an element (200 km / 2 = 100 km radial elements)."""
    ch = synth.earth_chunk(order=4, nlat=5, nlon=5, radii=RADII3, nrad=(2, 2, 2))
    pts = ch["points"]
    if nbins_per_element is None:
        edges = np.array(RADII3)
        edges[-1] += 10.0                          # (the surface nodes round to either side of R_EARTH)
    else:
        edges = np.linspace(RADII3[0] - 10.0, RADII3[-1] + 10.0, int(6 * nbins_per_element) + 1)
    mass, n_bad = ctx.gll_mass(4, pts)
    assert n_bad == 0
    bins, nout = ctx.radial_bins(pts, edges)
    ref_bins, ref_out, _ = RC.bins(pts, edges)
    assert np.array_equal(bins.numpy(), ref_bins) and nout == ref_out
    r = RC.radius(pts)
    fields = np.stack([r / 6.0e6, np.sin(r / 1.0e5), np.ones_like(r)]).reshape(3, *pts.shape[:2])
    _check_sum(ctx, mass.numpy(), fields, ref_bins, len(edges) - 1, what=nbins_per_element)
    out = ctx.binned_weighted_sum(mass, bins, len(edges) - 1, fields)              # device arrays in
    assert RC.same_bits_nan(out, RC.binned_weighted_sum(mass.numpy(), fields, ref_bins, len(edges) - 1))


def test_binned_sum_special_values(ctx):
    n, nbins = 4096 + 300, 12
    rng = np.random.default_rng(4)
    mass = rng.uniform(0.5, 2.0, n)
    field = rng.normal(size=(1, n))
    one = np.full(n, 5, dtype=np.int32)
    out = _check_sum(ctx, mass, field, one, nbins, what="one bin")
    assert (np.delete(out[0], 5).view(np.uint64) == 0).all()                       # empty bins: +0.0, sign bit clear
    none = np.full(n, -1, dtype=np.int32)
    out = _check_sum(ctx, mass, field, none, nbins, what="no bin")
    assert (out.view(np.uint64) == 0).all()
    # a NaN and an inf in bin 3 leave the other bins finite, whatever chunk and lane they sit in
    bins = rng.integers(0, nbins, n).astype(np.int32)
    bad = field.copy()
    k = np.nonzero(bins == 3)[0]
    bad[0, k[0]] = np.nan
    bad[0, k[-1]] = np.inf
    out = _check_sum(ctx, mass, bad, bins, nbins, what="nan")
    assert np.isnan(out[0, 3]) and np.isfinite(np.delete(out[0], 3)).all()
    out = _check_sum(ctx, mass, bad, bins, nbins, square=True, what="nan square")
    assert np.isnan(out[0, 3]) and np.isfinite(np.delete(out[0], 3)).all()
    # a field of -0.0: every product is -0.0, every sum starts from +0.0
    out = _check_sum(ctx, mass, np.full((1, n), -0.0), bins, nbins, what="-0.0")
    assert (out.view(np.uint64) == 0).all()


def test_binned_sum_argument_errors(ctx):
    m = ctx.to_device(np.ones(10))
    b = ctx.to_device(np.zeros(10, dtype=np.int32))
    out = ctx.to_device(np.full(4, 7.0))
    lib = ctx.lib
    assert lib.mm_binned_weighted_sum(ctx.handle, m.ptr, None, b.ptr, 10, 2, 2, 0, out.ptr, None) == MM_ERR_ARG
    assert lib.mm_binned_weighted_sum(ctx.handle, m.ptr, None, b.ptr, 10, 1, 0, 0, out.ptr, None) == MM_ERR_ARG
    assert lib.mm_binned_weighted_sum(ctx.handle, m.ptr, None, b.ptr, -1, 1, 2, 0, out.ptr, None) == MM_ERR_ARG
    assert lib.mm_binned_weighted_sum(None, m.ptr, None, b.ptr, 10, 1, 2, 0, out.ptr, None) == MM_ERR_ARG
    assert (out.numpy() == 7.0).all()
    assert lib.mm_binned_weighted_sum(ctx.handle, None, None, None, 0, 1, 4, 0, out.ptr, None) == 0     # n == 0: zeros
    assert (out.numpy().view(np.uint64) == 0).all()


# ---------------------------------------------------------------------------------------------- mm_radial_model_apply
def _table3():
    """Three layers with discontinuities on earth_chunk's two inner interfaces; a smooth row and a row that is constant
    per layer (1, 2, 3)."""
    R = np.array([5.7e6, RADII3[1], RADII3[1], 6_071_000.0, RADII3[2], RADII3[2], 6.4e6])
    V = np.array([[3.1, 3.4, 4.0, 4.2, 4.3, 4.9, 5.0], [1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 3.0]])
    return R, V


def _check_apply(ctx, pts, R, V, what=""):
    rng = np.random.default_rng(11)
    V = np.atleast_2d(V)
    n = pts.shape[0] * (pts.shape[1] if pts.ndim == 3 else 1)
    vin = rng.uniform(3.0, 5.0, (V.shape[0], n))
    ref0 = RC.model_apply(pts, R, V)
    for mode in range(5):
        ref = RC.model_apply(pts, R, V, mode, vin)
        out = ctx.radial_model_apply(pts, R, V, mode=mode, values_in=None if mode == 0 else vin)
        assert out.shape == (V.shape[0],) + pts.shape[:-1], what
        assert RC.same_bits_nan(out.numpy().reshape(ref.shape), ref), (what, mode)
        if mode:                                                                  # in place
            buf = ctx.to_device(vin)
            same = ctx.radial_model_apply(pts, R, V, mode=mode, values_in=buf, out=buf)
            assert same is buf and RC.same_bits_nan(buf.numpy(), ref), (what, mode, "in place")
    return ref0


@pytest.mark.parametrize("order", [1, 2, 4])
@pytest.mark.parametrize("ellipticity", [0.0, 3e-3])
def test_apply_on_earth_chunks_around_a_tile(ctx, order, ellipticity):
    ch = synth.earth_chunk(order=order, nlat=5, nlon=5, radii=RADII3, nrad=(2, 2, 2), ellipticity=ellipticity)
    pts, layer = ch["points"], ch["layer"]
    R, V = _table3()
    tile = 256 // pts.shape[1]
    for nelem in (1, tile - 1, tile, tile + 1, 3 * tile + max(tile // 2, 1), len(pts)):
        if 1 <= nelem <= len(pts):
            _check_apply(ctx, np.ascontiguousarray(pts[:nelem]), R, V, (order, ellipticity, nelem))
    # every node, the ones on the interfaces included, takes the side of its own element -- also on the deformed mesh,
    # whose nodes no longer sit on the table's radii
    out = ctx.radial_model_apply(pts, R, V).numpy()
    # (the lerp of a constant is the constant within 1 - t's rounding, the two products' and the sum's: 4u of it)
    assert (np.abs(out[1] - layer[:, None]) <= 4 * 2.0 ** -53 * layer[:, None]).all()
    r = RC.radius(pts).reshape(pts.shape[:2])
    for k, radius in ((1, RADII3[1]), (2, RADII3[2])):
        on = ch["z_node_1D"] == radius / synth.R_EARTH
        assert on[layer == k].any() and on[layer == k + 1].any()
        if ellipticity:
            assert np.abs(r[on] - radius).max() > 1000.0


def test_apply_on_points(ctx):
    """P = 1: counts around a tile of 256 points, points on a discontinuity (the upper side), below, above, NaN."""
    R, V = _table3()
    rng = np.random.default_rng(5)
    for n in (1, 255, 256, 257, 256 * 3 + 128):
        pts = rng.normal(size=(n, 3))
        pts *= (rng.uniform(5.6e6, 6.5e6, n) / np.linalg.norm(pts, axis=1))[:, None]
        special = [RADII3[1], RADII3[2], 1.0e6, 7.0e6, np.nan, R[0], R[-1]]
        for k, v in enumerate(special[:n]):
            pts[k] = 0.0
            pts[k, k % 3] = v
        ref = _check_apply(ctx, pts, R, V, ("points", n))
        if n >= 7:
            assert ref[1][:4].tolist() == [2.0, 3.0, 1.0, 3.0] and np.isnan(ref[:, 4]).all()
            assert ref[0][2] == V[0][0] and ref[0][3] == V[0][-1]


def test_apply_centres_beyond_the_table_and_a_nan_node(ctx):
    ch = synth.earth_chunk(order=2, nlat=3, nlon=3, radii=RADII3, nrad=(2, 2, 2))
    pts = ch["points"].copy()
    R = np.array([5.9e6, 6.0e6, 6.0e6, 6.1e6])                # the mesh reaches 130 km below and 270 km above the table
    V = np.array([[1.0, 2.0, 5.0, 7.0]])
    pts[20, 13, 1] = np.nan                                    # one NaN node: its element's centre is NaN
    ref = _check_apply(ctx, pts, R, V, "beyond").reshape(pts.shape[:2])
    assert np.isnan(ref[20]).all() and not np.isnan(np.delete(ref, 20, axis=0)).any()
    assert (ref[ch["layer"] == 1][:9] == 1.0).all() and (ref[ch["layer"] == 3][-9:] == 7.0).all()


def test_apply_small_and_large_tables(ctx):
    ch = synth.earth_chunk(order=4, nlat=3, nlon=3, radii=RADII3, nrad=(2, 2, 2))
    pts = ch["points"]
    _check_apply(ctx, pts, np.array([5.8e6, 6.3e6]), np.array([[1.0, 9.0], [4.0, -2.0]]), "two rows")
    # 3000 rows x (1 + 1) columns = 6000 doubles: more than the 4096 of the LDS path; discontinuities every 500 rows
    R = np.linspace(5.7e6, 6.4e6, 3000)
    R[500::500] = R[499:-1:500]
    V = np.cos(np.arange(3000.0))[None, :] + 3.0
    assert len(RC.layers(R)) == 6
    _check_apply(ctx, pts, R, V, "large")
    # and five components on a table that fits
    R5, V5 = _table3()
    _check_apply(ctx, pts[:7], R5, np.vstack([V5, V5[::-1], V5[:1] * 2.0]), "five components")


def test_apply_refuses_bad_tables_and_arguments(ctx):
    pts = synth.earth_chunk(order=1)["points"]
    for R in ([1.0, 2.0, 2.0, 2.0, 3.0], [1.0, 1.0, 2.0], [1.0, 2.0, 2.0], [1.0, 2.0, 1.5], [1.0, np.inf], [1.0, np.nan, 3.0]):
        with pytest.raises(ValueError):
            ctx.radial_model_apply(pts, R, np.zeros((1, len(R))))
    R = ctx.to_device(np.array([3.0, 2.0, 1.0]))
    V = ctx.to_device(np.zeros(3))
    p = ctx.to_device(pts)
    out = ctx.to_device(np.full(pts.shape[0] * 8, 7.0))
    lib = ctx.lib
    assert lib.mm_radial_model_apply(ctx.handle, p.ptr, pts.shape[0], 8, R.ptr, V.ptr, 3, 1, 0, None, out.ptr) == MM_ERR_ARG
    Rok = ctx.to_device(np.array([1.0, 2.0, 3.0]))
    assert lib.mm_radial_model_apply(ctx.handle, p.ptr, pts.shape[0], 8, Rok.ptr, V.ptr, 3, 1, 5, None, out.ptr) == MM_ERR_ARG
    assert lib.mm_radial_model_apply(ctx.handle, p.ptr, pts.shape[0], 8, Rok.ptr, V.ptr, 3, 1, 2, None, out.ptr) == MM_ERR_ARG
    assert lib.mm_radial_model_apply(ctx.handle, p.ptr, pts.shape[0], 300, Rok.ptr, V.ptr, 3, 1, 0, None, out.ptr) == MM_ERR_ARG
    assert (out.numpy() == 7.0).all()


def test_mode_4_after_mode_2_returns_the_input(ctx):
    """p = fl(fl(v - ref) / ref), back = fl(ref + fl(p * ref)): the three roundings on the way to p * ref leave
    (v - ref)(1 + d), |d| <= 3u + O(u^2), and the last addition one more relative u on the result, so
    |back - v| <= u (3 |v - ref| + |v|) (1 + 2^-50), u = 2^-53."""
    ch = synth.earth_chunk(order=4, nlat=3, nlon=3, radii=RADII3, nrad=(2, 2, 2))
    pts = ch["points"]
    R, V = _table3()
    ref = RC.model_apply(pts, R, V)
    v = ref * np.random.default_rng(3).uniform(0.9, 1.1, ref.shape)
    pert = ctx.radial_model_apply(pts, R, V, mode=2, values_in=v)
    back = ctx.radial_model_apply(pts, R, V, mode=4, values_in=pert).numpy().reshape(ref.shape)
    bound = 2.0 ** -53 * (3 * np.abs(v - ref) + np.abs(v)) * (1 + 2.0 ** -50)
    assert (np.abs(back - v) <= bound).all()
    assert np.abs(pert.numpy()).max() < 0.11


# ------------------------------------------------------------------------------------------------------------- the API
@pytest.fixture(scope="module")
def chunk_mesh():
    ch = synth.earth_chunk(order=4, nlat=4, nlon=4, radii=RADII3, nrad=(2, 2, 2))
    return ch


def test_radial_profile_of_a_function_of_the_radius(ctx, chunk_mesh):
    """f = g(r), constant in every bin: mean = S1 / S0 with S1 = sum m g and S0 = sum m over the n nodes of the bin.  Each
    sum of n terms is within n 2^-52 of exact in relative terms (positive terms; mass_cases.term_bound), the products add
    2^-53, the quotient 2^-53: |mean - g| <= (2 n + 2) 2^-52 |g|; the rms has one more product and a square root (which
    halves the error of its argument and rounds once): the same bound with + 4."""
    pts = chunk_mesh["points"]
    edges = np.array(RADII3)
    edges[0] -= 10.0
    edges[-1] += 10.0
    consts = np.array([-3.25, 4.5, 0.1])
    ref_bins, _, _ = RC.bins(pts, edges)
    f = consts[ref_bins].reshape(pts.shape[:2])
    mesh = GllMesh(pts, 4, {"F": f, "ONE": np.ones_like(f)})
    prof = api.radial_profile(mesh, ["F", "ONE"], edges=edges, context=ctx)
    assert prof.noutside == 0 and np.array_equal(prof.count, np.bincount(ref_bins, minlength=3))
    assert np.array_equal(prof.centres, 0.5 * (edges[:-1] + edges[1:]))
    bound = (2 * prof.count + 4) * EPS * np.abs(consts)
    assert (np.abs(prof.mean["F"] - consts) <= bound).all()
    assert (np.abs(prof.rms["F"] - np.abs(consts)) <= bound).all()
    assert (np.abs(prof.mean["ONE"] - 1.0) <= (2 * prof.count + 4) * EPS).all()
    # the volume per bin sums to the mesh's volume: both are sums of the same n masses in some order
    mass = api.gll_mass_matrix(mesh, context=ctx)
    volume = api.integrate(mesh, context=ctx)
    assert abs(prof.volume.sum() - volume) <= 2 * M.term_bound(mass) + 3 * EPS * volume
    assert M.same_bits(prof.volume, RC.binned_weighted_sum(mass, None, ref_bins, 3)[0])
    # an empty bin: NaN mean and rms, zero volume
    wide = api.radial_profile(mesh, ["F"], edges=[1.0e6, 2.0e6, edges[0], edges[-1]], context=ctx)
    assert np.isnan(wide.mean["F"][:2]).all() and np.isnan(wide.rms["F"][:2]).all() and (wide.volume[:2] == 0).all()
    assert wide.count.tolist() == [0, 0, ref_bins.size]
    # default edges cover the mesh
    auto = api.radial_profile(mesh, nbins=9, context=ctx)
    assert auto.noutside == 0 and auto.count.sum() == ref_bins.size and auto.mean == {} and len(auto.volume) == 9


def test_perturbation_from_the_mean_of_a_constant_model_is_zero(ctx, chunk_mesh):
    """f = c: every mean is c (1 + e), |e| <= (2 n + 2) 2^-52 with n the largest bin's count (the bound above); the lerp
    between two such values adds three roundings and (f - ref) / ref two more: (2 n + 8) 2^-52."""
    pts = chunk_mesh["points"]
    c = 4321.125
    mesh = GllMesh(pts, 4, {"VS": np.full(pts.shape[:2], c)})
    before = mesh.element_nodal_fields["VS"].copy()
    prof = api.radial_profile(mesh, ["VS"], nbins=6, context=ctx)
    bound = (2 * prof.count.max() + 8) * EPS
    rel = api.to_perturbation(mesh, ["VS"], "mean", nbins=6, context=ctx)
    assert rel.shape == (1,) + pts.shape[:2] and np.abs(rel).max() <= bound
    diff = api.to_perturbation(mesh, ["VS"], "mean", relative=False, nbins=6, context=ctx)
    assert np.abs(diff).max() <= bound * c
    assert np.array_equal(mesh.element_nodal_fields["VS"], before)                 # the mesh is untouched
    # and back, with an explicit model
    R, V = _table3()
    model = RadialModel(R, {"VS": V[0]})
    mesh2 = GllMesh(pts, 4, {"VS": api.evaluate_radial_model(model, mesh, context=ctx)[0] * 1.02})
    pert = api.to_perturbation(mesh2, ["VS"], model, context=ctx)
    assert np.abs(pert - 0.02).max() < 1e-15
    mesh3 = GllMesh(pts, 4, {"VS": pert[0]})
    back = api.from_perturbation(mesh3, ["VS"], model, context=ctx)
    assert np.abs(back[0] - mesh2.element_nodal_fields["VS"]).max() <= 4 * EPS * 5.2
    assert M.same_bits(api.evaluate_radial_model(model, mesh, context=ctx), RC.model_apply(pts, R, V[:1]).reshape(1, *pts.shape[:2]))


def test_hex_mesh_profile_and_model(ctx):
    pts, conn = synth.hex_mesh(7, seed=2, jitter=0.0, lo=(-1.0e5, -1.0e5, 6.0e6), hi=(1.0e5, 1.0e5, 6.3e6))
    c = 2.5
    mesh = HexMesh(pts, conn, {"RHO": np.full(len(pts), c)})
    prof = api.radial_profile(mesh, ["RHO"], nbins=5, context=ctx)
    assert prof.noutside == 0 and prof.count.sum() == len(pts)
    full = prof.count > 0
    assert (np.abs(prof.mean["RHO"][full] - c) <= (2 * prof.count[full] + 4) * EPS * c).all()
    assert abs(prof.volume.sum() - 2.0e5 * 2.0e5 * 3.0e5) <= 1e-9 * 1.2e16           # a regular grid: the corner rule is exact
    mass = api.hex8_mass_matrix(mesh, context=ctx)
    ref_bins, _, _ = RC.bins(pts, prof.edges)
    assert M.same_bits(prof.volume, RC.binned_weighted_sum(mass, None, ref_bins, 5)[0])
    model = RadialModel([6.0e6, 6.1e6, 6.1e6, 6.4e6], {"RHO": [2.0, 2.2, 2.6, 3.0]})
    out = api.evaluate_radial_model(model, mesh, context=ctx)
    assert out.shape == (1, len(pts))
    assert M.same_bits(out, RC.model_apply(pts, model.radius, model.table()[1]))
    assert M.same_bits(api.evaluate_radial_model(model, pts, context=ctx), out)
    pert = api.to_perturbation(mesh, ["RHO"], model, relative=False, context=ctx)
    assert M.same_bits(pert, c - out)
