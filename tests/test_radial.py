"""Radial 1-D profiles on the CPU: the NumPy statements of tests/radial_cases.py against independent routes (the
weighted sum of mass_cases, np.bincount, a linear table), the element-centre rule at a discontinuity, and the argument
handling of the API that needs no device."""
import numpy as np
import pytest

import mass_cases as M
import radial_cases as RC
from multimesh_amd import api, synth
from multimesh_amd.api import GllMesh, RadialModel

EPS = M.EPS
R_JUMP = 6_171_000.0


def _cloud(n, nbins, seed):
    rng = np.random.default_rng(seed)
    mass = rng.uniform(0.5, 2.0, n)
    field = rng.uniform(1.0, 3.0, (2, n))
    bins = rng.integers(-1, nbins + 1, n).astype(np.int32)        # -1 and nbins: no bin
    return mass, field, bins


@pytest.mark.parametrize("n", [1, 257, 4097, 4096 * 5 + 17])
def test_binned_statement_is_the_weighted_sum_of_the_masked_mass(n):
    nbins = 5
    mass, field, bins = _cloud(n, nbins, n)
    out = RC.binned_weighted_sum(mass, field, bins, nbins)
    assert out.shape == (2, nbins)
    for b in range(nbins):
        # strictly positive terms: 0.0 + t is t, so starting a lane from +0.0 or from its first term is the same sum
        ref = M.weighted_sum(np.where(bins == b, mass, 0.0), field)
        assert M.same_bits(out[:, b], ref), b
    inside = (bins >= 0) & (bins < nbins)
    for c in range(2):
        t = mass * field[c]
        direct = np.bincount(bins[inside], weights=t[inside], minlength=nbins)
        for b in range(nbins):
            assert abs(out[c, b] - direct[b]) <= 2 * M.term_bound(t[bins == b]) + EPS * abs(direct[b]), (c, b)
    assert np.array_equal(RC.bin_counts(bins, nbins), np.bincount(bins[inside], minlength=nbins))


def test_binned_statement_signs_and_non_members():
    mass = np.ones(600)
    field = np.full(600, -0.0)
    bins = np.zeros(600, dtype=np.int32)
    bins[300:] = 2
    field[400] = np.nan
    field[401] = np.inf
    out = RC.binned_weighted_sum(mass, field, bins, 4)[0]
    assert not np.signbit(out[0]) and out[0] == 0.0              # a sum of -0.0 terms from +0.0 is +0.0
    assert not np.signbit(out[1]) and not np.signbit(out[3])     # empty bins
    assert np.isnan(out[2]) and np.isfinite(out[[0, 1, 3]]).all()


def test_bins_statement_edges_and_outside():
    edges = np.array([1.0, 2.0, 4.0, 8.0])
    pts = np.zeros((7, 3))
    pts[:, 0] = [1.0, 2.0, 8.0, 0.5, 9.0, np.nan, 3.0]
    b, nout, r = RC.bins(pts, edges)
    assert b.tolist() == [0, 1, 2, -1, -1, -1, 1] and nout == 3 and b.dtype == np.int32


def test_linear_table_is_reproduced_to_a_few_ulps():
    """V = R: ref must be the clamped radius.  t carries three roundings (two differences and the quotient), so the exact
    lerp at the computed t is off by at most 3u t h <= 3u Rmax (u = 2^-53, h the interval); 1 - t and the product with R[i]
    add 2u Rmax, the second product u Rmax, the final sum u Rmax: 7u Rmax, asserted as 8u Rmax = 4 ulp of Rmax."""
    rng = np.random.default_rng(2)
    R = np.sort(rng.uniform(3.0e6, 6.4e6, 40))
    pts = rng.normal(size=(5000, 3))
    pts *= (rng.uniform(2.9e6, 6.5e6, 5000) / np.linalg.norm(pts, axis=1))[:, None]
    out = RC.model_apply(pts, R, R[None, :])[0]
    want = np.clip(RC.radius(pts), R[0], R[-1])
    assert np.abs(out - want).max() <= 8 * 2.0 ** -53 * R[-1]
    assert (want == R[0]).any() and (want == R[-1]).any()         # both clamps are exercised


def test_nodes_on_a_discontinuity_take_the_side_of_their_element():
    ch = synth.earth_chunk(order=2)
    R = np.array([5.9e6, R_JUMP, R_JUMP, 6.4e6])
    V = np.array([[1.0, 1.0, 2.0, 2.0]])
    out = RC.model_apply(ch["points"], R, V)[0].reshape(ch["points"].shape[:2])
    on = ch["z_node_1D"] == R_JUMP / synth.R_EARTH
    below, above = ch["layer"] == 1, ch["layer"] == 2
    assert on[below].any() and on[above].any()
    r = RC.radius(ch["points"]).reshape(on.shape)
    assert (r[on] < R_JUMP).any() or (r[on] > R_JUMP).any()       # the computed radii do not all sit on the jump
    # (the lerp of a constant is the constant within 1 - t's rounding, the two products' and the sum's: 4u of it)
    assert (np.abs(out[below] - 1.0) <= 4 * 2.0 ** -53).all() and (np.abs(out[above] - 2.0) <= 8 * 2.0 ** -53).all()
    # P = 1: a point exactly on the discontinuity takes the upper side
    assert RC.model_apply(np.array([[R_JUMP, 0.0, 0.0]]), R, V)[0, 0] == 2.0


def test_apply_statement_beyond_the_table_and_nan():
    R = np.array([2.0, 3.0, 3.0, 4.0])
    V = np.array([[10.0, 20.0, 30.0, 50.0]])
    pts = np.zeros((4, 1, 3))
    pts[:, 0, 0] = [1.0, 5.0, np.nan, 3.5]
    out = RC.model_apply(pts, R, V)[0]
    assert out[0] == 10.0 and out[1] == 50.0 and np.isnan(out[2]) and out[3] == 40.0
    back = RC.model_apply(pts, R, V, mode=4, values_in=RC.model_apply(pts, R, V, mode=2, values_in=[[11.0, 49.0, 1.0, 44.0]]))
    assert np.allclose(back[0][[0, 1, 3]], [11.0, 49.0, 44.0], rtol=1e-15)


@pytest.mark.parametrize("radius", [[1.0, 2.0, 2.0, 2.0, 3.0], [1.0, 1.0, 2.0], [1.0, 2.0, 2.0], [1.0, 2.0, 1.5],
                                    [1.0, np.inf], [1.0, np.nan, 3.0], [1.0]])
def test_radial_model_refuses_what_is_not_a_set_of_layers(radius):
    with pytest.raises(ValueError):
        RadialModel(radius, {"v": np.zeros(len(radius))})
    with pytest.raises(ValueError):
        RC.layers(radius)


def test_radial_model_holds_the_table():
    m = RadialModel([1.0, 2.0, 2.0, 3.0, 4.0], {"VS": [1, 2, 3, 4, 5], "RHO": [5, 4, 3, 2, 1]})
    assert m.layers == [(0, 1), (2, 4)] == RC.layers(m.radius)
    names, table = m.table(["RHO"])
    assert names == ["RHO"] and table.tolist() == [[5, 4, 3, 2, 1]]
    m2 = RadialModel.from_arrays(m.radius, m.table()[1], m.parameters)
    assert m2.parameters == ["VS", "RHO"] and np.array_equal(m2.values["RHO"], m.values["RHO"])
    with pytest.raises(ValueError):
        RadialModel([1.0, 2.0], {"v": [1.0, 2.0, 3.0]})
    with pytest.raises(ValueError):
        m.table(["VP"])


def test_profile_to_radial_model_skips_empty_bins():
    prof = api.RadialProfile([0.0, 1.0, 2.0, 3.0, 4.0], [1.0, 0.0, 2.0, 1.0], [3, 0, 5, 1], 2,
                             {"v": np.array([1.0, np.nan, 3.0, 4.0])}, {"v": np.array([1.0, np.nan, 3.0, 4.0])})
    m = prof.to_radial_model()
    assert m.radius.tolist() == [0.5, 2.5, 3.5] and m.values["v"].tolist() == [1.0, 3.0, 4.0] and len(m.layers) == 1
    with pytest.raises(ValueError):
        api.RadialProfile([0.0, 1.0, 2.0], [1.0, 0.0], [3, 0], 0, {}, {}).to_radial_model()


def test_default_edges_cover_the_mesh():
    ch = synth.earth_chunk(order=4, ellipticity=3e-3)
    for nbins in (1, 7, 64):
        edges = api.radial_edges(ch["points"], nbins)
        r = RC.radius(ch["points"])
        assert edges.shape == (nbins + 1,) and edges[0] == r.min() and edges[-1] == r.max()
        assert (np.diff(edges) > 0).all()
        b, nout, _ = RC.bins(ch["points"], edges)
        assert nout == 0 and b.min() == 0 and b.max() == nbins - 1
    with pytest.raises(ValueError):
        api.radial_edges(ch["points"], 0)
    with pytest.raises(ValueError):
        api.radial_edges(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), 4)    # one radius: no range


def test_radial_profile_checks_its_arguments_before_it_asks_for_a_device():
    ch = synth.earth_chunk(order=2)
    mesh = GllMesh(ch["points"], 2, {"VS": np.ones(ch["points"].shape[:2])})
    with pytest.raises(ValueError):
        api.radial_profile(mesh, ["VS"], edges=[5.9e6, 6.4e6], nbins=4)
    for edges in ([6.4e6, 5.9e6], [5.9e6], [5.9e6, np.nan], [[5.9e6, 6.4e6]]):
        with pytest.raises(ValueError):
            api.radial_profile(mesh, ["VS"], edges=edges)
    with pytest.raises(ValueError):
        api.radial_profile(mesh, ["VP"], nbins=4)
    with pytest.raises(ValueError):
        api.radial_profile(mesh, ["VS"], nbins=0)
    with pytest.raises(ValueError):
        api.to_perturbation(mesh, ["VS"], "median")
    with pytest.raises(ValueError):
        api.from_perturbation(mesh, ["VS"], "mean")
