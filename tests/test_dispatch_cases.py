"""The scenarios of tests/test_dispatch_matrix_gpu.py, checked on the CPU against the oracle alone: each one reaches the
branch of the kNN / locate dispatcher it is meant for (ties, padding, list lengths on each side of a threshold, targets
that need candidates beyond the 8th).  A GPU test over a scenario that misses its branch would prove nothing."""
import numpy as np
import pytest

import dispatch_cases as D


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_knn_clouds_have_ties_padding_and_unique_orders_where_claimed(dim):
    src, tgt, _ = D.knn_cloud("uniform", dim)
    idx, dist = D.knn_oracle("uniform", dim)
    assert (np.diff(dist, axis=1) > 0).all()                 # one order: every smaller k is a slice of k = 64
    assert (tgt < 0).any() and (tgt > 1).any()               # targets beyond the sources' box
    src, tgt, _ = D.knn_cloud("lattice", dim)
    idx, dist = D.knn_oracle("lattice", dim)
    tie = dist[:, 1:] == dist[:, :-1]
    assert tie.sum() > 1000 and tie[:, :19].any(axis=1).sum() > 100     # exact ties, also within short lists
    assert (np.diff(idx, axis=1)[tie] > 0).all()             # ... broken by index
    src, tgt, _ = D.knn_cloud("few", dim)
    idx, dist = D.knn_oracle("few", dim)
    assert len(src) == 13
    assert (idx[:, 13:] == 13).all() and np.isinf(dist[:, 13:]).all() and np.isfinite(dist[:, :13]).all()


def test_knn_graded_and_list_mode_clouds():
    src, tgt, idx, dist = D.graded_cloud()
    assert (np.diff(dist, axis=1) > 0).all()
    # density over orders of magnitude: the corner cubes of a tenth of the side at either end
    assert (src < 0.1).all(axis=1).sum() > 100 * max(1, (src > 0.9).all(axis=1).sum())
    for n in (5_000, 12_000):
        src, tgt, idx, dist = D.list_mode_cloud(n)
        assert (np.diff(dist, axis=1) > 0).all()
    assert len(D.list_mode_cloud(5_000)[1]) < D.LIST_WAVE_MAX < len(D.list_mode_cloud(12_000)[1])


def test_split_cloud_has_enough_targets_per_strip_for_several_waves():
    src, tgt, idx, dist = D.split_cloud()
    assert (np.diff(dist, axis=1) > 0).all()                 # one order: k = 8 is a slice of k = 25
    assert (tgt < 0).any() and (tgt > 1).any()
    # the launcher's formula at the default cell load: 8 sources per cell, two cells per strip, so nsrc / 16 strips;
    # it shares a strip among nsplit = (targets per strip + 64) / 128 waves
    assert 16 * len(tgt) / len(src) >= D.STRIP_SPLIT_MIN


def test_knn_distances_are_the_in_order_sum():
    src = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    tgt = np.array([[0.5, 0.5, 0.5]])
    d = D.knn_distances(src, tgt, np.array([[1, 2]]))
    assert d[0, 0] == np.sqrt((0.25 + 2.25) + 6.25) and np.isinf(d[0, 1])


def test_sheared_mesh_needs_candidates_beyond_the_8th_at_every_k():
    pa, ca, pb, fields, nn = D.sheared_mesh()
    for k in D.HEX_KS:
        enc, w, nf, status = D.hex8_oracle("sheared", k)
        if k > D.LAZY_K:
            # lazily evaluated lists: these targets fetch their full list, and some find their element there
            assert (status >= D.LAZY_K).sum() > 300 and ((status >= D.LAZY_K) & (status < k)).sum() > 50
        assert nf > 0 and nf == (status < 0).sum()
        assert (status >= k).sum() > 0 or k <= 2              # the smallest-error fallback
        assert not enc[status < 0].any() and not w[status < 0].any()


def test_tiny_mesh_has_fewer_elements_than_most_k():
    pa, ca, pb, fields, nn = D.tiny_mesh()
    assert len(ca) == 8 and nn.shape[1] == 8 and max(D.HEX_KS) > len(ca)
    enc, w, nf, status = D.hex8_oracle("tiny", 8)
    assert nf > 0 and (status >= 0).sum() > 1000


def test_graded_mesh_gives_a_long_list_and_a_second_pass_at_every_k():
    enc, w, nf, status8 = D.hex8_oracle("graded", 8)
    assert D.no_accept_within(status8, D.LAZY_K).sum() >= D.LONG_LIST_MIN
    enc, w, nf, status = D.hex8_oracle("graded", max(D.LONG_KS))
    assert np.array_equal(D.no_accept_within(status, D.LAZY_K), D.no_accept_within(status8, D.LAZY_K))
    # what the second pass leaves to the reference-order kernel shrinks with k: present at the longest list
    assert D.no_accept_within(status, max(D.LONG_KS)).sum() > 0


@pytest.mark.parametrize("nfar,k", D.OUTSIDE_CASES)
def test_outside_mesh_puts_its_lists_on_each_side_of_65536(nfar, k):
    enc, w, nf, status = D.outside_oracle(nfar, k)
    lazy = D.no_accept_within(status, min(k, D.LAZY_K)).sum()
    eager = D.no_accept_within(status, k).sum()
    assert nf >= nfar and (status >= k).sum() > 100          # every far target fails; the band falls back
    assert not enc[status < 0].any() and not w[status < 0].any()
    enc, w, nf_s, staged = D.outside_oracle(nfar, k, staged=True)
    assert nf_s >= nfar and (staged == 2 * k - 1).sum() > 50         # falls back to the last candidate
    staged = D.no_accept_within(staged, k).sum()
    if nfar == D.OUTSIDE_SMALL:
        assert max(lazy, eager, staged) < D.GROUP_LIST_MAX
    else:
        assert min(lazy, eager, staged) >= 70_000


@pytest.mark.parametrize("order,dim", [(o, d) for o in (1, 2, 4) for d in (2, 3)])
def test_gll_cases_need_candidates_beyond_the_8th(order, dim):
    from oracle import oracle as O

    gp, pts, fields, nn = D.gll_case(order, dim)
    assert gp.shape[0] >= max(D.GLL_KS)
    elem, co, miss = O.locate_gll(order, nn[:, :25], gp, pts)
    beyond8 = ((elem[:, None] != nn[:, :8]).all(axis=1) & (elem >= 0)).sum()
    assert miss > 0 and beyond8 > 0


def test_gather_cases_hold_negative_zeros():
    for P in (1, 8, 128):
        fields, ids, w = D.gather_case(P, 3)
        assert np.signbit(w[w == 0]).any() and (fields == 0).any() and ids.max() < fields.shape[1]
