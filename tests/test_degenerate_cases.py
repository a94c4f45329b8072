"""The scenarios of tests/degenerate_cases.py, checked on the CPU against the oracle and the host build of the kernels'
Newton solve alone: the degenerate elements really accept targets, make others fail or fall back, tie exactly in the kNN,
leave the fast Newton unsure and the GLL transform NaN.  A GPU test over a scenario that misses these would prove nothing."""
import numpy as np
import pytest

import degenerate_cases as G
from oracle import oracle as O
from test_newton_host import fast_stats, host  # noqa: F401  (host: the fixture that builds tests/host/newton_host.cpp)


def test_bad_hex_mesh_holds_every_kind_and_its_targets():
    pa, ca, pb, fields, nn, kind = G.bad_hex_mesh()
    assert (kind == G.REGULAR).sum() == 1331 and 55 <= (kind != G.REGULAR).sum() <= 65
    for code in (G.FLAT, G.ZERO, G.MIRRORED, G.TANGLED, G.EDGE, G.FACE, G.DUPLICATE):
        assert (kind == code).sum() >= 5, G.KIND_NAMES[code]
    assert (kind == G.HUGE).sum() == 1 and (kind == G.TINY).sum() == 1
    assert 5500 <= len(pb) <= 6500 and fields.shape == (3, len(pa))
    v = pa[ca]
    # flat: the eight nodes in one plane; zero-size: one point; collapsed: a repeated node id; the appended own their nodes
    for e in np.flatnonzero(kind == G.FLAT):
        assert np.linalg.svd(v[e] - v[e].mean(0), compute_uv=False)[2] < 1e-15
    assert (np.ptp(v[kind == G.ZERO], axis=1) == 0).all()
    assert all(len(set(r)) < 8 for r in ca[np.isin(kind, (G.EDGE, G.FACE))])
    own = ca[(kind != G.REGULAR) & (kind != G.DUPLICATE)]
    assert own.min() >= 12 ** 3 and len(np.unique(own)) == len(set(own.ravel()))
    assert (ca[kind == G.REGULAR].max() < 12 ** 3)
    huge = v[kind == G.HUGE][0]
    assert (huge.min(0) < pa[:1728].min(0)).all() and (huge.max(0) > pa[:1728].max(0)).all()
    assert 0 < G.shortest_edge(pa, ca)[kind == G.TINY][0] < 2e-9
    # targets: exactly on the appended elements' nodes and centroids, and far outside
    added = np.flatnonzero(kind != G.REGULAR)
    rows = {r.tobytes() for r in pb}
    assert all(p.tobytes() in rows for p in v[added].reshape(-1, 3)) and all(p.tobytes() in rows for p in v[added].mean(1))
    assert (np.abs(pb).max(axis=1) > 1.5).sum() == 300


def test_bad_hex_mesh_duplicates_tie_exactly_and_go_by_index():
    pa, ca, pb, fields, nn, kind = G.bad_hex_mesh()
    cen = O.centroid(ca, pa)
    dup = np.flatnonzero(kind == G.DUPLICATE)
    first = [int(np.flatnonzero((ca[:1331] == ca[e]).all(axis=1))[0]) for e in dup]
    assert all(cen[a].tobytes() == cen[b].tobytes() for a, b in zip(first, dup))
    idx, d2 = O.knn_brute(cen, pb, 20, want_d2=True)
    tie = d2[:, 1:] == d2[:, :-1]
    assert tie.sum() > 100 and (np.diff(idx, axis=1)[tie] > 0).all()
    pos = {int(b): int(a) for a, b in zip(first, dup)}
    follows = sum(1 for r in idx for a, b in zip(r[:-1], r[1:]) if pos.get(int(b)) == int(a))
    assert follows > 100                                             # the duplicate directly behind its original


def test_bad_hex_mesh_accepts_fails_and_falls_back():
    pa, ca, pb, fields, nn, kind = G.bad_hex_mesh()
    comparable = G.comparable_elements(pa, ca, kind)
    for k in G.HEX_KS:
        enc, w, nf, status = G.bad_hex_oracle(k)
        elem = G.accepted_element(status, nn, k)
        located = elem >= 0
        in_kind = {code: int((kind[elem[located]] == code).sum()) for code in range(1, 10)}
        assert nf > 100 and nf == (status < 0).sum()                                # some targets fail
        assert (status >= k).sum() > 100                                            # some fall back to the best candidate
        for code in (G.MIRRORED, G.TANGLED, G.EDGE, G.FACE, G.TINY):                # some are accepted in a degenerate element
            assert in_kind[code] > 10, (k, in_kind)
        assert not enc[status < 0].any() and not w[status < 0].any()
        # MM_FP_TOL's bound speaks about at least 80 % of the located targets (the targets a tol-mode comparison can use)
        assert comparable[elem[located]].mean() >= 0.8, (k, comparable[elem[located]].mean())
    st1, st20 = G.bad_hex_oracle(1)[3], G.bad_hex_oracle(20)[3]
    assert ((st1 >= 0) != (st20 >= 0)).sum() > 0                                    # k decides whether a target is located
    assert ((st20 < 0) | (st20 >= 20)).sum() > 500                                  # these fetch their full lists (lazy lists)
    # the bound is void exactly on the collapsed elements: their shortest edge is zero
    void = ~np.isfinite(G.fp_tol_rows(pa, ca))
    assert np.array_equal(void, np.isin(kind, (G.ZERO, G.EDGE, G.FACE)))


def test_bad_hex_mesh_leaves_the_fast_newton_unsure(host):  # noqa: F811
    # every (target, candidate) pair of the k = 20 lists through newton_hex8_fast (the host build of csrc/mm_newton_hex8.h):
    # it never certifies a wrong verdict, and at least 5 % of the solves are "unsure" -- the slow lists, their compaction,
    # the second pass and the reference-order kernel have work to do.  Measured: 17.6 % of 116500 solves.
    pnt, vtx = G.newton_pairs(20)
    st = fast_stats(host, pnt, vtx)
    print(f"bad_hex_mesh: {len(pnt)} solves, {st}")
    assert st["wrong"] == 0, st
    assert st["unsure"] >= 0.05 * len(pnt), st


@pytest.mark.parametrize("order,dim", [(o, d) for o in (1, 2, 4) for d in (2, 3)])
def test_bad_gll_meshes_give_nan_transforms_and_misses(order, dim):
    gp, pts, fields, nn, kind = G.bad_gll_mesh(order, dim)
    P = (order + 1) ** dim
    assert gp.shape[1:] == (P, dim) and fields.shape == (3,) + gp.shape[:2] and 2500 <= len(pts) <= 3500
    for code in (G.FLAT, G.ZERO, G.MIRRORED, G.DUPLICATE) + ((G.FOLDED,) if order > 1 else ()):
        assert (kind == code).sum() >= 4, G.KIND_NAMES[code]
    assert (np.ptp(gp[kind == G.ZERO], axis=1) == 0).all()
    # folded: the node in the middle of the face xi_1 = -1 lies beyond the middle of the face xi_1 = +1
    m, mid = order + 1, (order + 1) // 2
    lo = mid * m + (mid * m * m if dim == 3 else 0)
    for el in gp[kind == G.FOLDED]:
        centre = el.mean(axis=0)
        assert np.dot(el[lo] - el[lo + m - 1], el[lo + m - 1] - centre) > 0
    # ... so that the Jacobian changes sign inside; a mirrored element's is negative everywhere, a flat or zero-size
    # element's zero (to rounding, against the regular elements' scale), a regular element's positive
    det = G.gll_node_determinants(order, gp)
    scale = det[kind == G.REGULAR].min()
    assert scale > 0
    for el in det[kind == G.FOLDED]:
        assert el.min() < -0.1 * scale and el.max() > 0.1 * scale
    assert (det[kind == G.MIRRORED] < 0).all()
    assert (np.abs(det[np.isin(kind, (G.FLAT, G.ZERO))]) < 1e-12 * scale).all()
    for el in gp[kind == G.FLAT]:                                    # every node on one plane (3-D) or line (2-D)
        sv = np.linalg.svd(el - el.mean(0), compute_uv=False)
        assert sv[dim - 1] < 1e-13 * sv[0]
    # targets on the corners and the centroid of every appended element
    rows = {r.tobytes() for r in pts}
    for el in gp[kind != G.REGULAR]:
        assert el[0].tobytes() in rows and el[-1].tobytes() in rows and el.mean(axis=0).tobytes() in rows
    cen = gp.mean(axis=1)
    dup = np.flatnonzero(kind == G.DUPLICATE)
    assert all((cen[: dup[0]] == cen[e]).all(axis=1).any() for e in dup)
    for k in G.GLL_KS:
        elem, co, hard = O.locate_gll_v1(order, nn[:, :k], gp, pts)
        assert hard > 0, (k, hard)                                   # NaN transforms
        elem, co, miss = O.locate_gll(order, nn[:, :k], gp, pts)
        assert miss > 0 and (kind[elem[elem >= 0]] != G.REGULAR).sum() > 20, (k, miss)


def test_nonfinite_targets_and_mesh():
    pa, ca, pb, fields = G.good_hex_mesh()
    bad, mask = G.nonfinite_targets(pb)
    n = len(pb)
    assert 0.008 * n <= mask.sum() <= 0.04 * n
    assert mask[[0, n - 1, 63, 64, 65, 255, 256, 257]].all() and mask[n // 2:n // 2 + 70].all()
    assert np.array_equal(bad[~mask], pb[~mask]) and not np.shares_memory(bad, pb)
    row = bad[mask]
    assert (np.isnan(row).sum(axis=1) == 1).any() and np.isnan(row).all(axis=1).any()
    assert (row == np.inf).any() and (row == -np.inf).any() and (row == 1e308).any() and (row == -1e308).any()
    assert (~np.isfinite(row) | (np.abs(row) == 1e308)).any(axis=1).all()
    pa2, ca2, pb2, f2, affected = G.nonfinite_mesh()
    assert np.isnan(pa2).sum() == 2 and np.isinf(pa2).sum() == 1 and affected.sum() == 24
    cen = O.centroid(ca2, pa2)
    assert np.array_equal(~np.isfinite(cen).all(axis=1), affected)
