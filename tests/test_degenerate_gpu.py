"""Locate, kNN and the fused pipelines on degenerate elements and non-finite coordinates, against the oracle bit for bit.

The scenarios (tests/degenerate_cases.py; their CPU-side preconditions: tests/test_degenerate_cases.py) hold flat,
zero-size, mirrored, tangled, collapsed, duplicated, huge and tiny elements, folded GLL elements, targets with NaN, inf
and 1e308 coordinates and meshes with NaN and inf nodes.  The locate stage is the reference's arithmetic on whatever it
is given, so every one of these has a right answer: the oracle's.  The kNN stage promises, for non-finite rows, indices
in [0, nsrc] and the same rows on every route, and leaves the finite rows as they are without the others
(include/multimesh_hip.h).  Knobs read once per process (MM_KNN_KERNEL) run in child processes, one per knob.

What these tests cannot tell apart, by construction.  The lane kernel's `finite` flag on a target: without it a NaN or
infinite target still gets a NaN or infinite k-th key and is handed to the ring search by `!(kth < INFINITY)`, so its row
is the same.  The hex8 hull prefilter's treatment of NaN: a candidate with a NaN corner, or any candidate of a NaN target,
has a NaN Newton iterate and is accepted by nobody, and what the first pass does not accept is decided again by the
reference-order kernel, which has no prefilter -- in these scenes the oracle accepts no such candidate (no row has a NaN
weight, all 78 non-finite targets fail, no target is located in an element with a non-finite node).  Those two branches
are therefore covered for faults and bounds, not for results."""
import os
import subprocess
import sys

import numpy as np
import pytest

import degenerate_cases as G
import dispatch_cases as D
from multimesh_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF_KS = (1, 8, 20)


@pytest.fixture(scope="module")
def ctx():
    from multimesh_amd.device import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_tol():
    from multimesh_amd.device import Context

    c = Context(0)
    c.set_fp_mode("tol")
    yield c
    c.close()


def same(a, b):
    """Bit-identical up to NaN payloads: equal with NaN == NaN, and equal sign bits where the values are finite."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
        return False
    if a.dtype.kind != "f":
        return True
    fin = np.isfinite(b)
    return np.array_equal(np.signbit(a[fin]), np.signbit(b[fin]))


# ------------------------------------------------------------------------------------------------------------ hex8, exact
@pytest.mark.parametrize("k", G.HEX_KS)
def test_hex8_staged_locate_and_knn_on_degenerate_elements(ctx, k):
    pa, ca, pb, fields, nn, kind = G.bad_hex_mesh()
    enc_o, w_o, nf_o, status = G.bad_hex_oracle(k)
    failed = status < 0
    lists = np.ascontiguousarray(nn[:, :k])
    # kNN over centroids with exact duplicates: the brute-force rows, ties by index
    tree = ctx.knn_build(O.centroid(ca, pa))
    idx, dist = tree.query(pb, k, want_dist=True)
    tree.free()
    assert np.array_equal(idx.numpy(), lists), (k, sorted(ctx.last_knn_kernels()))
    assert np.array_equal(dist.numpy(), D.knn_distances(O.centroid(ca, pa), pb, lists))
    # the staged call into arrays the caller filled: rows of failed targets keep what was there
    enc0, w0 = np.full((len(pb), 8), 7, np.int64), np.full((len(pb), 8), 0.25)
    for conn, exodus in ((synth.reorder_hex8(ca), False), (ca, True)):
        enc, w, nf = ctx.locate_hex8(lists, conn, pa, pb, enc=ctx.to_device(enc0), weights=ctx.to_device(w0),
                                     conn_is_exodus=exodus)
        enc, w = enc.numpy(), w.numpy()
        st = ctx.last_locate_stats()
        print(f"staged exact k {k}: failed {nf}, fallback {(status >= k).sum()}, stats {st}")
        assert nf == nf_o
        assert np.array_equal(enc[~failed], enc_o[~failed]) and same(w[~failed], w_o[~failed])
        assert np.array_equal(enc[failed], enc0[failed]) and np.array_equal(w[failed], w0[failed])
        assert st["reference_order"] > 0


@pytest.mark.parametrize("k", G.HEX_KS)
def test_hex8_fused_pipeline_on_degenerate_elements(ctx, k):
    pa, ca, pb, fields, nn, kind = G.bad_hex_mesh()
    enc_o, w_o, nf_o, status = G.bad_hex_oracle(k)
    vals_o = O.gather(fields, enc_o, w_o)
    for lazy in (True, False):
        ctx.set_lazy_lists(lazy)
        try:
            vals, enc, w, nf = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k, want_operator=True)
            st = ctx.last_locate_stats()
            vals2, nf2 = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k)          # values only
        finally:
            ctx.set_lazy_lists(True)
        assert nf == nf2 == nf_o, (k, lazy, nf, nf2, nf_o)
        assert np.array_equal(enc.numpy(), enc_o) and same(w.numpy(), w_o), (k, lazy)
        assert same(vals.numpy(), vals_o) and same(vals2.numpy(), vals_o), (k, lazy)
        assert st["reference_order"] > 0


@pytest.mark.parametrize("k", [1, 20, 64])
def test_hex8_resident_source_and_host_entry_on_degenerate_elements(ctx, k):
    pa, ca, pb, fields, nn, kind = G.bad_hex_mesh()
    enc_o, w_o, nf_o, status = G.bad_hex_oracle(k)
    vals_o = O.gather(fields, enc_o, w_o)
    src = ctx.source(pa, ca)
    try:
        vals, enc, w, nf = src.interpolate(pb, fields, nelem_to_search=k, want_operator=True)
        vals2, nf2 = src.interpolate(pb, fields, nelem_to_search=k)
    finally:
        src.free()
    assert nf == nf2 == nf_o and np.array_equal(enc.numpy(), enc_o) and same(w.numpy(), w_o)
    assert same(vals.numpy(), vals_o) and same(vals2.numpy(), vals_o)
    vals, enc, w, nf = ctx.interpolate_hex8_host(pa, ca, pb, fields, nelem_to_search=k, want_operator=True)
    assert nf == nf_o and np.array_equal(enc, enc_o) and same(w, w_o) and same(vals, vals_o)
    vals2, nf2 = ctx.interpolate_hex8_host(pa, ca, pb, fields, nelem_to_search=k)
    assert nf2 == nf_o and same(vals2, vals_o)


# ------------------------------------------------------------------------------------------------------------ hex8, MM_FP_TOL
@pytest.mark.parametrize("k", G.HEX_KS)
def test_hex8_tol_mode_on_degenerate_elements(ctx_tol, k):
    # the reference-order path serves every target that none of its candidates accepts: by the oracle 864 of the 5825
    # targets at k >= 8 (382 fail, 482 fall back), 1489 at k = 1; the stats are printed
    pa, ca, pb, fields, nn, kind = G.bad_hex_mesh()
    enc_o, w_o, nf_o, status = G.bad_hex_oracle(k)
    vals_o = O.gather(fields, enc_o, w_o)
    elem = G.accepted_element(status, nn, k)
    located = elem >= 0
    # The header's bound divides by the element's shortest edge: it gives no bound on an element with a collapsed edge
    # (and says nothing about elements that lost their orientation).  Weights and values are compared on the targets
    # located in the other elements, each against the bound of its own element.
    compared = located & G.comparable_elements(pa, ca, kind)[np.maximum(elem, 0)]
    bound = G.fp_tol_rows(pa, ca)[elem[compared]]
    assert np.isfinite(bound).all() and compared.sum() >= 0.8 * located.sum()
    outs = []
    vals, enc, w, nf = ctx_tol.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k, want_operator=True)
    st = ctx_tol.last_locate_stats()
    print(f"tol fused k {k}: failed {nf}, compared {compared.sum()} of {located.sum()} located, stats {st}")
    assert st["reference_order"] > 0 and st["redone_exact"] > 0
    outs.append((enc.numpy(), w.numpy(), nf, vals.numpy()))
    enc, w, nf = ctx_tol.locate_hex8(np.ascontiguousarray(nn[:, :k]), synth.reorder_hex8(ca), pa, pb)
    st = ctx_tol.last_locate_stats()
    print(f"tol staged k {k}: stats {st}")
    assert st["reference_order"] > 0
    outs.append((enc.numpy(), w.numpy(), nf, None))
    for enc, w, nf, vals in outs:
        assert nf == nf_o and np.array_equal(enc, enc_o)                      # ids and the failed count: every target
        assert not w[~located].any()
        err = np.abs(w[compared] - w_o[compared]).max(axis=1)
        assert (err <= bound).all(), (k, err.max(), np.flatnonzero(err > bound)[:5])
        if vals is not None:
            verr = np.abs(vals[compared] - vals_o[compared]).max(axis=1)
            assert (verr <= bound * 8 * np.abs(fields).max()).all(), (k, verr.max())


# ------------------------------------------------------------------------------------------------------------ GLL
@pytest.mark.parametrize("order,dim", [(o, d) for o in (1, 2, 4) for d in (2, 3)])
def test_gll_locate_and_pipeline_on_degenerate_elements(ctx, order, dim):
    gp, pts, fields, nn, kind = G.bad_gll_mesh(order, dim)
    for k in G.GLL_KS:
        lists = np.ascontiguousarray(nn[:, :k])
        for tol, snap in ((1.05, False), (1.05, True), (1.03, False)):
            elem_o, co_o, miss_o = O.locate_gll(order, lists, gp, pts, tolerance=tol, snap_to_nearest=snap)
            vals_o = O.gather_elem(fields, elem_o, co_o)
            elem, co, miss = ctx.locate_gll(order, lists, gp, pts, tolerance=tol, snap_to_nearest=snap)
            assert miss == miss_o and np.array_equal(elem.numpy(), elem_o) and same(co.numpy(), co_o), (k, tol, snap)
            assert same(ctx.gather_elem(fields, elem, co).numpy(), vals_o), (k, tol, snap)
            for lazy in (True, False):
                ctx.set_lazy_lists(lazy)
                try:
                    v, el, c2, m2 = ctx.interpolate_gll(order, gp, pts, fields, nelem_to_search=k, tolerance=tol,
                                                        snap_to_nearest=snap, want_operator=True)
                finally:
                    ctx.set_lazy_lists(True)
                assert m2 == miss_o and np.array_equal(el.numpy(), elem_o) and same(c2.numpy(), co_o), (k, tol, snap, lazy)
                assert same(v.numpy(), vals_o), (k, tol, snap, lazy)
        elem_o, co_o, hard_o = O.locate_gll_v1(order, lists, gp, pts)
        elem, co, hard = ctx.locate_gll_bbox(order, lists, gp, pts)
        print(f"GLL order {order} dim {dim} k {k}: miss {miss_o} (tolerance 1.03), hard {hard_o}")
        assert hard == hard_o > 0 and np.array_equal(elem.numpy(), elem_o) and same(co.numpy(), co_o), k
        assert same(ctx.gather_elem(fields, elem, co).numpy(), O.gather_elem(fields, elem_o, co_o))


# ------------------------------------------------------------------------------------------------------------ non-finite targets
def test_staged_hex8_locate_with_nonfinite_targets(ctx, ctx_tol):
    # lists of the unmodified targets: a non-finite target still walks real candidates
    for mesh in ("good", "bad"):
        if mesh == "good":
            pa, ca, pb, fields = G.good_hex_mesh()
            nn = O.knn_brute(O.centroid(ca, pa), pb, 20)
            kind = np.zeros(len(ca), np.int64)
        else:
            pa, ca, pb, fields, nn, kind = G.bad_hex_mesh()
            nn = np.ascontiguousarray(nn[:, :20])
        bad, mask = G.nonfinite_targets(pb)
        conn = synth.reorder_hex8(ca)
        enc_o, w_o, nf_o, status = O.locate_hex8(nn, conn, pa, bad, want_status=True)
        enc, w, nf = ctx.locate_hex8(nn, conn, pa, bad)
        print(f"{mesh} mesh: {mask.sum()} non-finite targets, {(status[mask] < 0).sum()} of them fail, failed in all {nf_o}")
        assert nf == nf_o and np.array_equal(enc.numpy(), enc_o) and same(w.numpy(), w_o), mesh
        # MM_FP_TOL: ids and the failed count on every row; weights of the non-finite rows as the oracle's, bit for bit,
        # of the finite rows within the bound of the element (where it has one)
        enc, w, nf = ctx_tol.locate_hex8(nn, conn, pa, bad)
        enc, w = enc.numpy(), w.numpy()
        assert nf == nf_o and np.array_equal(enc, enc_o), mesh
        assert same(w[mask], w_o[mask]), mesh
        elem = G.accepted_element(status, nn, 20)
        compared = ~mask & (elem >= 0) & G.comparable_elements(pa, ca, kind)[np.maximum(elem, 0)]
        err = np.abs(w[compared] - w_o[compared]).max(axis=1)
        assert (err <= G.fp_tol_rows(pa, ca)[elem[compared]]).all(), (mesh, err.max())
        assert not w[elem < 0].any()


@pytest.mark.parametrize("order,dim", [(o, d) for o in (1, 2, 4) for d in (2, 3)])
def test_staged_gll_locate_with_nonfinite_targets(ctx, order, dim):
    gp, pts, fields, nn, kind = G.bad_gll_mesh(order, dim)
    bad, mask = G.nonfinite_targets(pts)
    lists = np.ascontiguousarray(nn[:, :20])
    for tol, snap in ((1.05, False), (1.05, True)):
        elem_o, co_o, miss_o = O.locate_gll(order, lists, gp, bad, tolerance=tol, snap_to_nearest=snap)
        elem, co, miss = ctx.locate_gll(order, lists, gp, bad, tolerance=tol, snap_to_nearest=snap)
        assert miss == miss_o and np.array_equal(elem.numpy(), elem_o) and same(co.numpy(), co_o), (tol, snap)
    elem_o, co_o, hard_o = O.locate_gll_v1(order, lists, gp, bad)
    elem, co, hard = ctx.locate_gll_bbox(order, lists, gp, bad)
    assert hard == hard_o and np.array_equal(elem.numpy(), elem_o) and same(co.numpy(), co_o)


def knn_nonfinite_scenes():
    """(name, sources, targets with non-finite rows, their mask): uniform clouds in 2 and 3 dimensions (20000 sources in
    3-D: the lane kernel and the tree apply), and the centroids of nonfinite_mesh -- non-finite SOURCES -- under finite
    and non-finite targets."""
    out = []
    for dim in (2, 3):
        src, tgt, _ = D.knn_cloud("uniform", dim)
        bad, mask = G.nonfinite_targets(tgt)
        out.append((f"uniform{dim}", src, bad, mask))
    pa, ca, pb, _, _ = G.nonfinite_mesh()
    cen = O.centroid(ca, pa)
    out.append(("nan_sources", cen, pb, np.zeros(len(pb), bool)))
    bad, mask = G.nonfinite_targets(pb)
    out.append(("nan_both", cen, bad, mask))
    return out


def knn_nonfinite_results(ctx):
    """{scene_k: idx, scene_k_d: dist} of every scene and k on the route the process's knobs select; the finite rows
    are checked here against the same call on the finite targets alone (indices and distances bit for bit).  Also
    {scene: kernels that ran}: only uniform3 has the sources (>= 4096, a finite cube) for the tree, so the scenes with
    non-finite SOURCES compare the grid kernels under each knob, never the tree's cells."""
    out, ran = {}, {}
    for name, src, tgt, mask in knn_nonfinite_scenes():
        index = ctx.knn_build(src)
        for k in NF_KS:
            idx, dist = index.query(tgt, k, want_dist=True)                      # (a) MM_OK, or this raises
            ran[name] = ran.get(name, set()) | ctx.last_knn_kernels()
            idx, dist = idx.numpy(), dist.numpy()
            if mask.any():
                idx_f, dist_f = index.query(np.ascontiguousarray(tgt[~mask]), k, want_dist=True)
                assert np.array_equal(idx[~mask], idx_f.numpy()), (name, k)       # (b)
                assert np.array_equal(dist[~mask], dist_f.numpy(), equal_nan=True), (name, k)
            assert idx.min() >= 0 and idx.max() <= len(src), (name, k)            # (c)
            out[f"{name}_{k}"], out[f"{name}_{k}_d"] = idx, dist
        index.free()
    return out, ran


@pytest.fixture(scope="module")
def default_route(ctx):
    """The default route's arrays: module-scoped, so computed before any test sets a knob."""
    return knn_nonfinite_results(ctx)[0]


def assert_same_route(got, want, route):
    assert sorted(got) == sorted(want)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=key.endswith("_d")), (route, key,
                                                                                  np.flatnonzero((got[key] != want[key]).any(axis=1))[:5])


def test_knn_with_nonfinite_targets_and_sources_default_route(default_route):
    res = default_route
    # finite rows against the oracle (uniform clouds: cKDTree; the centroids: brute force over the finite sources)
    for dim in (2, 3):
        src, tgt, _ = D.knn_cloud("uniform", dim)
        ref, refd = D.knn_oracle("uniform", dim)
        mask = G.nonfinite_targets(tgt)[1]
        for k in NF_KS:
            assert np.array_equal(res[f"uniform{dim}_{k}"][~mask], ref[~mask, :k])
            assert np.array_equal(res[f"uniform{dim}_{k}_d"][~mask], refd[~mask, :k])
    pa, ca, pb, _, affected = G.nonfinite_mesh()
    cen = O.centroid(ca, pa)
    ids = np.flatnonzero(~affected)
    ref = ids[O.knn_brute(np.ascontiguousarray(cen[~affected]), pb, max(NF_KS))]
    mask = G.nonfinite_targets(pb)[1]
    finite_src = np.concatenate([~affected, [False]])                            # (the padding id nsrc: not a finite source)
    for name, rows in (("nan_sources", np.ones(len(pb), bool)), ("nan_both", ~mask)):
        for k in NF_KS:
            idx = res[f"{name}_{k}"]
            fin = finite_src[idx]
            assert (fin[:, :-1] >= fin[:, 1:]).all(), (name, k)                   # no non-finite source before a finite one
            got, want = idx[rows], ref[rows, :k]
            assert np.array_equal(np.where(fin[rows], got, -1), np.where(fin[rows], want, -1)), (name, k)
            assert fin[rows].all(), (name, k)                                      # (more finite sources than k: full rows)
            assert np.array_equal(res[f"{name}_{k}_d"][rows], D.knn_distances(cen, pb[rows], want)), (name, k)


@pytest.mark.parametrize("route", ["tree", "list"])
def test_knn_with_nonfinite_targets_and_sources_tree_and_list_mode(ctx, default_route, monkeypatch, route):
    want = default_route
    monkeypatch.setenv("MM_KNN_TREE" if route == "tree" else "MM_KNN_FORCE_LIST", "1")
    got, ran = knn_nonfinite_results(ctx)
    print(f"{route}: kernels per scene {ran}")
    assert route in ran["uniform3"], ran
    assert_same_route(got, want, route)


_KNN_FORCED = r"""
import sys
import numpy as np
sys.path[:0] = [".", "tests"]
from multimesh_amd.device import Context
import test_degenerate_gpu as T
got, ran = T.knn_nonfinite_results(Context(0))
np.savez(sys.argv[1], **{"ran_" + name: np.array(sorted(names)) for name, names in ran.items()}, **got)
print("ok")
"""


def test_knn_with_nonfinite_targets_and_sources_forced_kernels(default_route, tmp_path):
    # MM_KNN_KERNEL is read once per process: one child per kernel, one after the other; a child that fails ends the test
    want = default_route
    for kernel in ("lane", "strip", "cell"):
        path = str(tmp_path / f"{kernel}.npz")
        env = dict(os.environ, MM_KNN_KERNEL=kernel)
        r = subprocess.run([sys.executable, "-c", _KNN_FORCED, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (kernel, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
        with np.load(path) as z:
            got = {key: z[key] for key in z.files if not key.startswith("ran_")}
            ran = {key[4:]: set(z[key].tolist()) for key in z.files if key.startswith("ran_")}
        print(f"{kernel}: kernels per scene {ran}")
        assert kernel in ran["uniform3"], (kernel, ran)
        assert_same_route(got, want, kernel)


def hex8_oracle_on_gpu_lists(ctx, pa, ca, pts, k):
    """The oracle's locate over the lists the GPU's own kNN gives for pts.  A row may be padded with the id nelem (a NaN
    target is nearest to nothing; the locate skips that id): the oracle gets one more element there -- no element accepts
    a NaN target, so which one it is does not matter."""
    index = ctx.knn_build(O.centroid(ca, pa))
    lists = index.query(pts, k).numpy()
    index.free()
    padded = (lists >= len(ca)).any(axis=1)
    assert np.isnan(pts[padded]).any(axis=1).all()
    conn = synth.reorder_hex8(ca)
    return O.locate_hex8(lists, np.concatenate([conn, conn[:1]]), pa, pts)


@pytest.mark.parametrize("k", NF_KS)
def test_fused_hex8_pipeline_with_nonfinite_targets(ctx, k):
    pa, ca, pb, fields = G.good_hex_mesh()
    bad, mask = G.nonfinite_targets(pb)
    for lazy in (True, False):
        ctx.set_lazy_lists(lazy)
        try:
            vals, enc, w, nf = ctx.interpolate_hex8(pa, ca, bad, fields, nelem_to_search=k, want_operator=True)
            vals_f, enc_f, w_f, nf_f = ctx.interpolate_hex8(pa, ca, np.ascontiguousarray(bad[~mask]), fields, nelem_to_search=k,
                                                            want_operator=True)
        finally:
            ctx.set_lazy_lists(True)
        vals, enc, w = vals.numpy(), enc.numpy(), w.numpy()
        assert np.array_equal(enc[~mask], enc_f.numpy()) and same(w[~mask], w_f.numpy()) and same(vals[~mask], vals_f.numpy())
        enc_o, w_o, nf_o = hex8_oracle_on_gpu_lists(ctx, pa, ca, np.ascontiguousarray(bad[mask]), k)
        assert np.array_equal(enc[mask], enc_o) and same(w[mask], w_o) and same(vals[mask], O.gather(fields, enc_o, w_o))
        assert nf == nf_f + nf_o, (k, lazy, nf, nf_f, nf_o)


@pytest.mark.parametrize("order,dim", [(1, 2), (2, 3), (4, 2), (4, 3)])
def test_fused_gll_pipeline_with_nonfinite_targets(ctx, order, dim):
    gp, pts, fields, nn, kind = G.bad_gll_mesh(order, dim)
    bad, mask = G.nonfinite_targets(pts)
    index = ctx.knn_build(gp.mean(axis=1))
    for k in NF_KS:
        lists = index.query(np.ascontiguousarray(bad[mask]), k).numpy()
        for snap in (False, True):
            v, el, co, miss = ctx.interpolate_gll(order, gp, bad, fields, nelem_to_search=k, snap_to_nearest=snap, want_operator=True)
            v_f, el_f, co_f, miss_f = ctx.interpolate_gll(order, gp, np.ascontiguousarray(bad[~mask]), fields, nelem_to_search=k,
                                                          snap_to_nearest=snap, want_operator=True)
            v, el, co = v.numpy(), el.numpy(), co.numpy()
            assert np.array_equal(el[~mask], el_f.numpy()) and same(co[~mask], co_f.numpy()) and same(v[~mask], v_f.numpy())
            el_o, co_o, miss_o = O.locate_gll(order, lists, gp, bad[mask], snap_to_nearest=snap)
            assert np.array_equal(el[mask], el_o) and same(co[mask], co_o), (k, snap)
            assert same(v[mask], O.gather_elem(fields, el_o, co_o)), (k, snap)
            assert miss == miss_f + miss_o, (k, snap, miss, miss_f, miss_o)
    index.free()


# ------------------------------------------------------------------------------------------------------------ non-finite mesh nodes
def test_hex8_locate_and_pipeline_on_a_mesh_with_nonfinite_nodes(ctx):
    pa, ca, pb, fields, affected = G.nonfinite_mesh()
    cen = O.centroid(ca, pa)
    ids = np.flatnonzero(~affected)
    k = 20
    lists = ids[O.knn_brute(np.ascontiguousarray(cen[~affected]), pb, k)]
    # the affected elements put into every list on purpose: first, in the middle and last
    rng = np.random.default_rng(7)
    for col in (0, k // 2, k - 1):
        lists[:, col] = rng.choice(np.flatnonzero(affected), len(pb))
    lists = np.ascontiguousarray(lists)
    conn = synth.reorder_hex8(ca)
    enc_o, w_o, nf_o = O.locate_hex8(lists, conn, pa, pb)
    enc, w, nf = ctx.locate_hex8(lists, conn, pa, pb)
    print(f"non-finite nodes, staged: failed {nf_o}, rows with a non-finite weight {np.isnan(w_o).any(axis=1).sum()}")
    assert nf == nf_o and np.array_equal(enc.numpy(), enc_o) and same(w.numpy(), w_o)
    # the fused pipeline: what is finite of the oracle's locate over the GPU's own lists
    for lazy in (True, False):
        ctx.set_lazy_lists(lazy)
        try:
            vals, enc, w, nf = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k, want_operator=True)
        finally:
            ctx.set_lazy_lists(True)
        enc_o, w_o, nf_o = hex8_oracle_on_gpu_lists(ctx, pa, ca, pb, k)
        with np.errstate(invalid="ignore"):
            vals_o = O.gather(fields, enc_o, w_o)
        vals, enc, w = vals.numpy(), enc.numpy(), w.numpy()
        rows = np.isfinite(w_o).all(axis=1)
        assert rows.mean() > 0.9 and nf == nf_o
        assert np.array_equal(enc[rows], enc_o[rows]) and same(w[rows], w_o[rows])
        fin = np.isfinite(vals_o)
        assert fin.mean() > 0.9 and np.array_equal(vals[fin], vals_o[fin]) and np.array_equal(np.signbit(vals[fin]), np.signbit(vals_o[fin]))
