"""Every branch the kNN and hex8 locate dispatchers pick at run time, against the oracle bit for bit.

The branches depend on the list length k (the template instances of mm_knn.hip's bucket sets, the 32- and 64-wide
reference-order group kernels), on how many targets a kernel hands over (list mode by waves up to 8192 targets, by lanes
above; long on-demand lists from 32768 on; the reference-order loop kernel from 65536 on) and on the grid (lane kernel
only on grids two cells deep or more).  Each test shows that its branch ran: the kNN kernels a call launched
(Context.last_knn_kernels), the locate stage's list lengths (Context.last_locate_stats) against what the oracle
predicts for them, a knob, or an alignment.  The scenarios and their CPU-side preconditions: tests/dispatch_cases.py,
tests/test_dispatch_cases.py.  Knobs read once per process (MM_KNN_KERNEL) run in child processes, one per knob."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dispatch_cases as D
from multimesh_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = range(1, D.KMAX + 1)


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


# ------------------------------------------------------------------------------------------------------------ kNN
def knn_sweep(ctx, ks=KS, clouds=None):
    """k = 1 .. 64 over the uniform, lattice (ties) and few-source (padding) clouds in 1, 2 and 3 dimensions: ids and
    distances bit-equal to the oracle's.  Returns {kernel: [(cloud, dim, k), ...]} of the kernels that ran."""
    ran = {}
    for kind, dim in clouds or [(c, d) for c in ("uniform", "lattice", "few") for d in (1, 2, 3)]:
        src, tgt, _ = D.knn_cloud(kind, dim)
        ref, refd = D.knn_oracle(kind, dim)
        tree = ctx.knn_build(src)
        for k in ks:
            idx, dist = tree.query(tgt, k, want_dist=True)
            kernels = ctx.last_knn_kernels()
            idx, dist = idx.numpy().reshape(len(tgt), k), dist.numpy().reshape(len(tgt), k)
            assert np.array_equal(idx, ref[:, :k]), (kind, dim, k, sorted(kernels), int((idx != ref[:, :k]).any(axis=1).sum()))
            assert np.array_equal(dist, refd[:, :k]), (kind, dim, k, sorted(kernels))
            for name in kernels:
                ran.setdefault(name, []).append((kind, dim, k))
        tree.free()
    return ran


def ks_where(ran, kernel, cloud=None):
    return {k for c, d, k in ran.get(kernel, []) if cloud is None or c == cloud}


def test_knn_every_k_default_path(ctx):
    ran = knn_sweep(ctx)
    # k > 32: the generic ring kernel (no density levels on these clouds); below, one of the tiled kernels
    assert ks_where(ran, "generic") == set(range(33, 65))
    tiled = ks_where(ran, "lane") | ks_where(ran, "strip") | ks_where(ran, "cell")
    assert tiled == set(range(1, 33))


_KNN_FORCED = r"""
import json, sys
sys.path[:0] = [".", "tests"]
from multimesh_amd.device import Context
import test_dispatch_matrix_gpu as T
ran = T.knn_sweep(Context(0))
print(json.dumps({name: sorted(set(k for _, _, k in v)) for name, v in ran.items()}))
"""


def test_knn_every_k_forced_lane_strip_and_cell_kernels():
    # MM_KNN_KERNEL is read once per process: one child per kernel, one after the other; a child that fails ends the test
    for kernel, covered in (("lane", range(1, 21)), ("strip", range(1, 33)), ("cell", range(1, 33))):
        env = dict(os.environ, MM_KNN_KERNEL=kernel)
        r = subprocess.run([sys.executable, "-c", _KNN_FORCED], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (kernel, r.returncode, r.stderr[-3000:])
        ran = {name: set(ks) for name, ks in json.loads(r.stdout.strip().splitlines()[-1]).items()}
        # the forced kernel served every k it applies to (lane: k <= 20 on grids two cells deep, the 3-D clouds) ...
        assert ran.get(kernel, set()) == set(covered), (kernel, ran)
        # ... and where it does not apply the dispatcher fell back: k > 32 the generic kernel, lane k > 20 the cell kernel
        assert ran.get("generic", set()) == set(range(33, 65))
        if kernel == "lane":
            assert set(range(21, 33)) <= ran.get("cell", set())


_KNN_SPLIT = r"""
import sys
sys.path[:0] = [".", "tests"]
import numpy as np
import dispatch_cases as D
from multimesh_amd.device import Context
ctx = Context(0)
src, tgt, ref, refd = D.split_cloud()
tree = ctx.knn_build(src)
for k in D.SPLIT_KS:
    idx, dist = tree.query(tgt, k, want_dist=True)
    assert "strip" in ctx.last_knn_kernels(), (k, sorted(ctx.last_knn_kernels()))
    idx, dist = idx.numpy().reshape(len(tgt), k), dist.numpy().reshape(len(tgt), k)
    assert np.array_equal(idx, ref[:, :k]), (k, int((idx != ref[:, :k]).any(axis=1).sum()))
    assert np.array_equal(dist, refd[:, :k]), k
print("split ok")
"""


def test_knn_strip_kernel_shares_a_strip_among_several_waves():
    # ~800 targets per strip: the launcher gives every strip nsplit ~ 6 waves (tests/test_dispatch_cases.py checks the
    # precondition); ids and distances bit-equal to the oracle, k = 8 (32 histogram buckets) and k = 25
    env = dict(os.environ, MM_KNN_KERNEL="strip")
    r = subprocess.run([sys.executable, "-c", _KNN_SPLIT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "split ok"


def test_knn_forced_list_mode_both_sides_of_8192(ctx, monkeypatch):
    monkeypatch.setenv("MM_KNN_FORCE_LIST", "1")
    ran = knn_sweep(ctx, ks=range(1, 33))
    assert ks_where(ran, "list") == set(range(1, 33)) and set(ran) == {"list"}
    for n in (5_000, 12_000):                      # one wave per target, then one lane per target
        src, tgt, ref, refd = D.list_mode_cloud(n)
        tree = ctx.knn_build(src)
        for k in range(1, 33):
            idx, dist = tree.query(tgt, k, want_dist=True)
            assert ctx.last_knn_kernels() == {"list"}
            assert np.array_equal(idx.numpy().reshape(n, k), ref[:, :k]), (n, k)
            assert np.array_equal(dist.numpy().reshape(n, k), refd[:, :k]), (n, k)


def test_knn_tree_every_k(ctx, monkeypatch):
    monkeypatch.setenv("MM_KNN_TREE", "1")
    ran = knn_sweep(ctx)
    # the tree serves 3-D clouds of at least 4096 sources for k <= 20; the rest falls back to the grid
    assert ks_where(ran, "tree", "uniform") == set(range(1, 21)) and ks_where(ran, "tree", "lattice") == set(range(1, 21))
    assert not ks_where(ran, "tree", "few")


def test_knn_graded_cloud_with_and_without_density_levels_every_k(ctx, monkeypatch):
    src, tgt, ref, refd = D.graded_cloud()
    monkeypatch.setenv("MM_KNN_TREE", "0")
    for levels, long_kernel in (("5", "levels"), ("1", "generic")):
        monkeypatch.setenv("MM_KNN_LEVELS", levels)
        tree = ctx.knn_build(src)
        for k in KS:
            idx, dist = tree.query(tgt, k, want_dist=True)
            kernels = ctx.last_knn_kernels()
            assert np.array_equal(idx.numpy().reshape(len(tgt), k), ref[:, :k]), (levels, k, sorted(kernels))
            assert np.array_equal(dist.numpy().reshape(len(tgt), k), refd[:, :k]), (levels, k)
            if k > 32:
                assert kernels == {long_kernel}, (levels, k, kernels)
        tree.free()


# ------------------------------------------------------------------------------------------------------------ hex8
def expected_stats(status, k, ncand, lazy, long_list=False):
    """What last_locate_stats must report: the first pass leaves the targets accepted in none of the candidates it saw
    (8 of a lazily evaluated list, else k); a long list's second pass leaves those accepted in none of all k."""
    k_eff = min(k, ncand)
    kq = min(D.LAZY_K, k_eff) if lazy and k > D.LAZY_K else k_eff
    first = int(D.no_accept_within(status, kq).sum())
    second = int(D.no_accept_within(status, k_eff).sum()) if long_list else 0
    return {"reference_order": first, "second_pass": second}


def check_stats(ctx, status, k, ncand, lazy, long_list=False):
    st = ctx.last_locate_stats()
    want = expected_stats(status, k, ncand, lazy, long_list)
    assert {key: st[key] for key in want} == want, (k, lazy, st, want)
    return st


def close_tol(a, b, tol):
    return np.abs(np.asarray(a) - np.asarray(b)).max(initial=0.0) <= tol


def check_pipeline(ctx, mesh, k, lazy, ncomps=(3,), tol=None, source=None, long_list=False):
    """The fused pipeline with the operator (C = ncomps[0]) and values only for every C of ncomps; bit-equal to the
    oracle (tol=None) or within MM_FP_TOL's contract; the locate stage's list lengths as the oracle predicts."""
    pa, ca, pb, fields, nn = {"sheared": D.sheared_mesh, "tiny": D.tiny_mesh, "graded": D.graded_mesh}[mesh]()
    fields = np.ascontiguousarray(np.concatenate([fields, -fields[:1] * 0.5]))        # a 4th component
    enc_o, w_o, nf_o, status = D.hex8_oracle(mesh, k)
    failed = status < 0
    ctx.set_lazy_lists(lazy)
    try:
        for i, c in enumerate(ncomps):
            f = np.ascontiguousarray(fields[:c])
            vals_o = O.gather(f, enc_o, w_o)
            if i == 0:
                if source is not None:
                    vals, enc, w, nf = source.interpolate(pb, f, nelem_to_search=k, want_operator=True)
                else:
                    vals, enc, w, nf = ctx.interpolate_hex8(pa, ca, pb, f, nelem_to_search=k, want_operator=True)
                enc, w = enc.numpy(), w.numpy()
                st = check_stats(ctx, status, k, nn.shape[1], lazy, long_list)
                assert nf == nf_o and np.array_equal(enc, enc_o), (mesh, k, lazy)
                assert not enc[failed].any() and not w[failed].any()
                if tol is None:
                    assert np.array_equal(w, w_o), (mesh, k, lazy)
                else:
                    assert close_tol(w, w_o, tol), (mesh, k, lazy, np.abs(w - w_o).max())
            else:
                vals, nf = ctx.interpolate_hex8(pa, ca, pb, f, nelem_to_search=k)
                assert nf == nf_o
            vals = vals.numpy()
            if tol is None:
                assert vals.tobytes() == np.ascontiguousarray(vals_o).tobytes(), (mesh, k, lazy, c)
            else:
                assert close_tol(vals, vals_o, tol * 8 * np.abs(f).max()), (mesh, k, lazy, c)
                assert vals[failed].tobytes() == np.ascontiguousarray(vals_o[failed]).tobytes()
    finally:
        ctx.set_lazy_lists(True)
    return st


@pytest.mark.parametrize("k", D.HEX_KS)
def test_fused_hex8_pipeline_every_k_lazy_and_eager(ctx, k):
    for lazy in (True, False):
        st = check_pipeline(ctx, "sheared", k, lazy, ncomps=(3, 1, 3, 4))
        assert st["reference_order"] > 0
        if lazy and k > 20:
            # the full lists came from the list-mode kernels (K = 40 and 64 for k > 32; up to 20 this graded index's tree)
            assert "list" in ctx.last_knn_kernels()
    for lazy in (True, False):
        check_pipeline(ctx, "tiny", k, lazy, ncomps=(3, 1))


@pytest.mark.parametrize("k", D.TOL_KS)
def test_fused_hex8_pipeline_resident_source(ctx, k):
    pa, ca, pb, fields, nn = D.sheared_mesh()
    src = ctx.source(pa, ca)
    check_pipeline(ctx, "sheared", k, True, ncomps=(3,), source=src)
    src.free()


@pytest.mark.parametrize("k", D.LONG_KS)
def test_long_on_demand_lists_and_their_second_pass(ctx, k):
    st = check_pipeline(ctx, "graded", k, True, ncomps=(1, 1), long_list=True)
    assert st["reference_order"] >= D.LONG_LIST_MIN and st["second_pass"] > 0


def test_long_on_demand_lists_second_pass_tol_against_exact(ctx, ctx_tol):
    # the second launch of the pass kernel (the rest of a long list's candidates) in MM_FP_TOL: node ids and the failed
    # count as in MM_FP_EXACT, weights and values within tests/test_fp_tol_gpu.py's bound
    k = min(D.LONG_KS)
    pa, ca, pb, fields, _ = D.graded_mesh()
    got = {}
    for mode, c in (("exact", ctx), ("tol", ctx_tol)):
        vals, enc, w, nf = c.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k, want_operator=True)
        got[mode] = (vals.numpy(), enc.numpy(), w.numpy(), nf, c.last_locate_stats())
    (vals_e, enc_e, w_e, nf_e, st_e), (vals_t, enc_t, w_t, nf_t, st_t) = got["exact"], got["tol"]
    dw, dv = np.abs(w_t - w_e).max(), np.abs(vals_t - vals_e).max()
    print(f"k = {k}: lists {st_t}, max |dw| {dw:.3e}, max |dv| {dv:.3e}, failed {nf_t}")
    assert st_t["reference_order"] >= D.LONG_LIST_MIN and st_t["second_pass"] > 0
    assert {key: st_t[key] for key in ("reference_order", "second_pass")} == {key: st_e[key] for key in ("reference_order", "second_pass")}
    assert nf_t == nf_e and np.array_equal(enc_t, enc_e)
    assert close_tol(w_t, w_e, 1e-12) and close_tol(vals_t, vals_e, 1e-12 * 8 * np.abs(fields).max())


def outside_stats_and_rows(ctx, nfar, k, tol=None):
    pa, ca, pb, fields, nn = D.outside_mesh(nfar)
    lists = []
    vals, enc, w, nf = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k, want_operator=True)   # lazy lists
    status = D.outside_oracle(nfar, k)[3]
    lists.append(check_stats(ctx, status, k, nn.shape[1], True)["reference_order"])
    outs = [(enc.numpy(), w.numpy(), nf, vals.numpy(), D.outside_oracle(nfar, k))]
    # the staged call, on lists whose nearest candidate comes last (fallbacks to the last candidate)
    status = D.outside_oracle(nfar, k, staged=True)[3]
    for conn, exodus in ((synth.reorder_hex8(ca), False), (ca, True)):
        enc, w, nf = ctx.locate_hex8(D.staged_lists(nn, k), conn, pa, pb, conn_is_exodus=exodus)
        lists.append(check_stats(ctx, status, k, nn.shape[1], False)["reference_order"])
        outs.append((enc.numpy(), w.numpy(), nf, None, D.outside_oracle(nfar, k, staged=True)))
    for enc, w, nf, vals, (enc_o, w_o, nf_o, status) in outs:
        failed = status < 0
        vals_o = O.gather(fields, enc_o, w_o)
        assert nf == nf_o and np.array_equal(enc, enc_o)
        assert not enc[failed].any() and not w[failed].any()
        if tol is None:
            assert np.array_equal(w, w_o)
        else:
            assert close_tol(w, w_o, tol)
        if vals is not None:
            if tol is None:
                assert vals.tobytes() == np.ascontiguousarray(vals_o).tobytes()
            else:
                assert close_tol(vals, vals_o, tol * 8 * np.abs(fields).max())
                assert vals[failed].tobytes() == np.ascontiguousarray(vals_o[failed]).tobytes()
    return lists


@pytest.mark.parametrize("nfar,k", D.OUTSIDE_CASES)
def test_reference_order_kernel_every_instance(ctx, nfar, k):
    # lists below 65536: locate_hex8_group_kernel, 32 lanes per target (k <= 32) or 64; from 65536 on: the loop kernel
    lists = outside_stats_and_rows(ctx, nfar, k)
    if nfar == D.OUTSIDE_SMALL:
        assert all(0 < n < D.GROUP_LIST_MAX for n in lists), lists
    else:
        assert all(n >= 70_000 for n in lists), lists


# ------------------------------------------------------------------------------------------------------------ MM_FP_TOL
@pytest.mark.parametrize("k", D.TOL_KS)
def test_fp_tol_over_k(ctx_tol, k):
    pa, ca = D.sheared_mesh()[:2]
    check_pipeline(ctx_tol, "sheared", k, True, ncomps=(3, 1), tol=D.fp_tol(pa, ca))
    pa, ca = D.graded_mesh()[:2]
    st = check_pipeline(ctx_tol, "graded", k, True, ncomps=(1,), tol=D.fp_tol(pa, ca), long_list=True)
    assert st["second_pass"] > 0
    pa, ca = D.outside_mesh(D.OUTSIDE_SMALL)[:2]
    for nfar in (D.OUTSIDE_SMALL, D.OUTSIDE_LARGE):
        if (nfar, k) in D.OUTSIDE_CASES:
            outside_stats_and_rows(ctx_tol, nfar, k, tol=D.fp_tol(pa, ca))


# ------------------------------------------------------------------------------------------------------------ GLL
@pytest.mark.parametrize("order,dim", [(o, d) for o in (1, 2, 4) for d in (2, 3)])
def test_gll_fused_pipeline_every_k(ctx, order, dim):
    gp, pts, fields, nn = D.gll_case(order, dim)
    for k in D.GLL_KS:
        for tol, snap in ((1.05, False), (1.05, True)):
            elem_o, co_o, miss_o = O.locate_gll(order, nn[:, :k], gp, pts, tolerance=tol, snap_to_nearest=snap)
            vals_o = O.gather_elem(fields, elem_o, co_o)
            beyond8 = int(((elem_o[:, None] != nn[:, :8]).all(axis=1) & (elem_o >= 0)).sum())
            assert snap or miss_o > 0
            assert k < 25 or beyond8 > 0                  # the lazily fetched full lists are needed
            for lazy in (True, False):
                ctx.set_lazy_lists(lazy)
                try:
                    vals, miss = ctx.interpolate_gll(order, gp, pts, fields, nelem_to_search=k, tolerance=tol,
                                                     snap_to_nearest=snap)
                    v2, elem, co, miss2 = ctx.interpolate_gll(order, gp, pts, fields, nelem_to_search=k, tolerance=tol,
                                                              snap_to_nearest=snap, want_operator=True)
                finally:
                    ctx.set_lazy_lists(True)
                assert miss == miss_o == miss2, (k, lazy, snap)
                assert vals.numpy().tobytes() == vals_o.tobytes() and v2.numpy().tobytes() == vals_o.tobytes(), (k, lazy, snap)
                assert np.array_equal(elem.numpy(), elem_o) and np.array_equal(co.numpy(), co_o), (k, lazy, snap)


# ------------------------------------------------------------------------------------------------------------ gather
def test_gather_every_p_both_layouts(ctx):
    for P in range(1, 129):
        for ncomp in (1, 3):
            fields, ids, w = D.gather_case(P, ncomp)
            ref = np.ascontiguousarray(O.gather_numpy(fields, ids, w))
            d_ids, d_w = ctx.to_device(ids), ctx.to_device(w)
            assert d_ids.ptr % 16 == 0 and d_w.ptr % 16 == 0        # P = 8: the 16-byte-aligned kernel
            out = ctx.gather(fields, d_ids, d_w).numpy()
            assert out.tobytes() == ref.tobytes(), (P, ncomp)
            out = ctx.gather(fields, d_ids, d_w, point_major=False).numpy()
            assert out.tobytes() == np.ascontiguousarray(ref.T).tobytes(), (P, ncomp)


def test_gather_p8_rows_eight_bytes_into_an_allocation(ctx):
    # ids or weights 8 bytes past a 16-byte boundary: mm_launch_gather takes the general kernel for P = 8
    from multimesh_amd.device import DeviceArray

    def shifted(a):
        buf = ctx.to_device(np.concatenate([np.zeros(1, a.dtype), a.ravel()]))
        assert buf.ptr % 16 == 0
        return DeviceArray(ctx, buf.ptr + 8, a.shape, a.dtype, owner=False, keepalive=buf)

    for ncomp in (1, 3):
        fields, ids, w = D.gather_case(8, ncomp, seed=1)
        ref = np.ascontiguousarray(O.gather_numpy(fields, ids, w))
        for d_ids, d_w in ((shifted(ids), shifted(w)), (shifted(ids), ctx.to_device(w)), (ctx.to_device(ids), shifted(w))):
            assert d_ids.ptr % 16 == 8 or d_w.ptr % 16 == 8
            assert ctx.gather(fields, d_ids, d_w).numpy().tobytes() == ref.tobytes()
            out = ctx.gather(fields, d_ids, d_w, point_major=False).numpy()
            assert out.tobytes() == np.ascontiguousarray(ref.T).tobytes()
