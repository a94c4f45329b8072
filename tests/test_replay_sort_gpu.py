"""The replayed target sort of mm_interpolate_hex8 (mm_context::target_replay, target_replay_kernel): a fused call keeps
every target's position in the cell-sorted order, the targets' cell starts and the lane kernel's work items; the next
call over as many targets on the same grid stores its records at those positions and checks, target by target, that the
position lies in the range of the cell the target is in NOW.  One target outside it: the call is run again with an
ordinary sort (a miss like a wrong box: mm_debug_grid_guess counts it; that rerun is "the ordinary call", it records,
and the call after it replays again).

Every result is compared bit for bit with a fresh context's on the same inputs.  Which path ran:
Context.last_knn_kernels() carries "target_replay" (then no count, scan, scatter or work-list kernel was launched for
the targets: the replay branch launches one kernel in their place), mm_debug_target_replay counts replays, recorded
sorts and the work lists built for them (the three lane_items_* kernels: a replay builds none).

The source side has no replay: it was built, measured slower than the atomic one-pass build and taken out (DESIGN.md
section 9), so there is no source-side case here; tests/test_one_pass_build_gpu.py covers the source sort as it is.

Shapes: 24 nodes per side (12 167 elements, 13 824 targets) is the smallest jittered mesh at which the fused pipeline
takes the lane kernel over a single-level grid (asserted below); one case at 1 M -> 1 M."""
import ctypes as C
import math

import numpy as np
import pytest

from multimesh_amd import synth

pytestmark = pytest.mark.gpu

N = 24


def _debug(ctx, symbol):
    out = (C.c_longlong * 8)()
    fn = getattr(ctx.lib, symbol)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    assert fn(ctx.handle, out) == 0
    return list(out)


def _state(ctx):
    g, t = _debug(ctx, "mm_debug_grid_guess"), _debug(ctx, "mm_debug_target_replay")
    return {"misses": g[1], "guessed": g[2], "held": t[0], "replays": t[1], "records": t[2], "npts": t[3]}


def _work_lists(ctx):
    """Dispatch-visible counter: lane work lists (the three lane_items_* kernels) built for kept sorts."""
    return _debug(ctx, "mm_debug_target_replay")[4]


def _run(ctx, case):
    """-> ((values, enc, w, nfailed), the kNN kernels of the call's last run)"""
    v, enc, w, nf = ctx.interpolate_hex8(*case, nelem_to_search=20, want_operator=True)
    return (v.numpy(), enc.numpy(), w.numpy(), nf), ctx.last_knn_kernels()


def _fresh(case):
    from multimesh_amd.device import Context

    with Context(0) as c:
        out, kernels = _run(c, case)
        assert "target_replay" not in kernels and "lane" in kernels and "tree" not in kernels, kernels
        return out


def _same(a, b):
    return a[3] == b[3] and all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))   # (bytes: NaN rows compare too)


def _case(n=N, seed=1):
    nodes, conn = synth.hex_mesh(n, seed=seed, jitter=0.3)
    pts, _ = synth.hex_mesh(n, seed=seed + 6, jitter=0.2)
    return nodes, conn, np.ascontiguousarray(0.01 + 0.98 * pts), synth.vector_field(nodes)[:1]


# ---- the grid's own arithmetic on the CPU (grid_layout, cell_of_point; centroid.c:17-22 for the centroids) ----------
def _grid(nodes, conn):
    cen = np.zeros((len(conn), 3))
    for p in range(8):
        cen = cen + nodes[conn[:, p]]
    cen = cen / 8.0
    lo, hi = cen.min(axis=0), cen.max(axis=0)
    ext = hi - lo
    edge = math.pow(float(np.prod(ext)) / (len(cen) / 8.0), 1.0 / 3.0)
    dims = np.minimum(np.maximum(np.ceil(ext / edge), 1), 1024).astype(np.int64)
    return lo, dims, 1.0 / (ext / dims)


def _cells(pts, lo, dims, inv_h):
    t = np.minimum(np.maximum((pts - lo) * inv_h, 0.0), (dims - 1).astype(np.float64)).astype(np.int64)
    return (t[:, 0] * dims[1] + t[:, 1]) * dims[2] + t[:, 2]


def _with_pts(case, pts):
    return case[0], case[1], np.ascontiguousarray(pts), case[3]


def _warm(c, case, ref):
    """Two calls: ordinary (records), then guessed with both sorts replayed."""
    got, kernels = _run(c, case)
    assert _same(got, ref) and "target_replay" not in kernels and "lane" in kernels, kernels
    got, kernels = _run(c, case)
    assert _same(got, ref) and {"target_replay", "one_pass", "lane"} <= kernels, kernels


@pytest.mark.parametrize("n", [N, 101])
def test_hit_three_identical_calls(n):
    from multimesh_amd.device import Context

    case = _case(n)
    ref = _fresh(case)
    with Context(0) as c:
        _warm(c, case, ref)
        got, kernels = _run(c, case)
        assert _same(got, ref) and {"target_replay", "one_pass", "lane"} <= kernels, kernels
        s = _state(c)
        assert s == {"misses": 0, "guessed": 2, "held": 1, "replays": 2, "records": 1, "npts": len(case[2])}
        # calls 2 and 3 replayed the target sort; the one work list is the first call's: call 3 launched no count, scan,
        # scatter or work-list kernel for the targets
        assert _work_lists(c) == 1


def _swapped(case):
    """Rows i and j of the targets exchanged, the two in different cells: every per-cell count is what it was."""
    lo, dims, inv_h = _grid(case[0], case[1])
    cells = _cells(case[2], lo, dims, inv_h)
    i = len(cells) // 3
    j = int(np.flatnonzero(cells != cells[i])[-1])
    pts = case[2].copy()
    pts[[i, j]] = pts[[j, i]]
    assert np.array_equal(np.bincount(_cells(pts, lo, dims, inv_h), minlength=int(dims.prod())),
                          np.bincount(cells, minlength=int(dims.prod())))
    return _with_pts(case, pts)


def _moved(case):
    """One target one cell further along x (the grid is the source's: the box does not change)."""
    lo, dims, inv_h = _grid(case[0], case[1])
    cells = _cells(case[2], lo, dims, inv_h)
    cx = np.floor((case[2][:, 0] - lo[0]) * inv_h[0])
    i = int(np.flatnonzero((cx >= 1) & (cx < dims[0] - 2))[7])
    pts = case[2].copy()
    pts[i, 0] += 1.0 / inv_h[0]
    moved = _cells(pts, lo, dims, inv_h)
    assert (moved != cells).sum() == 1 and 0.0 < pts[i, 0] < 1.0
    return _with_pts(case, pts)


def _permuted(case):
    return _with_pts(case, case[2][np.random.default_rng(3).permutation(len(case[2]))])


@pytest.mark.parametrize("change", [_swapped, _moved, _permuted])
def test_miss_is_run_again_and_the_next_call_replays(change):
    from multimesh_amd.device import Context

    case = _case()
    other = change(case)
    ref, ref_other = _fresh(case), _fresh(other)
    with Context(0) as c:
        _warm(c, case, ref)
        got, kernels = _run(c, other)          # the containment check misses: run again with an ordinary sort
        s = _state(c)
        assert _same(got, ref_other) and "target_replay" not in kernels and "one_pass" not in kernels, kernels
        assert s["misses"] == 1 and s["replays"] == 2 and s["records"] == 2 and s["held"] == 1, s
        got, kernels = _run(c, other)          # the rerun recorded the new positions: replayed
        s = _state(c)
        assert _same(got, ref_other) and {"target_replay", "one_pass"} <= kernels, kernels
        assert s["misses"] == 1 and s["replays"] == 3 and s["records"] == 2, s
        got, kernels = _run(c, case)           # second miss: this context stops guessing, and stays right
        s = _state(c)
        assert _same(got, ref) and "target_replay" not in kernels and s["misses"] == 2 and s["replays"] == 4, s
        got, kernels = _run(c, case)
        assert _same(got, ref) and kernels.isdisjoint({"target_replay", "one_pass"}), kernels
        assert _state(c)["replays"] == 4 and _state(c)["guessed"] == s["guessed"]


def test_another_target_count_is_not_a_miss():
    from multimesh_amd.device import Context

    case = _case()
    fewer = _with_pts(case, case[2][:-5])
    ref, ref_fewer = _fresh(case), _fresh(fewer)
    with Context(0) as c:
        _warm(c, case, ref)
        got, kernels = _run(c, fewer)
        s = _state(c)
        assert _same(got, ref_fewer) and "target_replay" not in kernels and "one_pass" in kernels, kernels
        assert s["misses"] == 0 and s["replays"] == 1 and s["records"] == 2 and s["npts"] == len(fewer[2]), s
        got, kernels = _run(c, fewer)
        assert _same(got, ref_fewer) and "target_replay" in kernels and _state(c)["misses"] == 0


def test_gll_and_tree_calls_in_between(monkeypatch):
    """The GLL pipeline leaves the kept target sort alone (it sorts into buffers of its own) and takes the source
    buffers: the hex8 call behind it is right.  A fused call through the kNN tree (MM_KNN_TREE=1 is read by the ordinary
    build: a source mesh of another size, so that the call is not guessed) writes its own order of the targets into the
    sorted-record buffer: the kept sort is dropped, the next call sorts the ordinary way, the one after replays."""
    from multimesh_amd.device import Context

    case, tree_case = _case(), _case(20, seed=2)
    ref = _fresh(case)
    gll = synth.gll_mesh(12, 2, seed=3)
    gll_fields = np.ascontiguousarray(gll[None, :, :, 0])
    gll_pts = np.random.default_rng(9).uniform(0.1, 0.9, size=(2000, 3))
    monkeypatch.setenv("MM_KNN_TREE", "1")
    with Context(0) as c:
        ref_tree, kernels = _run(c, tree_case)
        assert "tree" in kernels, kernels
    monkeypatch.delenv("MM_KNN_TREE")
    with Context(0) as c:
        _warm(c, case, ref)
        c.interpolate_gll(2, gll, gll_pts, gll_fields)
        got, kernels = _run(c, case)
        # (the GLL path sorts into the source buffers -- no one-pass build behind it -- and takes none of the kept target sort's)
        assert _same(got, ref) and "one_pass" not in kernels and "target_replay" in kernels, kernels
        assert _state(c)["misses"] == 0 and _state(c)["records"] == 1 and _state(c)["replays"] == 2
        got, kernels = _run(c, case)
        assert _same(got, ref) and {"target_replay", "one_pass"} <= kernels, kernels
        monkeypatch.setenv("MM_KNN_TREE", "1")
        got, kernels = _run(c, tree_case)
        assert _same(got, ref_tree) and "tree" in kernels and "target_replay" not in kernels and _state(c)["held"] == 0, kernels
        monkeypatch.delenv("MM_KNN_TREE")
        records = _state(c)["records"]
        got, kernels = _run(c, case)
        s = _state(c)
        assert _same(got, ref) and "target_replay" not in kernels and s["records"] == records + 1 and s["held"] == 1, (kernels, s)
        got, kernels = _run(c, case)
        assert _same(got, ref) and "target_replay" in kernels and _state(c)["misses"] == 0, kernels


def test_non_finite_target_in_both_calls():
    from multimesh_amd.device import Context

    case = _case()
    pts = case[2].copy()
    pts[1234] = np.nan
    case = _with_pts(case, pts)
    ref = _fresh(case)
    with Context(0) as c:
        _warm(c, case, ref)
        assert _state(c)["misses"] == 0


def test_resident_source():
    from multimesh_amd.device import Context

    case = _case()
    other = _swapped(case)
    ref, ref_other = _fresh(case), _fresh(other)
    with Context(0) as c:
        src = c.source(case[0], case[1])

        def run(k):
            out = src.interpolate(k[2], k[3], nelem_to_search=20, want_operator=True)
            return (out[0].numpy(), out[1].numpy(), out[2].numpy(), out[3]), c.last_knn_kernels()

        got, kernels = run(case)
        assert _same(got, ref) and "target_replay" not in kernels and "lane" in kernels, kernels
        got, kernels = run(case)
        assert _same(got, ref) and "target_replay" in kernels and _state(c)["replays"] == 1, kernels
        got, kernels = run(other)              # a miss: run again with an ordinary sort
        s = _state(c)
        assert _same(got, ref_other) and "target_replay" not in kernels and s["misses"] == 1 and s["replays"] == 2, (kernels, s)
        got, kernels = run(other)
        assert _same(got, ref_other) and "target_replay" in kernels and _state(c)["misses"] == 1, kernels
        src.free()
