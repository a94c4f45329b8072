"""The one-pass source sort of a guessed mm_interpolate_hex8 call (mm_knn_build_one_pass: the centroid kernel places every
record at cell_start[cell] + rank by the PREVIOUS call's cell_start, a check kernel compares the per-cell counts
afterwards): a hit, a hit with the elements in another order, a miss by the counts alone, a miss by the box with the
elements crowded into a few cells, the calls after a miss, and a call behind another user of the context's buffers.
Every result is compared bit for bit with a fresh context in a process run under MM_GRID_GUESS=0 (the switch is read
once per process).  Which path a call took: Context.last_knn_kernels() carries "one_pass", mm_debug_grid_guess counts
the guessed calls and the misses.

A call that misses is run again the ordinary way inside the same call, as with a wrong box: that rerun is "the
ordinary call over the new mesh", and the call after it is one-pass again."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from multimesh_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_FRESH = (
    "import sys, numpy as np\n"
    "from multimesh_amd.device import Context\n"
    "d = np.load(sys.argv[1])\n"
    "out = {}\n"
    "for name in [str(s) for s in d['cases']]:\n"
    "    c = Context(0)\n"
    "    v, enc, w, nf = c.interpolate_hex8(d[name + '_nodes'], d[name + '_conn'], d[name + '_pts'], d[name + '_fields'],\n"
    "                                       nelem_to_search=20, want_operator=True)\n"
    "    assert c.last_knn_kernels().isdisjoint({'one_pass'})\n"
    "    out[name + '_v'], out[name + '_enc'], out[name + '_w'] = v.numpy(), enc.numpy(), w.numpy()\n"
    "    out[name + '_nf'] = np.int64(nf)\n"
    "    c.close()\n"
    "np.savez(sys.argv[2], **out)\n"
    "print('ok')\n"
)


def _fresh_unguessed(tmp_path, cases):
    """cases: {name: (nodes, conn, pts, fields)} -> {name: (values, enc, w, nfailed)} from fresh contexts of a process
    started with MM_GRID_GUESS=0."""
    arrays = {"cases": np.array(sorted(cases))}
    for name, (nodes, conn, pts, fields) in cases.items():
        arrays[name + "_nodes"], arrays[name + "_conn"] = nodes, conn
        arrays[name + "_pts"], arrays[name + "_fields"] = pts, fields
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **arrays)
    r = subprocess.run([sys.executable, "-c", _FRESH, src, dst], env=dict(os.environ, MM_GRID_GUESS="0"),
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
    o = np.load(dst)
    return {name: (o[name + "_v"], o[name + "_enc"], o[name + "_w"], int(o[name + "_nf"])) for name in cases}


def _guess_state(ctx):
    out = (C.c_longlong * 4)()
    fn = ctx.lib.mm_debug_grid_guess
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    assert fn(ctx.handle, out) == 0
    return {"valid": out[0], "misses": out[1], "guessed": out[2], "nsrc": out[3]}


def _run(ctx, case):
    """-> ((values, enc, w, nfailed), the call's last run was one-pass)"""
    v, enc, w, nf = ctx.interpolate_hex8(*case, nelem_to_search=20, want_operator=True)
    return (v.numpy(), enc.numpy(), w.numpy(), nf), "one_pass" in ctx.last_knn_kernels()


def _same(a, b):
    return a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


# ---- the grid's own arithmetic on the CPU (grid_layout, cell_of_point; centroid.c:17-22 for the centroids) ----------
def _centroids(nodes, conn):
    acc = np.zeros((len(conn), 3))
    for p in range(8):
        acc = acc + nodes[conn[:, p]]     # connectivity order, from 0.0
    return acc / 8.0


def _grid(cen):
    lo, hi = cen.min(axis=0), cen.max(axis=0)
    ext = hi - lo
    edge = math.pow(float(np.prod(ext)) / (len(cen) / 8.0), 1.0 / 3.0)
    dims = np.minimum(np.maximum(np.ceil(ext / edge), 1), 1024).astype(np.int64)
    inv_h = 1.0 / (ext / dims)
    return lo, hi, dims, inv_h


def _cells(cen, lo, dims, inv_h):
    t = np.minimum(np.maximum((cen - lo) * inv_h, 0.0), (dims - 1).astype(np.float64)).astype(np.int64)
    return (t[:, 0] * dims[1] + t[:, 1]) * dims[2] + t[:, 2]


def _one_centroid_across_a_face(nodes, conn):
    """A copy of `nodes` with ONE interior node moved along x so that exactly one centroid changes its cell and the box
    of the centroids stays what it was (searched for; every property is asserted by the caller)."""
    cen = _centroids(nodes, conn)
    lo, hi, dims, inv_h = _grid(cen)
    cells = _cells(cen, lo, dims, inv_h)
    h = 1.0 / inv_h[0]
    n_side = round(len(nodes) ** (1.0 / 3.0))
    spacing = 1.0 / (n_side - 1)
    tx = (cen[:, 0] - lo[0]) * inv_h[0]
    room = (np.floor(tx) + 1.0 - tx) * h          # distance of each centroid to its cell's upper x face
    idx = np.arange(len(nodes))
    i, j, k = idx // (n_side * n_side), (idx // n_side) % n_side, idx % n_side
    interior = (np.minimum(np.minimum(i, j), k) >= 3) & (np.maximum(np.maximum(i, j), k) <= n_side - 4)
    for e in np.argsort(room)[:200]:
        delta = 8.0 * room[e] * 1.5 + 1e-9
        if delta > 0.1 * spacing:
            break
        for node in conn[e]:
            if not interior[node]:
                continue
            moved = nodes.copy()
            moved[node, 0] += delta
            cen2 = _centroids(moved, conn)
            changed = np.flatnonzero(_cells(cen2, lo, dims, inv_h) != cells)
            if len(changed) == 1 and np.array_equal(cen2.min(axis=0), lo) and np.array_equal(cen2.max(axis=0), hi):
                return moved
    raise AssertionError("no interior node moves exactly one centroid across a cell face")


def _mesh_case(n, seed, npts, ncomp=1, jitter=0.3):
    nodes, conn = synth.hex_mesh(n, seed=seed, jitter=jitter)
    pts = np.random.default_rng(seed + 100).uniform(0.02, 0.98, size=(npts, 3))
    return nodes, conn, pts, synth.vector_field(nodes)[:ncomp]


@pytest.mark.timeout(900)
def test_hit_three_calls_and_permuted_elements(tmp_path):
    """A small mesh and one of 1 M elements (many waves contend for every cell's cursor).  Calls two and three over one
    mesh are one-pass and confirmed; the same mesh with the rows of conn permuted has the same per-cell counts, so
    it confirms too (and is compared with a fresh context over the permuted rows: the ids of a tie follow them)."""
    from multimesh_amd.device import Context

    cases = {}
    for name, n, npts in (("small", 30, 40_000), ("big", 101, 200_000)):
        nodes, conn, pts, fields = _mesh_case(n, 1, npts, ncomp=2)
        cases[name] = (nodes, conn, pts, fields)
        perm = np.random.default_rng(11).permutation(len(conn))
        cases[name + "_perm"] = (nodes, np.ascontiguousarray(conn[perm]), pts, fields)
    ref = _fresh_unguessed(tmp_path, cases)
    for name in ("small", "big"):
        c = Context(0)
        try:
            got, one = _run(c, cases[name])
            assert _same(got, ref[name]) and not one
            for call in (1, 2):
                got, one = _run(c, cases[name])
                assert one and _same(got, ref[name]), (name, call)
                s = _guess_state(c)
                assert s["guessed"] == call and s["misses"] == 0 and s["valid"] == 1
            got, one = _run(c, cases[name + "_perm"])
            assert one and _same(got, ref[name + "_perm"]), name
            s = _guess_state(c)
            assert s["guessed"] == 3 and s["misses"] == 0
            got, one = _run(c, cases[name])        # ... and back
            assert one and _same(got, ref[name]) and _guess_state(c)["misses"] == 0
        finally:
            c.close()


@pytest.mark.timeout(600)
def test_counts_only_miss_and_the_calls_after_it(tmp_path):
    """Same element count, same box of the centroids, one centroid in another cell: only the count check can tell.  The
    call is run again (misses + 1) and is right; the call after it is one-pass over the new mesh."""
    from multimesh_amd.device import Context

    nodes, conn, pts, fields = _mesh_case(30, 3, 30_000)
    moved = _one_centroid_across_a_face(nodes, conn)
    # the premise, in the grid's own arithmetic: one node differs, the box is the same, exactly one centroid changed cell
    assert (moved != nodes).any(axis=1).sum() == 1
    cen, cen2 = _centroids(nodes, conn), _centroids(moved, conn)
    lo, hi, dims, inv_h = _grid(cen)
    lo2, hi2, dims2, inv_h2 = _grid(cen2)
    assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2) and np.array_equal(dims, dims2) and np.array_equal(inv_h, inv_h2)
    assert (_cells(cen, lo, dims, inv_h) != _cells(cen2, lo, dims, inv_h)).sum() == 1
    cases = {"a": (nodes, conn, pts, fields), "b": (moved, conn, pts, synth.vector_field(moved)[:1])}
    ref = _fresh_unguessed(tmp_path, cases)
    c = Context(0)
    try:
        assert _same(_run(c, cases["a"])[0], ref["a"])
        got, one = _run(c, cases["a"])
        assert one and _same(got, ref["a"])
        got, one = _run(c, cases["b"])             # box equal, counts not: rerun the ordinary way
        s = _guess_state(c)
        assert _same(got, ref["b"]) and not one
        assert s["guessed"] == 2 and s["misses"] == 1 and s["valid"] == 1
        got, one = _run(c, cases["b"])             # the rerun left mesh b's sort: one pass again
        assert one and _same(got, ref["b"])
        s = _guess_state(c)
        assert s["guessed"] == 3 and s["misses"] == 1
    finally:
        c.close()


@pytest.mark.timeout(600)
def test_box_miss_with_crowded_cells(tmp_path):
    """Another mesh of the same element count, shrunk into a corner of the first one's box: on the guessed grid all its
    centroids fall into a few cells with room for a handful of records each, so nearly every record finds no room and is
    dropped (every store of centroid_sort_kernel is guarded by the cell's room and by [0, nelem)).  The call is run
    again and returns what a fresh context returns."""
    from multimesh_amd.device import Context

    nodes, conn, pts, fields = _mesh_case(40, 5, 30_000)
    nodes2 = np.ascontiguousarray(0.01 + 0.03 * nodes)
    pts2 = np.ascontiguousarray(0.01 + 0.03 * pts)
    cases = {"a": (nodes, conn, pts, fields), "b": (nodes2, conn, pts2, synth.vector_field(nodes2)[:1])}
    ref = _fresh_unguessed(tmp_path, cases)
    c = Context(0)
    try:
        assert _same(_run(c, cases["a"])[0], ref["a"])
        got, one = _run(c, cases["a"])
        assert one and _same(got, ref["a"])
        got, one = _run(c, cases["b"])
        assert _same(got, ref["b"]) and not one
        s = _guess_state(c)
        assert s["guessed"] == 2 and s["misses"] == 1
        got, one = _run(c, cases["b"])
        assert one and _same(got, ref["b"])
        got, one = _run(c, cases["a"])             # second miss: this context stops guessing, and stays right
        assert _same(got, ref["a"]) and not one and _guess_state(c)["misses"] == 2
        got, one = _run(c, cases["a"])
        assert _same(got, ref["a"]) and not one and _guess_state(c)["guessed"] == 4
    finally:
        c.close()


@pytest.mark.timeout(600)
def test_another_build_in_the_context_buffers_switches_one_pass_off(tmp_path):
    """The GLL pipeline sorts ITS centroids into the same context buffers: the hex8 call behind it still guesses the
    grid from the box but may not place records by that cell_start (two-pass guessed build), and the call after that is
    one-pass again."""
    from multimesh_amd.device import Context

    case = _mesh_case(30, 7, 20_000)
    ref = _fresh_unguessed(tmp_path, {"a": case})["a"]
    gll = synth.gll_mesh(12, 2, seed=3)
    gll_fields = np.ascontiguousarray(gll[None, :, :, 0])
    gll_pts = np.random.default_rng(9).uniform(0.1, 0.9, size=(2000, 3))
    c = Context(0)
    try:
        assert _same(_run(c, case)[0], ref)
        got, one = _run(c, case)
        assert one and _same(got, ref)
        c.interpolate_gll(2, gll, gll_pts, gll_fields)
        got, one = _run(c, case)
        s = _guess_state(c)
        assert _same(got, ref) and not one and s["guessed"] == 2 and s["misses"] == 0
        got, one = _run(c, case)
        assert one and _same(got, ref) and _guess_state(c)["misses"] == 0
    finally:
        c.close()
