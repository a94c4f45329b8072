"""knn_lane_kernel at the smallest shapes that reach it: rows against the oracle on ids (ties by id) and on distances bit
for bit (tests/dispatch_cases.knn_distances).  The kernel's exact-distance phase fetches the records of its K + 1 candidates
in chunks of five, all of a chunk in flight at once; the cases cover both list lengths (K = 8: chunks of 5 + 4, rows in
registers; K = 20: 5 + 5 + 5 + 5 + 1, rows through LDS), rounds after a widened retry, lists that end in sentinel keys (the
record position clamped to 0), tiles that overflow, hull targets, duplicated sources and the fused pipeline's sorted rows.

These are bit-identity checks: they hold the rows where they were and would pass before the loads were grouped as well.

MM_KNN_KERNEL and the other knobs are read once per process: every case runs in a child process forced to the lane kernel,
with one grid level (MM_KNN_LEVELS=1: the lane kernel serves single-level indexes only, and a strip too full for the tile is
then handed to the list kernel through fb_list), and asserts which kernels ran.  The library reports no hand-over counts:
that targets were handed over is asserted by the list kernel having run, and that the shape asks for it by laying the grid
out on the CPU the way grid_layout does and counting the tiles' entries."""
import os
import subprocess
import sys

import pytest

_PRELUDE = r"""
import sys
import numpy as np
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from dispatch_cases import knn_distances
from multimesh_amd import synth
from multimesh_amd.device import Context
from oracle import oracle as O
ctx = Context(0)
TILE_CAP, PAD, Z = 768, 16, 7        # kLaneTileCap, kLanePad, kLaneZ

def check(src, q, k, brute=False):
    idx, dist = ctx.knn_build(src).query(q, k, want_dist=True)
    ran = ctx.last_knn_kernels()
    assert "lane" in ran, sorted(ran)
    ref = O.knn_brute(src, q, k) if brute else O.knn_ckdtree(src, q, k, workers=-1)[0]
    got = idx.numpy()
    assert np.array_equal(got, ref), (k, int((got != ref).any(axis=1).sum()))
    assert np.array_equal(dist.numpy(), knn_distances(src, q, ref)), k
    return ran

def tiles(src, q):
    # the tiles of the strips that hold targets: (entries, entries of the tile's top cell layer), on the grid of ~8 sources
    # per cubic cell over the sources' box
    lo, ext = src.min(axis=0), src.max(axis=0) - src.min(axis=0)
    edge = (ext.prod() / max(len(src) / 8.0, 1.0)) ** (1.0 / 3.0)
    dims = np.maximum(np.ceil(ext / edge), 1).astype(int)
    cell = lambda p: np.clip(np.floor((p - lo) / (ext / dims)).astype(int), 0, dims - 1)
    cnt = np.zeros(tuple(dims + np.array([2, 2, 0])), dtype=np.int64)
    cs = cell(src)
    np.add.at(cnt, (cs[:, 0] + 1, cs[:, 1] + 1, cs[:, 2]), 1)
    col9 = sum(cnt[1 + a:dims[0] + 1 + a, 1 + b:dims[1] + 1 + b] for a in (-1, 0, 1) for b in (-1, 0, 1))
    cq = cell(q)
    out = set()
    for cx, cy, s in set(zip(cq[:, 0], cq[:, 1], cq[:, 2] // Z)):
        za, zb = max(s * Z - 1, 0), min(min(s * Z + Z, dims[2]), dims[2] - 1)
        out.add((int(col9[cx, cy, za:zb + 1].sum()), int(col9[cx, cy, zb])))
    return out

pa, ca = synth.hex_mesh(21, seed=1)          # 20^3 elements
cen = O.centroid(ca, pa)
rng = np.random.default_rng(5)
"""

_CASES = {
    # 20^3 source centroids; the 20^3 jittered nodes of another mesh and 3,000 uniform random points
    "smallest": ({}, r"""
pb, _ = synth.hex_mesh(20, seed=7)
for k in (8, 20):
    check(cen, pb, k)
    check(cen, rng.uniform(size=(3000, 3)), k)
"""),
    # windows of one thin layer either way: nearly every round of the short lists is widened, and the exact phase runs a
    # second time over keys whose slots lie behind and before the first scan
    "widened": ({"MM_KNN_LANE_W": "1"}, r"""
pb, _ = synth.hex_mesh(20, seed=7)
check(cen, pb, 8)
check(cen, rng.uniform(size=(3000, 3)), 8)
"""),
    # partly filled staging trips: a uniform cloud under a thin sprinkle of sources, so that the tiles' lengths are no
    # multiples of 64 and the top cell layer of the upper tiles holds fewer than kLanePad entries (the tile ends within
    # the padding's reach of that layer's start); targets up there see fewer than K + 2 sources: sentinel keys
    "partial_trips": ({}, r"""
src = np.concatenate([rng.uniform(size=(6000, 3)), rng.uniform(size=(30, 3)) * [1, 1, 0.12] + [0, 0, 1.0]])
q = np.concatenate([rng.uniform(size=(6000, 3)), rng.uniform(size=(600, 3)) * [1, 1, 0.12] + [0, 0, 1.0]])
t = tiles(src, q)
assert any(0 < n <= TILE_CAP and n % 64 for n, _ in t), sorted(t)[:8]
assert any(0 < n <= TILE_CAP and top < PAD for n, top in t), sorted(t)[:8]
for k in (8, 20):
    ran = check(src, q, k)
    assert "list" in ran, sorted(ran)     # (the sparse top: too few sources in a window)
"""),
    # a clustered cloud: the strips through the cluster overflow kLaneTileCap and are handed over whole, through fb_list
    "overflow": ({}, r"""
cloud = np.concatenate([rng.uniform(size=(8000, 3)), 0.5 + 0.004 * rng.standard_normal((6000, 3))])
q = np.concatenate([rng.uniform(size=(4000, 3)), 0.5 + 0.004 * rng.standard_normal((2000, 3))])
t = tiles(cloud, q)
assert any(n > TILE_CAP for n, _ in t) and any(0 < n <= TILE_CAP for n, _ in t), sorted(t)[-4:]
for k in (8, 20):
    ran = check(cloud, q, k)
    assert "list" in ran, sorted(ran)
"""),
    # targets on the hull (the certificate fails: hand-over to the list kernel) and exactly duplicated sources
    # (bit-equal distances, ranked by id: the brute-force oracle)
    "hull_and_duplicates": ({}, r"""
dup = np.concatenate([cen, cen[::3]])
corners = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
lo, hi = cen.min(axis=0), cen.max(axis=0)
q = np.concatenate([lo + (hi - lo) * corners, corners, pa[::2], cen[::7]])
for k in (8, 20):
    ran = check(dup, q, k, brute=True)
    assert "list" in ran, sorted(ran)
"""),
    # the fused pipeline, 24^3 -> 24^3, both fp modes: on a single-level index it asks the lane kernel for rows in the
    # cell-sorted order of the targets (sorted_rows = 1; the library does not report the flag)
    "fused": ({}, r"""
pa, ca = synth.hex_mesh(24, seed=1)
pb, _ = synth.hex_mesh(24, seed=7)
fields = synth.vector_field(pa)
nn, _ = O.knn_ckdtree(O.centroid(ca, pa), pb, 20)
enc_o, w_o, nf_o = O.locate_hex8(nn, synth.reorder_hex8(ca), pa, pb)
vals_o = O.gather(fields, enc_o, w_o)
for mode in ("exact", "tol"):
    ctx.set_fp_mode(mode)
    vals, enc, w, nf = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=20, want_operator=True)
    assert "lane" in ctx.last_knn_kernels(), sorted(ctx.last_knn_kernels())
    vals, enc, w = vals.numpy(), enc.numpy(), w.numpy()
    assert nf == nf_o == 0 and np.array_equal(enc, enc_o), mode
    if mode == "exact":
        assert np.array_equal(w, w_o) and np.array_equal(vals, vals_o)
    else:
        assert np.abs(w - w_o).max() <= 1e-12 and np.abs(vals - vals_o).max() <= 1e-12 * 8 * np.abs(fields).max()
"""),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_CASES))
def test_lane_kernel_rows_match_the_oracle(case):
    knobs, body = _CASES[case]
    env = dict(os.environ, MM_KNN_KERNEL="lane", MM_KNN_LEVELS="1", **knobs)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body + 'print("ok")\n'], cwd=root, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
