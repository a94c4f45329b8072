"""Scenarios of the dispatch-matrix tests (tests/test_dispatch_matrix_gpu.py), and the oracle's view of them.

The kNN query and the hex8 locate pick their kernels at run time from the list length k, the length of the lists of
targets a kernel hands over, and how the targets spread over the grid.  Every builder here returns plain NumPy arrays;
tests/test_dispatch_cases.py checks on the CPU that each scenario really reaches the branch it is meant for (ties,
padding, lists longer than 32768 or 65536, targets that need candidates beyond the 8th) before anything runs on a GPU.

Oracles (oracle/oracle.py): cKDTree on clouds in general position, the brute kNN where exact ties occur (ties by
index, as ours), the C restatement of the reference's locate, NumPy-order gathers.  Results are cached per process.
"""
import functools

import numpy as np

from multimesh_amd import synth
from oracle import oracle as O

WORKERS = 16                       # CPU pools: at most 16 threads
KMAX = 64                          # MM_KNN_MAX_K
LIST_WAVE_MAX = 8192               # mm_knn.hip kListWaveMax: list mode, one wave per target up to this many
LONG_LIST_MIN = 32768              # mm_common.h MM_LONG_LIST_MIN
GROUP_LIST_MAX = 1 << 16           # mm_locate_hex8.hip kGroupListMax: longer reference-order lists take the loop kernel
LAZY_K = 8                         # mm_pipeline.hip kLazyK, mm_locate_gll.hip kGllLazyK
HEX_KS = (1, 2, 7, 8, 9, 16, 17, 20, 21, 25, 30, 32, 33, 40, 41, 64)
LONG_KS = (9, 25, 32, 33, 64)
TOL_KS = (9, 33, 64)
GLL_KS = (1, 8, 9, 25, 33, 64)


# ------------------------------------------------------------------------------------------------------------ kNN
@functools.lru_cache(maxsize=None)
def knn_cloud(kind, dim):
    """(sources, targets, tie-free?) of one cloud:
    uniform -- general position, targets reaching past the sources' box;
    lattice -- a jittered lattice of exactly representable points, targets on a finer lattice: exact distance ties;
    few     -- 13 sources, fewer than most k: rows padded with idx = nsrc, dist = inf."""
    rng = np.random.default_rng(100 * dim + {"uniform": 1, "lattice": 2, "few": 3}[kind])
    if kind == "uniform":
        nsrc = {1: 4000, 2: 12000, 3: 20000}[dim]
        return rng.uniform(size=(nsrc, dim)), rng.uniform(-0.1, 1.1, size=(3000, dim)), True
    if kind == "lattice":
        side = {1: 512, 2: 48, 3: 18}[dim]
        grid = np.stack(np.meshgrid(*[np.arange(side)] * dim, indexing="ij"), axis=-1).reshape(-1, dim)
        src = (grid + rng.integers(-1, 2, size=grid.shape) / 4.0) / 8.0      # multiples of 1/32: exact sums of squares
        tgt = rng.integers(-16, 32 * side + 16, size=(1500, dim)) / 32.0
        return np.ascontiguousarray(src), tgt, False
    return rng.uniform(size=(13, dim)), rng.uniform(-0.2, 1.2, size=(600, dim)), False


@functools.lru_cache(maxsize=None)
def knn_oracle(kind, dim):
    """(idx int64[N, 64], dist f64[N, 64]) of a cloud: rows padded beyond nsrc; ties by index where there are any."""
    src, tgt, tie_free = knn_cloud(kind, dim)
    kk = min(KMAX, len(src))
    idx = O.knn_ckdtree(src, tgt, kk, workers=WORKERS)[0] if tie_free else O.knn_brute(src, tgt, kk)
    full = np.full((len(tgt), KMAX), len(src), np.int64)
    full[:, :kk] = idx
    return full, knn_distances(src, tgt, full)


def knn_distances(src, tgt, idx):
    """sqrt of the in-order sum of squared coordinate differences (the kernels' dist_d); inf for padded ids."""
    pad = idx >= len(src)
    diff = src[np.where(pad, 0, idx)] - tgt[:, None, :]
    s = diff[..., 0] * diff[..., 0]
    for a in range(1, src.shape[1]):
        s = s + diff[..., a] * diff[..., a]
    return np.where(pad, np.inf, np.sqrt(s))


@functools.lru_cache(maxsize=None)
def graded_cloud():
    """Sources u^3 (density over orders of magnitude: several grid levels); the targets the same way and beyond."""
    rng = np.random.default_rng(41)
    src = rng.uniform(size=(60_000, 3)) ** 3.0
    tgt = np.concatenate([rng.uniform(size=(3_000, 3)) ** 3.0, rng.uniform(-0.1, 1.1, size=(1_000, 3))])
    idx = O.knn_ckdtree(src, tgt, KMAX, workers=WORKERS)[0]
    return src, tgt, idx, knn_distances(src, tgt, idx)


@functools.lru_cache(maxsize=None)
def list_mode_cloud(ntgt):
    """A uniform cloud queried by ntgt targets (both sides of LIST_WAVE_MAX), with its k = 32 oracle."""
    rng = np.random.default_rng(ntgt)
    src = rng.uniform(size=(30_000, 3))
    tgt = rng.uniform(-0.2, 1.2, size=(ntgt, 3))
    idx = O.knn_ckdtree(src, tgt, 32, workers=WORKERS)[0]
    return src, tgt, idx, knn_distances(src, tgt, idx)


SPLIT_KS = (8, 25)
STRIP_SPLIT_MIN = 192              # mm_knn.hip launch_fast: targets per strip from which nsplit = (n + 64) / 128 exceeds 1


@functools.lru_cache(maxsize=None)
def split_cloud():
    """Many more targets than sources (about 800 per strip of two cells): the strip kernel shares a strip's targets
    among several waves (nsplit > 1).  Targets reach past the sources' box; oracle for the longest k of SPLIT_KS."""
    rng = np.random.default_rng(77)
    src = rng.uniform(size=(2_000, 3))
    tgt = rng.uniform(-0.1, 1.1, size=(100_000, 3))
    idx = O.knn_ckdtree(src, tgt, max(SPLIT_KS), workers=WORKERS)[0]
    return src, tgt, idx, knn_distances(src, tgt, idx)


# ------------------------------------------------------------------------------------------------------------ hex8
def no_accept_within(status, m):
    """Targets the oracle accepts in none of their first m candidates (fallback to the best one, or failed)."""
    return (status < 0) | (status >= m)


@functools.lru_cache(maxsize=None)
def sheared_mesh():
    """A jittered mesh sheared and flattened so that the containing element's centroid is often not among the 8
    nearest; targets in and partly outside its box (the scene of test_fused_pipeline_lazy_equals_eager_when_lists_run_out)."""
    pa, ca = synth.hex_mesh(20, seed=5, jitter=0.3)
    pa = pa.copy()
    pa[:, 0] += 0.9 * pa[:, 2] + 0.5 * pa[:, 1]
    pa[:, 2] *= 0.15
    rng = np.random.default_rng(12)
    pb = rng.uniform(pa.min(axis=0) - 0.02, pa.max(axis=0) + 0.02, size=(12_000, 3))
    fields = synth.vector_field(pa)
    nn = O.knn_ckdtree(O.centroid(ca, pa), pb, KMAX, workers=WORKERS)[0]
    return pa, ca, pb, fields, nn


@functools.lru_cache(maxsize=None)
def tiny_mesh():
    """8 elements: fewer than most k (the kNN rows are padded with nelem; the locate skips those ids)."""
    pa, ca = synth.hex_mesh(3, seed=2, jitter=0.2)
    rng = np.random.default_rng(13)
    pb = np.concatenate([rng.uniform(-0.05, 1.05, size=(3_000, 3)), rng.uniform(2.0, 3.0, size=(200, 3))])
    nn = O.knn_ckdtree(O.centroid(ca, pa), pb, len(ca), workers=WORKERS)[0]
    return pa, ca, pb, synth.vector_field(pa), nn


@functools.lru_cache(maxsize=None)
def hex8_oracle(mesh, k):
    """(enc, w, nfailed, status) of the oracle's locate over the first k candidates (all of them if fewer)."""
    pa, ca, pb, _, nn = {"sheared": sheared_mesh, "tiny": tiny_mesh, "graded": graded_mesh}[mesh]()
    return O.locate_hex8(nn[:, :k], synth.reorder_hex8(ca), pa, pb, want_status=True)


@functools.lru_cache(maxsize=None)
def graded_mesh():
    """The u^2.2 graded mesh of test_graded_mesh_with_a_long_list_of_exhausted_targets: more than 32768 targets
    exhaust their 8 lazily evaluated candidates, so their full lists take the long-list path."""
    pa, ca = synth.hex_mesh(90, seed=3, jitter=0.1)
    pb, _ = synth.hex_mesh(90, seed=9, jitter=0.1)
    pa, pb = pa ** 2.2, pb ** 2.2
    nn = O.knn_ckdtree(O.centroid(ca, pa), pb, KMAX, workers=WORKERS)[0]
    return pa, ca, pb, synth.vector_field(pa)[:1], nn


@functools.lru_cache(maxsize=None)
def outside_mesh(nfar):
    """A 5^3-element mesh, nfar targets far outside it (no candidate is accepted, every row fails), targets in a thin
    band just outside (accepted by the smallest-error fallback) and targets inside.  Through the pipeline and the
    staged call alike these go to the reference-order kernel: the group kernel below 65536 of them, the loop above."""
    pa, ca = synth.hex_mesh(6, seed=4, jitter=0.2)
    rng = np.random.default_rng(nfar)
    far = rng.uniform(1.6, 2.6, size=(nfar, 3)) * rng.choice([-1.0, 1.0], size=(nfar, 3))
    band = rng.uniform(-0.02, 1.02, size=(20_000, 3))
    band = band[((band < 0) | (band > 1)).any(axis=1)][:1_500]
    inside = rng.uniform(0.05, 0.95, size=(3_000, 3))
    pb = np.concatenate([far, band, inside])
    pb = np.ascontiguousarray(pb[rng.permutation(len(pb))])
    nn = O.knn_ckdtree(O.centroid(ca, pa), pb, KMAX, workers=WORKERS)[0]
    return pa, ca, pb, synth.vector_field(pa)[:2], nn


OUTSIDE_SMALL, OUTSIDE_LARGE = 40_000, 72_000
OUTSIDE_CASES = [(OUTSIDE_SMALL, k) for k in (20, 32, 33, 64)] + [(OUTSIDE_LARGE, k) for k in (20, 64)]


def staged_lists(nn, k):
    """The first k candidates with the nearest moved to the end: a target just outside the mesh then falls back to
    its LAST candidate, which a reference-order kernel that stops short of the end of the list would miss."""
    return np.ascontiguousarray(np.roll(nn[:, :k], -1, axis=1))


@functools.lru_cache(maxsize=None)
def outside_oracle(nfar, k, staged=False):
    """(enc, w, nfailed, status) of the pipeline's lists (cKDTree order) or, staged=True, of staged_lists."""
    pa, ca, pb, _, nn = outside_mesh(nfar)
    return O.locate_hex8(staged_lists(nn, k) if staged else nn[:, :k], synth.reorder_hex8(ca), pa, pb, want_status=True)


def fp_tol(nodes, conn):
    """MM_FP_TOL's stated bound (include/multimesh_hip.h): max(1e-12, 64 eps max|x| / shortest element edge)."""
    v = nodes[conn]                                   # exodus corners [E, 8, 3]
    edges = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
    shortest = min(np.linalg.norm(v[:, a] - v[:, b], axis=1).min() for a, b in edges)
    return max(1e-12, 64 * np.finfo(np.float64).eps * np.abs(nodes).max() / shortest)


# ------------------------------------------------------------------------------------------------------------ GLL
@functools.lru_cache(maxsize=None)
def gll_case(order, dim):
    """A sheared GLL mesh (many targets outside, many not in one of their 8 nearest elements), 3 fields, cKDTree lists."""
    gp = synth.gll_mesh(7 if dim == 3 else 12, order, seed=9, jitter=0.25, dim=dim).copy()
    gp[..., 0] += 1.7 * gp[..., 1]
    rng = np.random.default_rng(10 * order + dim)
    lo, hi = gp.reshape(-1, dim).min(axis=0), gp.reshape(-1, dim).max(axis=0)
    pts = rng.uniform(lo - 0.02, hi + 0.02, size=(4_000, dim))
    fields = np.stack([synth.field_linear(gp), synth.field_smooth(gp.reshape(-1, dim)).reshape(gp.shape[:2]),
                       -1.0 - synth.field_linear(gp) ** 2])
    nn = O.knn_ckdtree(gp.mean(axis=1), pts, KMAX, workers=WORKERS)[0]
    return gp, pts, fields, nn


# ------------------------------------------------------------------------------------------------------------ gather
def gather_case(P, ncomp, seed=0):
    """fields f64[C, M] with zeros, ids int64[N, P], weights with -0.0 and negative entries: rows of -0.0 products."""
    rng = np.random.default_rng(1000 * P + ncomp + seed)
    nsrc, n = 5_000, 700
    fields = rng.normal(size=(ncomp, nsrc))
    fields[:, rng.random(nsrc) < 0.1] = 0.0
    ids = rng.integers(0, nsrc, size=(n, P))
    w = rng.normal(size=(n, P))
    w[rng.random((n, P)) < 0.1] = -0.0
    w[:50] = -0.0                                     # whole rows of -0.0 products: the sum's sign is NumPy's
    return fields, ids, w
