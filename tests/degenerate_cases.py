"""Scenarios for testing locate, kNN and the fused pipelines on degenerate elements and non-finite coordinates, and the
oracle's view of them.

Real inputs hold these: exodus meshes carry collapsed hexes, make_spherical leaves a point at the centre alone, a model with
a masked region has NaN nodes.  The builders return plain NumPy arrays; tests/test_degenerate_cases.py checks on the CPU
that each scenario does what it is for (targets accepted in degenerate elements, failures, fallbacks, exact ties, solves the
fast Newton cannot certify, NaN transforms): a GPU test over a scenario that misses them would prove nothing.

The meshes contain duplicate centroids, so the lists come from the brute-force kNN (oracle/oracle.py), ties by index as
the kernels order them.  Results are cached per process and must not be modified by a test."""
import functools

import numpy as np

from multimesh_amd import synth
from oracle import oracle as O

KMAX = 64                          # MM_KNN_MAX_K
HEX_KS = (1, 8, 20, 33, 64)
GLL_KS = (1, 8, 20)
GLL_NN = 25                        # candidates kept per GLL target (the 2-D meshes have fewer than 64 elements)
EPS = np.finfo(np.float64).eps

# kinds of elements (0: an element of the regular mesh)
REGULAR, FLAT, ZERO, MIRRORED, TANGLED, EDGE, FACE, DUPLICATE, HUGE, TINY, FOLDED = range(11)
KIND_NAMES = ("regular", "flat", "zero-size", "mirrored", "tangled", "collapsed edge", "collapsed face", "duplicate", "huge",
              "tiny", "folded")
# elements MM_FP_TOL's stated bound says nothing about: orientation lost (mirrored, tangled, folded), or -- found by its
# shortest edge -- an edge of length zero (zero-size, collapsed edge, collapsed face)
NOT_ORIENTED = (MIRRORED, TANGLED, FOLDED)

_CUBE = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], float) - 0.5
# exodus corner pairs that share an edge
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _centres(rng, n, size):
    """n element centres: most inside the unit box, every fourth just outside one of its faces."""
    c = rng.uniform(0.1, 0.9, size=(n, 3))
    for i in range(3, n, 4):
        a = rng.integers(0, 3)
        c[i, a] = rng.choice([-0.4 * size, 1.0 + 0.4 * size])
    return c


# ------------------------------------------------------------------------------------------------------------ hex8
@functools.lru_cache(maxsize=None)
def bad_hex_mesh():
    """(nodes, exodus connectivity, targets, fields, lists int64[N, 64], kind int[E]): the 1331 jittered elements of
    synth.hex_mesh(12) and, appended, elements that own their nodes (the neighbours stay intact): flat, zero-size, mirrored,
    tangled, with a collapsed edge or face (connectivity repeats a node id), exact duplicates of regular elements (the same
    connectivity row: identical centroids, the kNN tie goes by index), one huge element around the whole mesh and one
    tiny one with edges of 1e-9."""
    pa, ca = synth.hex_mesh(12, seed=21, jitter=0.2)
    rng = np.random.default_rng(2101)
    h = 1.0 / 11
    nodes, conn, kind = [pa], [ca], [np.zeros(len(ca), np.int64)]
    next_id = len(pa)

    def add(corners, code, ids=None):
        nonlocal next_id
        nodes.append(np.asarray(corners, float))
        row = next_id + (np.arange(8) if ids is None else np.asarray(ids))
        conn.append(row[None, :])
        kind.append(np.array([code]))
        next_id += 8

    def cube(c, size):
        return c + (_CUBE + rng.uniform(-0.15, 0.15, size=(8, 3))) @ _rotation(rng).T * size

    plan = [(FLAT, 8), (ZERO, 7), (MIRRORED, 8), (TANGLED, 10), (EDGE, 8), (FACE, 7)]
    centres = _centres(rng, sum(n for _, n in plan), h)
    i = 0
    for code, n in plan:
        for j in range(n):
            c, i = centres[i], i + 1
            v = cube(c, h * rng.uniform(0.7, 1.3))
            if code == FLAT:                       # all eight nodes in one plane: zero determinant everywhere
                nrm = _rotation(rng)[0]
                v = v - ((v - c) @ nrm)[:, None] * nrm
                add(v, code)
            elif code == ZERO:
                add(np.repeat(c[None], 8, axis=0), code)
            elif code == MIRRORED:                 # bottom and top face swapped: negative determinant
                add(v, code, ids=[4, 5, 6, 7, 0, 1, 2, 3])
            elif code == TANGLED:
                add(v, code, ids=rng.permutation(8))
            elif code == EDGE:                     # one edge collapsed, or two: a wedge
                add(v, code, ids=[0, 0, 2, 3, 4, 5, 6, 7] if j % 2 else [0, 0, 2, 3, 4, 4, 6, 7])
            else:                                  # the top face collapsed: a pyramid
                add(v, code, ids=[0, 1, 2, 3, 4, 4, 4, 4])
    for e in rng.choice(len(ca), 8, replace=False):            # exact duplicates: the same row, the same centroid
        conn.append(ca[e][None, :])
        kind.append(np.array([DUPLICATE]))
    add(0.5 + _CUBE * 1.3, HUGE)
    add(rng.uniform(0.3, 0.7, size=3) + _CUBE * 1e-9, TINY)
    nodes, conn, kind = np.ascontiguousarray(np.concatenate(nodes)), np.ascontiguousarray(np.concatenate(conn)), np.concatenate(kind)

    added = np.flatnonzero(kind != REGULAR)
    v = nodes[conn[added]]                                       # [A, 8, 3]
    wts = rng.dirichlet(np.full(8, 0.5), size=(len(added), 12))  # points in and around every appended element
    far = rng.uniform(1.6, 2.6, size=(300, 3)) * rng.choice([-1.0, 1.0], size=(300, 3))
    pb = np.concatenate([rng.uniform(-0.02, 1.02, size=(4300, 3)), v.reshape(-1, 3), v.mean(axis=1),
                         nodes[conn[kind == ZERO][:, 0]], np.einsum("aqc,acj->aqj", wts, v).reshape(-1, 3), far])
    pb = np.ascontiguousarray(pb[rng.permutation(len(pb))])
    nn = O.knn_brute(O.centroid(conn, nodes), pb, KMAX)
    return nodes, conn, pb, synth.vector_field(nodes), nn, kind


@functools.lru_cache(maxsize=None)
def bad_hex_oracle(k):
    """(enc, w, nfailed, status) of the oracle's locate over the first k candidates of bad_hex_mesh."""
    pa, ca, pb, _, nn, _ = bad_hex_mesh()
    return O.locate_hex8(nn[:, :k], synth.reorder_hex8(ca), pa, pb, want_status=True)


def accepted_element(status, nn, k):
    """The element every target was located in (-1: failed), from the oracle's status (j accepted, k + j the fallback)."""
    j = np.where(status >= k, status - k, status)
    return np.where(status < 0, -1, nn[np.arange(len(nn)), np.maximum(j, 0)])


def shortest_edge(nodes, conn):
    v = nodes[conn]
    return np.min([np.linalg.norm(v[:, a] - v[:, b], axis=1) for a, b in EDGES], axis=0)


def comparable_elements(nodes, conn, kind):
    """Elements MM_FP_TOL's bound applies to: not mirrored, tangled or folded, and the shortest edge positive."""
    return ~np.isin(kind, NOT_ORIENTED) & (shortest_edge(nodes, conn) > 0)


def fp_tol_rows(nodes, conn):
    """MM_FP_TOL's stated bound (include/multimesh_hip.h) for every element on its own: max(1e-12, 64 eps max|x| / the
    element's shortest edge) -- dispatch_cases.fp_tol over that one element.  inf where an edge has length zero."""
    with np.errstate(divide="ignore"):
        return np.maximum(1e-12, 64 * EPS * np.abs(nodes).max() / shortest_edge(nodes, conn))


def newton_pairs(k=20):
    """(points f64[N k, 3], corners f64[N k, 8, 3] in the locator's order) of every (target, candidate) pair of bad_hex_mesh."""
    pa, ca, pb, _, nn, _ = bad_hex_mesh()
    conn = synth.reorder_hex8(ca)
    return np.ascontiguousarray(np.repeat(pb, k, axis=0)), np.ascontiguousarray(pa[conn[nn[:, :k].ravel()]])


# ------------------------------------------------------------------------------------------------------------ GLL
def gll_element(order, corners):
    """The control nodes of one element from its corners (exodus / counter-clockwise order), as synth.gll_mesh places them."""
    corners = np.asarray(corners, float)
    dim = corners.shape[1]
    g = synth.gll_nodes_1d(order)
    if dim == 3:
        sign = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], float)
        k_, j_, i_ = np.meshgrid(g, g, g, indexing="ij")
        xi = np.stack([i_.ravel(), j_.ravel(), k_.ravel()], axis=1)
    else:
        sign = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float)
        j_, i_ = np.meshgrid(g, g, indexing="ij")
        xi = np.stack([i_.ravel(), j_.ravel()], axis=1)
    shape = np.prod(1.0 + xi[:, None, :] * sign[None, :, :], axis=2) / 2 ** dim
    return shape @ corners


@functools.lru_cache(maxsize=None)
def bad_gll_mesh(order, dim):
    """(gll_points, targets, fields f64[3, E, P], lists int64[N, 25], kind int[E]): synth.gll_mesh (5 nodes a side in 3-D, 8
    in 2-D) and, appended: flat, zero-size and mirrored elements, duplicates of regular elements and, at orders 2 and
    4, folded elements -- a control node in the middle of one face pushed through the opposite face, so that the Jacobian
    changes sign inside."""
    n = 5 if dim == 3 else 8
    gp = synth.gll_mesh(n, order, seed=31, jitter=0.2, dim=dim)
    rng = np.random.default_rng(3100 + 10 * order + dim)
    h = 1.0 / (n - 1)
    m = order + 1
    unit = (_CUBE if dim == 3 else _CUBE[:4, :2])
    extra, kind = [], []

    def corners(c):
        v = unit + rng.uniform(-0.15, 0.15, size=unit.shape)
        if dim == 3:
            v = v @ _rotation(rng).T
        return c + v * h * rng.uniform(0.7, 1.3)

    centres = _centres(rng, 16, h)[:, :dim]
    for i, c in enumerate(centres):
        code = (FLAT, ZERO, MIRRORED, FOLDED)[i % 4]
        v = corners(c)
        if code == FLAT:                           # every node on one plane (3-D) or line (2-D)
            nrm = _rotation(rng)[0][:dim]
            nrm /= np.linalg.norm(nrm)
            el = gll_element(order, v - ((v - c) @ nrm)[:, None] * nrm)
        elif code == ZERO:
            el = np.repeat(c[None], m ** dim, axis=0)
        elif code == MIRRORED:
            el = gll_element(order, v[[4, 5, 6, 7, 0, 1, 2, 3]] if dim == 3 else v[[3, 2, 1, 0]])
        else:
            if order == 1:
                continue
            el = gll_element(order, v)
            mid = m // 2
            lo = mid * m + (mid * m * m if dim == 3 else 0)       # the middle of the face xi_1 = -1 ...
            hi = lo + m - 1                                       # ... and of the face xi_1 = +1
            el[lo] = el[hi] + 0.4 * (el[hi] - el[lo])
        extra.append(el)
        kind.append(code)
    for e in rng.choice(len(gp), 4, replace=False):
        extra.append(gp[e])
        kind.append(DUPLICATE)
    kind = np.concatenate([np.zeros(len(gp), np.int64), np.array(kind)])
    extra = np.stack(extra)
    gp = np.ascontiguousarray(np.concatenate([gp, extra]))

    wts = rng.dirichlet(np.full(m ** dim, 0.5), size=(len(extra), 20))
    far = rng.uniform(1.6, 2.6, size=(200, dim)) * rng.choice([-1.0, 1.0], size=(200, dim))
    # on the corners of every appended element, on a stride across all their other control nodes, on their centroids
    corner_ids = [i + m * (j + m * k) for k in ((0, m - 1) if dim == 3 else (0,)) for j in (0, m - 1) for i in (0, m - 1)]
    on_nodes = extra.reshape(-1, dim)
    on_nodes = on_nodes[::max(1, len(on_nodes) // 250)]
    pts = np.concatenate([rng.uniform(-0.02, 1.02, size=(2000, dim)), extra[:, corner_ids].reshape(-1, dim), on_nodes,
                          extra.mean(axis=1),
                          np.einsum("aqc,acj->aqj", wts, extra).reshape(-1, dim), far])
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    fields = np.stack([synth.field_linear(gp), synth.field_smooth(gp.reshape(-1, dim)).reshape(gp.shape[:2]),
                       -1.0 - synth.field_linear(gp) ** 2])
    nn = O.knn_brute(gp.mean(axis=1), pts, GLL_NN)
    return gp, pts, np.ascontiguousarray(fields), nn, kind


def gll_node_determinants(order, elements):
    """det of the Jacobian dx / dxi at every control node of elements f64[E, P, dim] -> f64[E, P]."""
    dmat = synth.gll_derivative_matrix(order)                # dmat[i, a] = l_a'(g_i)
    nel, npts, dim = elements.shape
    m = order + 1
    x = elements.reshape((nel,) + (m,) * dim + (dim,))       # [E, (k,) j, i, c]
    cols = []
    for axis in range(dim):                                  # reference axis 0 is the fastest index i = the last grid axis
        moved = np.moveaxis(x, dim - axis, -2)               # [..., a, c]
        cols.append(np.moveaxis(np.einsum("ia,...ac->...ic", dmat, moved), -2, dim - axis))
    jac = np.stack(cols, axis=-1)                            # [E, grid, c, axis]
    return np.linalg.det(jac).reshape(nel, npts)


# ------------------------------------------------------------------------------------------------------------ non-finite
def nonfinite_targets(pts, seed=0):
    """(a copy of pts with about 1 % of its rows replaced, the mask of those rows).  The replacements cycle through a NaN
    in one coordinate, NaN in all, +inf, -inf, +1e308 and -1e308; they sit in the first and the last row, on either side of
    rows 64 and 256 (wave and workgroup boundaries), in one run of 70 consecutive rows (a whole wave and more) and
    at random rows."""
    pts = np.array(pts, dtype=np.float64)
    n, dim = pts.shape
    rng = np.random.default_rng(seed + n)
    rows = {0, n - 1, 63, 64, 65, 255, 256, 257}
    start = n // 2
    rows.update(range(start, start + 70))
    rows.update(rng.choice(n, max(0, n // 100 - len(rows)), replace=False).tolist())
    rows = np.array(sorted(r for r in rows if 0 <= r < n))
    for i, r in enumerate(rows):
        axis = (i // 6) % dim
        case = i % 6
        if case == 0:
            pts[r, axis] = np.nan
        elif case == 1:
            pts[r] = np.nan
        else:
            pts[r, axis] = (np.inf, -np.inf, 1e308, -1e308)[case - 2]
    mask = np.zeros(n, bool)
    mask[rows] = True
    return np.ascontiguousarray(pts), mask


@functools.lru_cache(maxsize=None)
def good_hex_mesh():
    """(nodes, exodus connectivity, targets, fields) of a well-shaped mesh: the scene of the non-finite targets."""
    pa, ca = synth.hex_mesh(12, seed=23, jitter=0.2)
    rng = np.random.default_rng(2301)
    pb = np.ascontiguousarray(rng.uniform(-0.02, 1.02, size=(3000, 3)))
    return pa, ca, pb, synth.vector_field(pa)


@functools.lru_cache(maxsize=None)
def nonfinite_mesh():
    """(nodes, exodus connectivity, targets, fields, mask of the affected elements): good_hex_mesh with one coordinate of
    two interior nodes NaN and of one interior node inf -- 8 elements around each."""
    pa, ca, pb, _ = good_hex_mesh()
    pa = pa.copy()
    n = 12
    bad = [(3 * n + 4) * n + 5, (7 * n + 7) * n + 2, (9 * n + 3) * n + 8]
    pa[bad[0], 0] = np.nan
    pa[bad[1], 2] = np.nan
    pa[bad[2], 1] = np.inf
    affected = np.isin(ca, bad).any(axis=1)
    assert affected.sum() == 24
    with np.errstate(invalid="ignore"):
        fields = synth.vector_field(pa)                   # (NaN at the masked nodes, as a masked model has)
    return pa, ca, pb, fields, affected
