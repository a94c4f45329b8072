"""The NumPy statement of the GLL mass matrix and of the weighted sum (mm_gll_mass / mm_weighted_sum in
include/multimesh_hip.h), an independent construction of the quadrature tables, and the error bounds the tests assert.
Nothing here imports the code under test.

  J[0][c] = sum_a D[i][a] X[a,j,k][c]     J[1][c] = sum_a D[j][a] X[i,a,k][c]     J[2][c] = sum_a D[k][a] X[i,j,a][c]
  det3 = (J00*(J11*J22 - J12*J21) - J01*(J10*J22 - J12*J20)) + J02*(J10*J21 - J11*J20)        det2 = J00*J11 - J01*J10
  mass = ((w_k * w_j) * w_i) * |det3|                                                  (2-D: (w_j * w_i) * |det2|)

with p = i + m j + m^2 k, m = order + 1.  Every product is rounded on its own (NumPy forms each as an array), every sum
starts from its first term and adds in ascending ``a``: the loop over ``a`` below is sequential, everything else is
vectorised over elements and nodes.

The weighted sum: t[i] = mass[i] * field[i] (or mass[i]), padded with +0.0 to whole chunks of CHUNK = 4096 values.  In a
chunk, lane l of LANES = 256 adds t[l], t[l + 256], ... t[l + 3840] in that order; then the 256 lane sums are halved eight
times, s[l] = s[l] + s[l + h] for h = 128, 64, ... 1.  The chunk sums are summed by the same rule until one value is left.
"""
import math

import numpy as np

EPS = 2.0 ** -52
CHUNK, LANES = 4096, 256


def tile_elems(order, dim):
    """Elements that share one 256-thread block of the GLL element tile (TILE of multimesh_amd/csrc/mm_gll_tile.h, on which
    mm_gll_mass, mm_gll_gradient and mm_gll_diffusion_apply work): as many whole elements as fit."""
    return 256 // (order + 1) ** dim


MAX_BLOCKS = 2048    # kMaxBlocks of mm_gll_tile.h: the blocks of a launch stride over the tiles beyond it
# (order, side, elements): the first ``elements`` elements of synth.gll_mesh(side, order), 3-D counts just past two tiles
# per block, where a block takes a third tile -- so both halves of a double buffer are refilled and a short tile arrives
# as a prefetched step.
#   order 4 (2 elements per tile): 4098 tiles, the last one short; blocks 0 and 1 take three steps, the rest two
#   order 2 (9 per tile, 243 of 256 lanes hold a node): 4097 tiles, the last one of 5 elements; block 0 takes three steps
MULTI_TILE = ((4, 22, 8195), (2, 35, 36869))


# ------------------------------------------------------------------------------------------------ tables, independently
def independent_tables(nodes):
    """(weights, D) of the GLL rule on ``nodes`` (the order + 1 GLL points) by another route than the package's:
    w_i = 2 / (N (N + 1) L_N(g_i)^2) with numpy.polynomial.legendre, D from barycentric differences
    D[i][a] = (lam_a / lam_i) / (g_i - g_a), D[i][i] = -sum of the rest of the row."""
    g = np.asarray(nodes, dtype=np.float64)
    n = len(g) - 1
    ln = np.polynomial.legendre.legval(g, [0.0] * n + [1.0])
    w = 2.0 / (n * (n + 1) * ln * ln)
    lam = np.array([1.0 / np.prod([g[i] - g[a] for a in range(n + 1) if a != i]) for i in range(n + 1)])
    D = np.zeros((n + 1, n + 1))
    for i in range(n + 1):
        for a in range(n + 1):
            if a != i:
                D[i, a] = (lam[a] / lam[i]) / (g[i] - g[a])
        D[i, i] = -sum(D[i, a] for a in range(n + 1) if a != i)
    return w, D


# ------------------------------------------------------------------------------------------------ the mass matrix
def mass(gll_points, order, w, D):
    """gll_points f64[E, P, dim] -> (mass f64[E, P], det f64[E, P])."""
    gp = np.asarray(gll_points, dtype=np.float64)
    w, D = np.asarray(w, dtype=np.float64), np.asarray(D, dtype=np.float64)
    E, P, dim = gp.shape
    m = order + 1
    assert P == m ** dim and dim in (2, 3)
    X = gp.reshape((E,) + (m,) * dim + (dim,))          # [E, k, j, i, c] (3-D) / [E, j, i, c]: i is the fastest
    axis_of = {0: dim, 1: dim - 1, 2: 1}                # tensor direction -> its axis of X
    J = []
    for d in range(dim):
        ax = axis_of[d]
        shape = [1] * (dim + 2)
        shape[ax] = m
        acc = None
        for a in range(m):
            line = np.take(X, [a], axis=ax)                              # X[.., a, ..] along direction d, kept as size 1
            t = D[:, a].reshape(shape) * line                            # D[i_d][a] * X[a][c], a rounded product
            acc = t if acc is None else acc + t
        J.append(acc)                                                    # [E, (k,) j, i, c]
    if dim == 3:
        J00, J01, J02 = J[0][..., 0], J[0][..., 1], J[0][..., 2]
        J10, J11, J12 = J[1][..., 0], J[1][..., 1], J[1][..., 2]
        J20, J21, J22 = J[2][..., 0], J[2][..., 1], J[2][..., 2]
        det = (J00 * (J11 * J22 - J12 * J21) - J01 * (J10 * J22 - J12 * J20)) + J02 * (J10 * J21 - J11 * J20)
        wp = (w[:, None, None] * w[None, :, None]) * w[None, None, :]    # [k, j, i]: (w_k * w_j) * w_i
    else:
        J00, J01, J10, J11 = J[0][..., 0], J[0][..., 1], J[1][..., 0], J[1][..., 1]
        det = J00 * J11 - J01 * J10
        wp = w[:, None] * w[None, :]                                     # [j, i]: w_j * w_i
    return (wp[None] * np.abs(det)).reshape(E, P), det.reshape(E, P)


def n_bad(det):
    """Nodes whose determinant is not > 0 (zero, negative, NaN)."""
    return int((~(np.asarray(det) > 0)).sum())


def mirrored(gll_points, e):
    """A copy with element ``e`` mirrored: its x coordinates negated about the element's centroid."""
    gp = np.array(gll_points, dtype=np.float64)
    cx = gp[e, :, 0].mean()
    gp[e, :, 0] = 2.0 * cx - gp[e, :, 0]
    return gp


# ------------------------------------------------------------------------------------------------ the weighted sum
def _sum_once(t):
    n = t.shape[-1]
    nchunk = max(1, -(-n // CHUNK))
    pad = np.zeros(t.shape[:-1] + (nchunk * CHUNK,))
    pad[..., :n] = t
    pad = pad.reshape(t.shape[:-1] + (nchunk, CHUNK // LANES, LANES))
    s = pad[..., 0, :]
    for r in range(1, CHUNK // LANES):
        s = s + pad[..., r, :]
    h = LANES // 2
    while h >= 1:
        s = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]                                                     # [..., nchunk]


def weighted_sum(mass_values, fields=None):
    """mass f64[n] (any shape, flattened), fields f64[C, n] or None -> f64[C] (f64[1] without fields)."""
    mv = np.asarray(mass_values, dtype=np.float64).reshape(-1)
    if fields is None:
        t = mv[None, :]
    else:
        f = np.asarray(fields, dtype=np.float64)
        t = mv[None, :] * (f.reshape(-1, mv.size) if mv.size else f.reshape(f.shape[0], 0))
    while True:
        t = _sum_once(t)
        if t.shape[-1] == 1:
            return np.ascontiguousarray(t[:, 0])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------ bounds
def term_bound(terms):
    """n * 2^-52 * sum|t|: n terms added in ANY order, each add with a relative error of at most 2^-53 on a partial sum
    that never exceeds sum|t| (tests/test_transpose.py::_row_bound)."""
    t = np.abs(np.asarray(terms, dtype=np.float64)).reshape(-1)
    return t.size * EPS * math.fsum(t)


def chunk_volume(r0, r1, half_lat_deg, lon_deg):
    """The volume of a spherical shell chunk: (r1^3 - r0^3) / 3 * (2 sin(lat)) * lon."""
    return (r1 ** 3 - r0 ** 3) / 3.0 * 2.0 * math.sin(math.radians(half_lat_deg)) * math.radians(lon_deg)
