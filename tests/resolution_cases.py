"""The NumPy statements of mm_gll_resolution and mm_arg_extreme (include/multimesh_hip.h), vectorised, plain NumPy, and the
case lists the CPU and GPU tests share.  Every difference, product, sum, root and quotient below is one NumPy operation,
rounded on its own; minima and maxima have no order.  ``x * x``, never ``x ** 2``."""
import numpy as np

#: (order, dim, P, TILE): the elements a 256-lane block takes per step
TILES = [(4, 3, 125, 2), (2, 3, 27, 9), (1, 3, 8, 32), (4, 2, 25, 10), (2, 2, 9, 28), (1, 2, 4, 64)]
#: element counts per tile size: none, one, a tile less one, a tile, a tile and one, three tiles and one
def element_counts(tile):
    return [0, 1, tile - 1, tile, tile + 1, 3 * tile + 1]


ARG_EXTREME_N = [0, 1, 255, 256, 257, 100_003]
GUARDED_NELEM = [512, 64, 1, 2, 101]
GUARDED_N = [1, 2, 255, 512, 4097]


def same_bits(a, b):
    """Equal shapes, NaN in the same places (its payload is not part of a statement), equal bits everywhere else."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return bool(np.array_equal(np.where(na, 0.0, a).view(np.uint64), np.where(nb, 0.0, b).view(np.uint64)))


def corner_nodes(order, dim):
    """Node p = n i + m n j + m m n k of every tensor corner c = i + 2 j + 4 k (2-D: the first four)."""
    n, m = int(order), int(order) + 1
    return np.array([n * (c & 1) + m * n * ((c >> 1) & 1) + m * m * n * (c >> 2) for c in range(1 << dim)], dtype=np.int64)


def edge_pairs(dim):
    """The corner pairs (c, c | 1 << d) with bit d of c clear: 12 in 3-D, 4 in 2-D."""
    return [(c, c | (1 << d)) for c in range(1 << dim) for d in range(dim) if not (c >> d) & 1]


def distance(earlier, later):
    """sqrt((dx*dx + dy*dy) + dz*dz) with d = later - earlier; 2-D: sqrt(dx*dx + dy*dy)."""
    d = later - earlier
    s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    if d.shape[-1] == 3:
        s = s + d[..., 2] * d[..., 2]
    return np.sqrt(s)


def node_spacing(gp, order):
    """h f64[E, P]: the least distance from every node to its tensor-line neighbours."""
    gp = np.asarray(gp, dtype=np.float64)
    E, P, dim = gp.shape
    m = order + 1
    assert P == m ** dim
    grid = gp.reshape((E,) + (m,) * dim + (dim,))        # [E, (k,) j, i, dim]: direction d is axis dim - d
    h = np.full((E,) + (m,) * dim, np.inf)
    with np.errstate(all="ignore"):
        for d in range(dim):
            axis = dim - d
            lo = [slice(None)] * (dim + 1)
            hi = [slice(None)] * (dim + 1)
            lo[axis], hi[axis] = slice(0, m - 1), slice(1, m)
            lo, hi = tuple(lo), tuple(hi)
            seg = distance(grid[lo], grid[hi])              # node -> its successor along d
            h[lo] = np.minimum(h[lo], seg)
            h[hi] = np.minimum(h[hi], seg)
    return h.reshape(E, P)


def edges(gp, order):
    """f64[E, 12] (2-D: [E, 4]): the straight corner-to-corner edge lengths (chords)."""
    gp = np.asarray(gp, dtype=np.float64)
    dim = gp.shape[2]
    corners = gp[:, corner_nodes(order, dim)]
    with np.errstate(all="ignore"):
        cols = [distance(corners[:, a], corners[:, b]) for a, b in edge_pairs(dim)]
    return np.stack(cols, axis=1) if len(gp) else np.zeros((0, len(cols)))


def resolution(gp, order, fast=None, slow=None):
    """(out f64[5, E] -- f64[3, E] without fast --, info int64[2], h f64[E, P]) as mm_gll_resolution states them."""
    gp = np.asarray(gp, dtype=np.float64)
    E, P, dim = gp.shape
    h = node_spacing(gp, order)
    ed = edges(gp, order)
    geo = ~np.isfinite(gp).all(axis=(1, 2))
    rows = [h.min(axis=1), ed.min(axis=1), ed.max(axis=1)] if E else [np.zeros(0)] * 3
    model = geo.copy()
    if fast is not None:
        fast = np.asarray(fast, dtype=np.float64)
        slow = np.zeros((0, E, P)) if slow is None else np.asarray(slow, dtype=np.float64)
        fast, slow = (v[None] if v.ndim == 2 else v for v in (fast, slow))
        assert fast.shape[0] >= 1 and fast.shape[1:] == (E, P) == slow.shape[1:]
        with np.errstate(all="ignore"):
            vfast = fast.max(axis=0)
            step = (h / vfast).min(axis=1) if E else np.zeros(0)
            positive = slow > 0
            least = np.where(positive, slow, np.inf).min(axis=0) if slow.shape[0] else np.full((E, P), np.inf)
            vslow = np.where(positive.any(axis=0), least, fast.min(axis=0))
            period = rows[2] / vslow.min(axis=1) if E else np.zeros(0)
        model |= ~np.isfinite(fast).all(axis=(0, 2)) | (fast <= 0).any(axis=(0, 2))
        model |= ~np.isfinite(slow).all(axis=(0, 2)) | (slow < 0).any(axis=(0, 2))
        rows += [np.where(model, np.nan, step), np.where(model, np.nan, period)]
    else:
        assert slow is None
    out = np.stack(rows).astype(np.float64)
    out[:3, geo] = np.nan
    h = h.copy()
    h[geo] = np.nan
    return out, np.array([geo.sum(), model.sum()], dtype=np.int64), h


def arg_extreme(values, want_max=False):
    """(value f64[R], index int64[R], nvalid int64[R]) of values f64[R, n] (or [n]: one row): the least or greatest value
    that is not a NaN, the lowest index among equals (-0.0 == +0.0), the value stored there; NaN and -1 for none."""
    v = np.asarray(values, dtype=np.float64)
    v = v.reshape(1, -1) if v.ndim == 1 else v.reshape(v.shape[0], -1)
    value, index = np.full(len(v), np.nan), np.full(len(v), -1, dtype=np.int64)
    nvalid = np.zeros(len(v), dtype=np.int64)
    for r, row in enumerate(v):
        valid = np.flatnonzero(~np.isnan(row))
        nvalid[r] = len(valid)
        if len(valid):
            index[r] = valid[np.argmax(row[valid]) if want_max else np.argmin(row[valid])]
            value[r] = row[index[r]]
    return value, index, nvalid


def velocities(gp, ncomp, seed, lo=3000.0, hi=8000.0):
    """ncomp positive fields f64[ncomp, E, P] over a mesh, seeded."""
    return np.random.default_rng(seed).uniform(lo, hi, (ncomp,) + gp.shape[:2])
