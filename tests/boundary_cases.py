"""The NumPy statements of mm_boundary_faces, mm_boundary_classify, mm_boundary_nodes, mm_cutoff_distance and
mm_distance_taper (include/multimesh_hip.h), written from the header's text: np.unique over every face key, a plain loop
over the faces, a brute-force minimum over EVERY source -- no table, no grid, nothing skipped.  NumPy rounds every product,
quotient and sum on its own, as the library is built to."""
import numpy as np

FACE_CORNERS = np.array([[0, 2, 4, 6], [1, 3, 5, 7], [0, 1, 4, 5], [2, 3, 6, 7], [0, 1, 2, 3], [4, 5, 6, 7]])
FACE_CYCLIC = np.array([[0, 2, 6, 4], [1, 3, 7, 5], [0, 1, 5, 4], [2, 3, 7, 6], [0, 1, 3, 2], [4, 5, 7, 6]])
EXODUS_TO_TENSOR = [0, 1, 3, 2, 4, 5, 7, 6]
SIDE, TOP, BOTTOM = 0, 1, 2


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def corner_nodes(order):
    """node p = n i + m n j + m m n k of corner c = i + 2 j + 4 k"""
    n, m = order, order + 1
    return np.array([n * (c & 1) + m * n * ((c >> 1) & 1) + m * m * n * (c >> 2) for c in range(8)])


def face_nodes(order):
    """[6, m * m]: the nodes with i = 0, i = n, j = 0, j = n, k = 0, k = n, ascending"""
    m = order + 1
    p = np.arange(m ** 3)
    index = (p % m, (p // m) % m, p // (m * m))
    return np.array([p[index[f // 2] == (f % 2) * order] for f in range(6)])


def corner_ids(corners):
    """ids int64[E, 8] of corners f64[E, 8, 3] by coordinate identity, and their number"""
    flat = np.asarray(corners, dtype=np.float64).reshape(-1, 3) + 0.0           # (-0.0 -> +0.0)
    uniq, inverse = np.unique(flat, axis=0, return_inverse=True)
    return inverse.reshape(-1, 8).astype(np.int64), len(uniq)


def boundary_faces(ids):
    """(codes int64[nb] ascending, the number of faces whose key occurs more than twice)"""
    ids = np.asarray(ids, dtype=np.int64)
    keys = np.sort(ids[:, FACE_CORNERS], axis=2).reshape(-1, 4)
    if len(keys) == 0:
        return np.zeros(0, np.int64), 0
    _, inverse, counts = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    per_face = counts[inverse.reshape(-1)]
    return np.flatnonzero(per_face == 1).astype(np.int64), int((per_face > 2).sum())


def classify(corners, faces, up=None, cos_min=0.5):
    """side int32[nb]; up None: radial"""
    corners = np.asarray(corners, dtype=np.float64)
    side = np.zeros(len(faces), np.int32)
    for b, code in enumerate(np.asarray(faces)):
        c = corners[code // 6]
        q0, q1, q2, q3 = c[FACE_CYCLIC[code % 6]]
        a, bb = q2 - q0, q3 - q1
        n = np.array([a[1] * bb[2] - a[2] * bb[1], a[2] * bb[0] - a[0] * bb[2], a[0] * bb[1] - a[1] * bb[0]])
        fc = ((q0 + q1) + (q2 + q3)) * 0.25
        ec = (((((((c[0] + c[1]) + c[2]) + c[3]) + c[4]) + c[5]) + c[6]) + c[7]) * 0.125
        g = fc - ec
        if (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2] < 0:
            n = -n
        u = fc if up is None else np.asarray(up, dtype=np.float64)
        t = (n[0] * u[0] + n[1] * u[1]) + n[2] * u[2]
        lim = cos_min * np.sqrt(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) * ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]))
        side[b] = TOP if t >= lim else (BOTTOM if t <= -lim else SIDE)
    return side


def boundary_nodes(points, order, faces, side, mask):
    """f64[K, 3]: the nodes of the faces with bit (1 << side) in mask, face by face"""
    points = np.asarray(points, dtype=np.float64)
    nodes = face_nodes(order)
    rows = [points[code // 6][nodes[code % 6]] for code, s in zip(np.asarray(faces), np.asarray(side)) if (mask >> s) & 1]
    return np.concatenate(rows) if rows else np.zeros((0, 3))


def cutoff_distance(points, sources, cutoff):
    """(d f64[n], the number of d < cutoff): d = cutoff; for every source: if r < d: d = r"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    src = np.asarray(sources, dtype=np.float64).reshape(-1, 3)
    d = np.full(len(pts), float(cutoff))
    chunk = max(1, 2_000_000 // max(len(src), 1))
    for s in range(0, len(pts), chunk):
        p = pts[s:s + chunk]
        dx, dy, dz = (p[:, None, a] - src[None, :, a] for a in range(3))
        with np.errstate(invalid="ignore"):
            r = np.sqrt((dx * dx + dy * dy) + dz * dz)
        if r.shape[1]:
            least = np.where(np.isnan(r), np.inf, r).min(axis=1)                  # (a NaN r is never below d)
            d[s:s + chunk] = np.where(least < cutoff, least, cutoff)
    return d, int((d < cutoff).sum())


def taper_weight(d, inner, outer, elem=None):
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (d - inner) / (outer - inner)
        w = np.where(d <= inner, 0.0, np.where(d >= outer, 1.0, (s * s) * (3.0 - 2.0 * s)))
    if elem is not None:
        w = np.where(np.asarray(elem) < 0, 0.0, w)
    return w


def distance_taper(d, inner, outer, a, b=None, elem=None):
    """(out f64[C, n], w f64[n], the number of w < 1) for a, b f64[C, n]"""
    w = taper_weight(np.asarray(d).reshape(-1), inner, outer, None if elem is None else np.asarray(elem).reshape(-1))
    a = np.asarray(a, dtype=np.float64).reshape(-1, len(w))
    with np.errstate(invalid="ignore"):
        if b is None:
            out = w[None] * a
        else:
            b = np.asarray(b, dtype=np.float64).reshape(a.shape)
            out = np.where(w[None] == 0.0, b, np.where(w[None] == 1.0, a, (w[None] * a) + ((1.0 - w[None]) * b)))
    return out, w, int((w < 1.0).sum())


def holed(gp, drop=(0, 1, 13)):
    """the mesh without some elements"""
    return np.ascontiguousarray(np.delete(gp, list(drop), axis=0))
