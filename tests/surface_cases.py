"""The NumPy statements of mm_boundary_triangles and mm_surface_distance (include/multimesh_surface.h), written from the
header's text: the faces' node grids cut into triangles, the closest-point region walk vectorised with np.where in the
header's branch order, and a brute-force minimum over EVERY triangle -- no grid, nothing skipped.  NumPy rounds every
product, quotient and sum on its own, as the library is built to."""
import numpy as np

from boundary_cases import face_nodes, same_bits  # noqa: F401  (same_bits is part of this module's interface)


def boundary_triangles(points, order, faces, side, mask):
    """f64[T, 3, 3]: two triangles per sub-quad of the node grid q[j][i] of every face with bit (1 << side) in mask (side
    None: every face), j-major, face by face"""
    points = np.asarray(points, dtype=np.float64)
    m = order + 1
    nodes = face_nodes(order)                                 # ascending node index: q[j][i] = row[i + m * j]
    faces = np.asarray(faces)
    selected = np.ones(len(faces), bool) if side is None else ((mask >> np.asarray(side)) & 1).astype(bool)
    out = []
    for code in faces[selected]:
        q = points[code // 6][nodes[code % 6]].reshape(m, m, 3)
        for j in range(order):
            for i in range(order):
                out.append([q[j][i], q[j][i + 1], q[j + 1][i + 1]])
                out.append([q[j][i], q[j + 1][i + 1], q[j + 1][i]])
    return np.array(out, dtype=np.float64).reshape(-1, 3, 3)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def closest(p, a, b, c):
    """q f64[..., 3] for p, a, b, c f64[..., 3] (broadcast): the region walk, the first condition that holds decides"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (p, a, b, c)))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        v_ab = (d1 / (d1 - d3))[..., None]
        w_ac = (d2 / (d2 - d6))[..., None]
        w_bc = (e43 / (e43 + e56))[..., None]
        den = 1.0 / ((va + vb) + vc)
        v, w = (vb * den)[..., None], (vc * den)[..., None]
        conditions = [(d1 <= 0) & (d2 <= 0),
                      (d3 >= 0) & (d4 <= d3),
                      (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                      (d6 >= 0) & (d5 <= d6),
                      (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                      (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        values = [a, b, a + v_ab * ab, c, a + w_ac * ac, b + w_bc * (c - b)]
        q = (a + ab * v) + ac * w
        for cond, value in zip(reversed(conditions), reversed(values)):
            q = np.where(cond[..., None], value, q)
    return q


def triangle_distance(p, a, b, c):
    """r f64[...]: sqrt((dx*dx + dy*dy) + dz*dz) of p - closest(p; a, b, c)"""
    with np.errstate(all="ignore"):
        dlt = np.asarray(p, dtype=np.float64) - closest(p, a, b, c)
        return np.sqrt((dlt[..., 0] * dlt[..., 0] + dlt[..., 1] * dlt[..., 1]) + dlt[..., 2] * dlt[..., 2])


def with_cutoff(unbounded, cutoff):
    """(d, the number of d < cutoff) of ``surface_distance(..., cutoff)`` from ``surface_distance(..., inf)[0]`` of the same
    points and triangles: the statement's d is the least r where that is below the cutoff and the cutoff elsewhere, so one
    brute-force pass serves every cutoff of a test"""
    least = np.asarray(unbounded, dtype=np.float64)
    d = np.where(least < cutoff, least, float(cutoff))
    return d, int((d < cutoff).sum())


def surface_distance(points, tri, cutoff):
    """(d f64[n], the number of d < cutoff): d = cutoff; for every triangle: if r < d: d = r"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    cutoff = float(cutoff)
    d = np.full(len(pts), cutoff)
    chunk = max(1, 400_000 // max(len(tri), 1))
    for s in range(0, len(pts), chunk):
        if not len(tri):
            break
        r = triangle_distance(pts[s:s + chunk, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        least = np.where(np.isnan(r), np.inf, r).min(axis=1)                      # (a NaN r is never below d)
        d[s:s + chunk] = np.where(least < cutoff, least, cutoff)
    return d, int((d < cutoff).sum())
