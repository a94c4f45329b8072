"""The NumPy statement of mm_harmonic_model_transpose (include/multimesh_harmonic_adjoint.h), written from the header and not
from the kernel.  Nothing here imports the code under test.  What a node is comes from harmonic_cases (the statement of the
forward call); every product is one NumPy float64 operation, every sum a sequential one in the stated order.

  node_terms        the four terms (cosine, sine) x (Lo, Hi) of every node and (l, k) for one component
  model_transpose   the segment sums by np.cumsum along the node axis (its last column is the left-to-right sum), the
                    segments in ascending order, then Lo_j + Hi_{j-1}
  dense_matrix      H column by column from harmonic_cases.model_apply, for the tests that need a matrix
  cgls              the CGLS recurrence of multimesh_amd.harmonic_adjoint.fit_harmonic_model in NumPy
"""
import numpy as np

import harmonic_cases as HC

SEGMENT_NODES = 16384


def order_of(L):
    """int[NLM]: the order k of every idx(l, k)."""
    k_of = np.empty(HC.nlm(L), dtype=np.int64)
    for k in range(L + 1):
        k_of[HC.idx(k, k, L):HC.idx(L, k, L) + 1] = k
    return k_of


def node_terms(e0, e1, Pl, C, S, L):
    """e0, e1 f64[n] of one component -> f64[2 planes, 2 sides, NLM, n]: a0 * P_lk, a1 * P_lk, b0 * P_lk, b1 * P_lk."""
    k_of = order_of(L)
    with np.errstate(all="ignore"):
        Cq, Sq = C[k_of], S[k_of]
        zero = (k_of == 0)[:, None]
        a0 = np.where(zero, e0[None, :], e0[None, :] * Cq)
        a1 = np.where(zero, e1[None, :], e1[None, :] * Cq)
        b0, b1 = e0[None, :] * Sq, e1[None, :] * Sq
        return np.stack([np.stack([a0 * Pl, a1 * Pl]), np.stack([b0 * Pl, b1 * Pl])])


def model_transpose(points, radius_table, L, values, weight=None, extend=False):
    """points f64[G, P, 3] (or [N, 3]: P = 1), values f64[NC, G * P] -> (grad f64[NC, m, 2, NLM], noutside)."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 2:
        pts = pts[:, None, :]
    G, P, _ = pts.shape
    n = G * P
    R = np.asarray(radius_table, dtype=np.float64)
    m = R.size
    values = np.asarray(values, dtype=np.float64)
    values = values.reshape(-1, n) if n else values.reshape(values.shape[0] if values.ndim > 1 else 1, 0)
    NC = values.shape[0]
    lo = np.zeros((NC, m - 1, 2, HC.nlm(L)))
    hi = np.zeros((NC, m - 1, 2, HC.nlm(L)))
    nout = 0
    if G and NC:
        i, t, dead, outside = (x.reshape(-1) for x in HC.intervals(pts, R, extend))
        nout = int(outside.sum())
        part = ~(dead | outside)
        ct, st, cp, sp = HC.direction(pts.reshape(-1, 3))
        Pl = HC.legendre(ct, st, L)
        C, S = HC.fourier(cp, sp, L)
        Gs = max(1, SEGMENT_NODES // P)
        with np.errstate(all="ignore"):
            g = values if weight is None else np.asarray(weight, dtype=np.float64).reshape(1, n) * values
            e0, e1 = (1.0 - t) * g, t * g
            for c in range(NC):
                terms = node_terms(e0[c], e1[c], Pl, C, S, L)              # [plane, side, NLM, n]
                for first in range(0, n, Gs * P):                           # the segments, ascending
                    sl = slice(first, min(first + Gs * P, n))
                    for iv in np.unique(i[sl][part[sl]]):
                        member = part[sl] & (i[sl] == iv)
                        x = np.where(member, terms[..., sl], 0.0)           # +0.0 at non-members: their NaN does not reach the sum
                        x = np.concatenate([np.zeros(x.shape[:-1] + (1,)), x], axis=-1)   # the sum starts from +0.0
                        seg = np.cumsum(x, axis=-1)[..., -1]                # [plane, side, NLM]
                        lo[c, iv] = lo[c, iv] + seg[:, 0]
                        hi[c, iv] = hi[c, iv] + seg[:, 1]
    zero = np.zeros((NC, 1, 2, HC.nlm(L)))
    with np.errstate(all="ignore"):
        grad = np.concatenate([lo, zero], axis=1) + np.concatenate([zero, hi], axis=1)   # Lo_j + Hi_{j-1}
    grad[:, :, 1, :L + 1] = 0.0                                              # the sine plane at k = 0
    return grad, nout


def dense_matrix(points, radius_table, L, extend=False):
    """H f64[n, m * 2 * NLM] of one component, column by column from the forward statement on unit coefficients (the columns
    of the sine plane at k = 0 are zero: the forward call never reads them)."""
    R = np.asarray(radius_table, dtype=np.float64)
    ncol = R.size * 2 * HC.nlm(L)
    cols = []
    for q in range(ncol):
        unit = np.zeros(ncol)
        unit[q] = 1.0
        plane, at = (q // HC.nlm(L)) % 2, q % HC.nlm(L)
        if plane == 1 and at <= L:
            cols.append(None)
            continue
        cols.append(HC.model_apply(points, R, unit.reshape(1, R.size, 2, HC.nlm(L)), L, extend=extend)[0][0])
    n = next(c for c in cols if c is not None).size
    return np.stack([np.zeros(n) if c is None else c for c in cols], axis=1)


def cgls(H, f, w=None, damping=0.0, rtol=1e-8, max_iter=200):
    """min |W^(1/2) (H c - f)|^2 + damping |c|^2 from zero: the recurrence of fit_harmonic_model.  H f64[n, N], f f64[n],
    w f64[n] or None -> (c, iterations, residual |H^T W (f - H c) - damping c| / |H^T W f|)."""
    w = np.ones(H.shape[0]) if w is None else w
    x = np.zeros(H.shape[1])
    r = f.copy()
    s = H.T @ (w * r)
    p = s.copy()
    gamma = gamma0 = s @ s
    iterations, residual = 0, 1.0
    if gamma0 == 0.0:
        return x, 0, 0.0
    while iterations < max_iter:
        q = H @ p
        delta = (q * q * w).sum() + damping * (p @ p)
        alpha = gamma / delta
        x += alpha * p
        r -= alpha * q
        s = H.T @ (w * r) - damping * x
        gamma_new = s @ s
        iterations += 1
        residual = float(np.sqrt(gamma_new / gamma0))
        if not residual > rtol:
            break
        p = s + (gamma_new / gamma) * p
        gamma = gamma_new
    return x, iterations, residual


def shell_cloud(n, seed, m=3):
    """(points f64[n, 3], radii f64[m]): n random directions at random radii inside a table of m knots without a
    discontinuity: a well-conditioned global cover."""
    R = HC.knots(m, discontinuity=False)
    return HC.cloud(n, seed, R[0], R[-1]), R
