"""The NumPy statement of the GLL stiffness operator (mm_gll_diffusion_apply in include/multimesh_hip.h), of the diffusion
steps that smooth a field with it, and the bounds the tests assert.  Nothing here imports the code under test.

At node (i, j, k) of an element, p = i + m j + m^2 k, m = order + 1 (J, det and mass as in tests/mass_cases.py):

  rdet = 1 / det
  G[0][0] = (J11*J22 - J12*J21)*rdet   G[0][1] = (J02*J21 - J01*J22)*rdet   G[0][2] = (J01*J12 - J02*J11)*rdet
  G[1][0] = (J12*J20 - J10*J22)*rdet   G[1][1] = (J00*J22 - J02*J20)*rdet   G[1][2] = (J02*J10 - J00*J12)*rdet
  G[2][0] = (J10*J21 - J11*J20)*rdet   G[2][1] = (J01*J20 - J00*J21)*rdet   G[2][2] = (J00*J11 - J01*J10)*rdet
      (2-D: G[0][0] = J11*rdet, G[0][1] = (-J01)*rdet, G[1][0] = (-J10)*rdet, G[1][1] = J00*rdet)
  g[0] = sum_a D[i][a] u[a,j,k]        g[1] = sum_a D[j][a] u[i,a,k]        g[2] = sum_a D[k][a] u[i,j,a]
  gr[c] = (G[c][0]*g[0] + G[c][1]*g[1]) + G[c][2]*g[2]
  isotropic:   F[c] = (mass * kh) * gr[c]
  anisotropic: rn = sqrt((x*x + y*y) + z*z), rh[c] = x[c] / rn (0 where rn == 0), s = (rh[0]*gr[0] + rh[1]*gr[1]) + rh[2]*gr[2],
               F[c] = mass * (kh*gr[c] + ((kr - kh)*s) * rh[c])
  f[d] = (G[0][d]*F[0] + G[1][d]*F[1]) + G[2][d]*F[2]
  y = (sum_a D[a][i] f[0][a,j,k] + sum_a D[a][j] f[1][i,a,k]) + sum_a D[a][k] f[2][i,j,a]

with kh = kh_scalar * kh_array[n] (kh_scalar without an array), kr likewise.  Every product is rounded on its own (NumPy
forms each as an array), every sum over ``a`` starts from its first term and runs in ascending ``a``: the loop over ``a``
below is sequential, everything else is vectorised over components, elements and nodes.
"""
import math

import numpy as np

EPS = 2.0 ** -52


def _lines(T, A, axis):
    """sum_a T[i_d][a] * A[.. a ..] along ``axis`` (the tensor direction d): sequential in a, from the first term."""
    m = T.shape[0]
    shape = [1] * A.ndim
    shape[axis] = m
    acc = None
    for a in range(m):
        t = T[:, a].reshape(shape) * np.take(A, [a], axis=axis)
        acc = t if acc is None else acc + t
    return acc


def geometry(gll_points, order, w, D):
    """gll_points f64[E, P, dim] -> (G[c][d] each f64[E, (k,) j, i], mass f64[E, (k,) j, i], det)."""
    gp = np.asarray(gll_points, dtype=np.float64)
    w, D = np.asarray(w, dtype=np.float64), np.asarray(D, dtype=np.float64)
    E, P, dim = gp.shape
    m = order + 1
    assert P == m ** dim and dim in (2, 3)
    X = gp.reshape((E,) + (m,) * dim + (dim,))          # [E, k, j, i, c]: i is the fastest
    J = [_lines(D, X, X.ndim - 2 - d) for d in range(dim)]
    if dim == 3:
        J00, J01, J02 = J[0][..., 0], J[0][..., 1], J[0][..., 2]
        J10, J11, J12 = J[1][..., 0], J[1][..., 1], J[1][..., 2]
        J20, J21, J22 = J[2][..., 0], J[2][..., 1], J[2][..., 2]
        det = (J00 * (J11 * J22 - J12 * J21) - J01 * (J10 * J22 - J12 * J20)) + J02 * (J10 * J21 - J11 * J20)
        rdet = 1.0 / det
        G = [[(J11 * J22 - J12 * J21) * rdet, (J02 * J21 - J01 * J22) * rdet, (J01 * J12 - J02 * J11) * rdet],
             [(J12 * J20 - J10 * J22) * rdet, (J00 * J22 - J02 * J20) * rdet, (J02 * J10 - J00 * J12) * rdet],
             [(J10 * J21 - J11 * J20) * rdet, (J01 * J20 - J00 * J21) * rdet, (J00 * J11 - J01 * J10) * rdet]]
        wp = (w[:, None, None] * w[None, :, None]) * w[None, None, :]    # [k, j, i]: (w_k * w_j) * w_i
    else:
        J00, J01, J10, J11 = J[0][..., 0], J[0][..., 1], J[1][..., 0], J[1][..., 1]
        det = J00 * J11 - J01 * J10
        rdet = 1.0 / det
        G = [[J11 * rdet, (-J01) * rdet], [(-J10) * rdet, J00 * rdet]]
        wp = w[:, None] * w[None, :]
    return G, wp[None] * np.abs(det), det


def apply(gll_points, order, w, D, u, kh=1.0, kh_array=None, kr=None, kr_array=None):
    """y = K_e u: u f64[C, E, P] (or [E, P]) -> f64[C, E, P].  ``kr`` None: isotropic."""
    gp = np.asarray(gll_points, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    E, P, dim = gp.shape
    m = order + 1
    u = np.asarray(u, dtype=np.float64)
    ncomp = u.shape[0] if u.ndim == 3 else 1
    u = u.reshape((ncomp, E) + (m,) * dim)
    G, mass, _ = geometry(gp, order, w, D)
    grid = (E,) + (m,) * dim
    khv = np.float64(kh) * np.asarray(kh_array, dtype=np.float64).reshape(grid) if kh_array is not None else np.float64(kh)
    g = [_lines(D, u, u.ndim - 1 - d) for d in range(dim)]
    if dim == 3:
        gr = [(G[c][0] * g[0] + G[c][1] * g[1]) + G[c][2] * g[2] for c in range(3)]
    else:
        gr = [G[c][0] * g[0] + G[c][1] * g[1] for c in range(2)]
    if kr is None:
        assert kr_array is None
        mk = mass * khv
        F = [mk * gr[c] for c in range(dim)]
    else:
        assert dim == 3
        krv = (np.float64(kr) * np.asarray(kr_array, dtype=np.float64).reshape(grid) if kr_array is not None
               else np.float64(kr))
        X = gp.reshape(grid + (3,))
        x = [X[..., c] for c in range(3)]
        rn = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        safe = np.where(rn > 0.0, rn, 1.0)
        rh = [np.where(rn > 0.0, x[c] / safe, 0.0) for c in range(3)]
        s = (rh[0] * gr[0] + rh[1] * gr[1]) + rh[2] * gr[2]
        ks = (krv - khv) * s
        F = [mass * (khv * gr[c] + ks * rh[c]) for c in range(3)]
    if dim == 3:
        f = [(G[0][d] * F[0] + G[1][d] * F[1]) + G[2][d] * F[2] for d in range(3)]
    else:
        f = [G[0][d] * F[0] + G[1][d] * F[1] for d in range(2)]
    Dt = np.ascontiguousarray(D.T)
    y = _lines(Dt, f[0], u.ndim - 1) + _lines(Dt, f[1], u.ndim - 2)
    if dim == 3:
        y = y + _lines(Dt, f[2], u.ndim - 3)
    return np.ascontiguousarray(y.reshape(ncomp, E, P))


def element_matrices(gll_points, order, w, D, **kappa):
    """K_e f64[E, P, P] of the statement: column q is ``apply`` of the q-th unit vector of every element."""
    gp = np.asarray(gll_points, dtype=np.float64)
    E, P, _ = gp.shape
    eye = np.broadcast_to(np.eye(P)[:, None, :], (P, E, P))                 # component q: u[e][p] = (p == q)
    cols = apply(gp, order, w, D, np.ascontiguousarray(eye), **kappa)        # [q, E, p]
    return np.ascontiguousarray(cols.transpose(1, 2, 0))                     # [E, p, q]


def unique_nodes(gll_points):
    """(number of unique nodes, inverse int64[E * P]) over the coordinates, bit for bit."""
    gp = np.asarray(gll_points, dtype=np.float64)
    uniq, inv = np.unique(gp.reshape(-1, gp.shape[-1]), axis=0, return_inverse=True)
    return len(uniq), np.asarray(inv).reshape(-1)


def assembled(gll_points, order, w, D, **kappa):
    """(M f64[U] the assembled mass, K scipy.sparse.csr [U, U] = A^T K_e A, inverse int64[E * P], element mass [E * P])."""
    import scipy.sparse as sp

    gp = np.asarray(gll_points, dtype=np.float64)
    E, P, _ = gp.shape
    nu, inv = unique_nodes(gp)
    _, mass, _ = geometry(gp, order, w, D)
    me = mass.reshape(-1)
    Mu = np.zeros(nu)
    np.add.at(Mu, inv, me)
    Ke = element_matrices(gp, order, w, D, **kappa)
    ids = inv.reshape(E, P)
    rows = np.broadcast_to(ids[:, :, None], (E, P, P)).reshape(-1)
    cols = np.broadcast_to(ids[:, None, :], (E, P, P)).reshape(-1)
    K = sp.coo_matrix((Ke.reshape(-1), (rows, cols)), shape=(nu, nu)).tocsr()
    return Mu, K, inv, me


def node_mean(fields, inv, me, Mu):
    """The mass-weighted mean over the copies of every unique node: f64[C, E * P] -> f64[C, U]."""
    f = np.asarray(fields, dtype=np.float64).reshape(-1, inv.size)
    out = np.zeros((f.shape[0], Mu.size))
    for c in range(f.shape[0]):
        np.add.at(out[c], inv, me * f[c])
    return out / Mu[None]


def smooth_direct(gll_points, order, w, D, fields, steps, **kappa):
    """``steps`` backward-Euler steps (M + tau K) u_new = M u_old, tau = 1 / (2 steps), by a sparse direct solve of the
    statement's matrices.  fields f64[C, E, P] -> (u f64[C, U] on the unique nodes, u0 f64[C, U] the node-averaged input,
    M f64[U], inverse)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    Mu, K, inv, me = assembled(gll_points, order, w, D, **kappa)
    u0 = node_mean(fields, inv, me, Mu)
    u = u0.copy()
    if steps:
        lu = spla.splu((sp.diags(Mu) + K / (2.0 * steps)).tocsc())
        for _ in range(steps):
            u = np.stack([lu.solve(Mu * u[c]) for c in range(u.shape[0])])
    return u, u0, Mu, inv


def m_norm(Mu, v):
    return math.sqrt(math.fsum(Mu * v * v))


def gaussian_symbol(sigma, lam, steps):
    """What ``steps`` backward-Euler steps to the time sigma^2 / 2 do to an eigenfunction of eigenvalue ``lam``:
    (1 + sigma^2 lam / (2 steps))^-steps, which tends to exp(-sigma^2 lam / 2) as steps grows."""
    return (1.0 + sigma * sigma * lam / (2.0 * steps)) ** -steps


def welded(gll_points, bits=32):
    """Coordinates rounded to multiples of 2^-bits.  The copies of a shared node of ``synth.gll_mesh`` come from different
    elements' shape-function sums and differ in their last bits, so by their bits they are different nodes and the mesh
    falls apart along those faces; rounded, they are one node (the tests assert the count of unique nodes)."""
    scale = 2.0 ** bits
    return np.ascontiguousarray(np.round(np.asarray(gll_points, dtype=np.float64) * scale) / scale)
