"""The NumPy statement of the GLL gradient (mm_gll_gradient in include/multimesh_hip.h).  Nothing here imports the code under
test; the Jacobian, its inverse G and the tensor-line sums are those of tests/diffusion_cases.py, stated once there.

At node (i, j, k) of an element, p = i + m j + m^2 k, m = order + 1:

  J, det, rdet = 1 / det, G[c][d]   : as diffusion_cases.geometry
  g[0] = sum_a D[i][a] u[a,j,k]      g[1] = sum_a D[j][a] u[i,a,k]      g[2] = sum_a D[k][a] u[i,j,a]
  gr[c] = (G[c][0]*g[0] + G[c][1]*g[1]) + G[c][2]*g[2]                  (2-D: the first two terms)
  norm = sqrt((gr[0]*gr[0] + gr[1]*gr[1]) + gr[2]*gr[2])                (2-D: sqrt(gr[0]*gr[0] + gr[1]*gr[1]))
  rn = sqrt((x*x + y*y) + z*z),  rh[c] = x[c] / rn (0 where rn == 0)
  s = (rh[0]*gr[0] + rh[1]*gr[1]) + rh[2]*gr[2]                                        the radial derivative
  l[c] = gr[c] - s*rh[c],  lateral = sqrt((l[0]*l[0] + l[1]*l[1]) + l[2]*l[2])

Every product is rounded on its own (NumPy forms each as an array), every sum over ``a`` starts from its first term and runs
in ascending ``a`` (diffusion_cases._lines).
"""
import numpy as np

from diffusion_cases import _lines, geometry

EPS = 2.0 ** -52

# Largest |gr - a| observed on the statement for u = a . x + b, a = (0.3, -1.7, 2.2), on synth.gll_mesh(6, order) in 3-D and
# gll_mesh(12, order, dim=2) (n - 1 elements per side): the tests assert ten times these.  In units of
# EPS * max|a| * cond, with cond = ||D||_inf * 2 (n - 1) -- the row sum of |D| (1, 4, 16.3 at orders 1, 2, 4: the rounding
# of a tensor-line sum of values of size |a|) times d xi / d x = 2 / h of an element of width h = 1 / (n - 1) -- they are
# 0.55, 0.77, 0.84 in 3-D and 0.33, 0.53, 0.52 in 2-D.
A = np.array([0.3, -1.7, 2.2])
SIDE = {3: 6, 2: 12}
LINEAR_OBSERVED = {(1, 3): 2.7e-15, (2, 3): 1.5e-14, (4, 3): 6.7e-14, (1, 2): 3.6e-15, (2, 2): 2.3e-14, (4, 2): 9.1e-14}


def linear_bound(order, dim, D):
    """(the bound on |gr - a| the tests assert for the linear field above, its multiple of EPS * max|a| * cond)."""
    cond = np.abs(np.asarray(D)).sum(axis=1).max() * 2.0 * (SIDE[dim] - 1)
    unit = EPS * np.abs(A).max() * cond
    multiple = 10.0 * LINEAR_OBSERVED[(order, dim)] / unit
    return multiple * unit, multiple


def gradient(gll_points, order, D, u):
    """u f64[C, E, P] (or [E, P]) -> (grad f64[C, dim, E, P], radial, lateral, norm each f64[C, E, P]); radial and
    lateral are None in 2-D."""
    gp = np.asarray(gll_points, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    E, P, dim = gp.shape
    m = order + 1
    u = np.asarray(u, dtype=np.float64)
    ncomp = u.shape[0] if u.ndim == 3 else 1
    u = u.reshape((ncomp, E) + (m,) * dim)
    G, _, _ = geometry(gp, order, np.ones(m), D)          # (the weights only enter the mass, which is not used)
    g = [_lines(D, u, u.ndim - 1 - d) for d in range(dim)]
    flat = (ncomp, E, P)
    if dim == 2:
        gr = [G[c][0] * g[0] + G[c][1] * g[1] for c in range(2)]
        norm = np.sqrt(gr[0] * gr[0] + gr[1] * gr[1])
        grad = np.stack([x.reshape(flat) for x in gr], axis=1)
        return np.ascontiguousarray(grad), None, None, np.ascontiguousarray(norm.reshape(flat))
    gr = [(G[c][0] * g[0] + G[c][1] * g[1]) + G[c][2] * g[2] for c in range(3)]
    norm = np.sqrt((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2])
    X = gp.reshape((E,) + (m,) * dim + (3,))
    x = [X[..., c] for c in range(3)]
    rn = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    safe = np.where(rn > 0.0, rn, 1.0)
    rh = [np.where(rn > 0.0, x[c] / safe, 0.0) for c in range(3)]
    s = (rh[0] * gr[0] + rh[1] * gr[1]) + rh[2] * gr[2]
    lat = [gr[c] - s * rh[c] for c in range(3)]
    lateral = np.sqrt((lat[0] * lat[0] + lat[1] * lat[1]) + lat[2] * lat[2])
    grad = np.stack([v.reshape(flat) for v in gr], axis=1)
    return (np.ascontiguousarray(grad), np.ascontiguousarray(s.reshape(flat)),
            np.ascontiguousarray(lateral.reshape(flat)), np.ascontiguousarray(norm.reshape(flat)))
