"""The NumPy statement of mm_harmonic_model_apply (include/multimesh_harmonics.h), written from the header and not from the
kernel: vectorised over the points, looped over (k, l).  Nothing here imports the code under test.  Every operation is one
NumPy float64 operation, bracketed as the header brackets it; only + - * / sqrt.

  direction   r, rho, ct, st, cp, sp of a point; the equator at the origin, longitude 0 on the axis
  fourier     C_k, S_k by complex multiplication
  legendre    4-pi-normalised P_lk without the Condon-Shortley phase, by the stated recurrences with the tables d, a, b
  lateral     S_j = term_0 + term_1 + ..., term_k = U_jk * C_k + V_jk * S_k
  apply       the element's centre picks the layer, the node's radius is clamped to it, bisected and lerped; three modes
"""
import numpy as np

from radial_cases import layers, radius, same_bits_nan  # noqa: F401  (same_bits_nan: re-exported for the tests)


def nlm(L):
    return (L + 1) * (L + 2) // 2


def idx(l, k, L):
    return k * (L + 1) - k * (k - 1) // 2 + (l - k)


def tables(L):
    """d f64[L + 1], a and b f64[NLM] at idx(l, k): integer products, one division, one sqrt; unused entries 0."""
    d, a, b = np.zeros(L + 1), np.zeros(nlm(L)), np.zeros(nlm(L))
    for k in range(1, L + 1):
        d[k] = np.sqrt(np.float64(3.0)) if k == 1 else np.sqrt(np.float64(2 * k + 1) / np.float64(2 * k))
    for k in range(L + 1):
        for l in range(k + 1, L + 1):
            a[idx(l, k, L)] = np.sqrt(np.float64((2 * l + 1) * (2 * l - 1)) / np.float64((l - k) * (l + k)))
            if l >= k + 2:
                b[idx(l, k, L)] = np.sqrt(np.float64((l - 1 - k) * (l - 1 + k)) / np.float64((2 * l - 1) * (2 * l - 3)))
    return d, a, b


def direction(points):
    """-> ct, st, cp, sp f64[N] of points f64[N, 3]."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) + z * z)
        rho = np.sqrt(x * x + y * y)
        ct = np.where(r == 0.0, 0.0, z / r)
        st = np.where(r == 0.0, 1.0, rho / r)
        cp = np.where(rho == 0.0, 1.0, x / rho)
        sp = np.where(rho == 0.0, 0.0, y / rho)
    return ct, st, cp, sp


def fourier(cp, sp, L):
    """-> C, S f64[L + 1, N]."""
    C, S = np.empty((L + 1, cp.size)), np.empty((L + 1, cp.size))
    C[0], S[0] = 1.0, 0.0
    with np.errstate(all="ignore"):
        for k in range(1, L + 1):
            if k == 1:
                C[1], S[1] = cp, sp
            else:
                C[k] = C[k - 1] * cp - S[k - 1] * sp
                S[k] = S[k - 1] * cp + C[k - 1] * sp
    return C, S


def legendre(ct, st, L):
    """-> P f64[NLM, N] at idx(l, k)."""
    d, a, b = tables(L)
    P = np.empty((nlm(L), ct.size))
    pkk = np.ones(ct.size)
    with np.errstate(all="ignore"):
        for k in range(L + 1):
            if k > 0:
                pkk = (d[k] * st) * pkk
            P[idx(k, k, L)] = pkk
            if k + 1 <= L:
                P[idx(k + 1, k, L)] = (a[idx(k + 1, k, L)] * ct) * pkk
            for l in range(k + 2, L + 1):
                q = idx(l, k, L)
                P[q] = a[q] * (ct * P[q - 1] - b[q] * P[q - 2])
    return P


def lateral(coef, rows, P, C, S, L):
    """coef f64[NC, m, 2, NLM], rows int[N] -> S_rows f64[NC, N]: sums left to right from their first term."""
    total = None
    with np.errstate(all="ignore"):
        for k in range(L + 1):
            U = V = None
            for l in range(k, L + 1):
                q = idx(l, k, L)
                u = coef[:, rows, 0, q] * P[q]
                U = u if U is None else U + u
                if k > 0:
                    v = coef[:, rows, 1, q] * P[q]
                    V = v if V is None else V + v
            term = U if k == 0 else U * C[k] + V * S[k]
            total = term if total is None else total + term
    return total


def intervals(points, radius_table, extend):
    """points f64[G, P, 3] -> (i int[G, P], t f64[G, P], dead bool[G, P], outside bool[G, P]): mm_radial_model_apply's
    layer, r', i and t; outside: the element's centre radius lies outside the table and extend is off."""
    pts = np.asarray(points, dtype=np.float64)
    G, P, _ = pts.shape
    R = np.asarray(radius_table, dtype=np.float64)
    lay = layers(R)
    with np.errstate(all="ignore"):
        c = pts[:, 0, :].copy()
        for p in range(1, P):
            c = c + pts[:, p, :]
        c = c / float(P)
        rc = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        dead_e = np.isnan(rc)
        outside_e = np.zeros(G, dtype=bool) if extend else (~dead_e) & ((rc < R[0]) | (rc > R[-1]))
        lo = np.array([R[a] for a, _ in lay])
        k = np.clip(np.searchsorted(lo, np.where(dead_e, lo[0], rc), side="right") - 1, 0, len(lay) - 1)
        ones = np.ones((1, P), dtype=np.int64)
        a = np.array([x[0] for x in lay])[k][:, None] * ones
        b = np.array([x[1] for x in lay])[k][:, None] * ones
        r = radius(pts).reshape(G, P)
        off = (dead_e | outside_e)[:, None] | np.zeros((1, P), dtype=bool)
        rr = np.where(off | np.isnan(r), R[a], r)
        rr = np.minimum(np.maximum(rr, R[a]), R[b])
        i = np.empty((G, P), dtype=np.int64)
        for (la, lb) in lay:
            sel = a == la
            i[sel] = np.clip(la + np.searchsorted(R[la:lb + 1], rr[sel], side="right") - 1, la, lb - 1)
        # (a NaN radius of a node in a live element: the clamps keep the NaN, the bisection sorts it behind every row, and
        # t is NaN)
        rr = np.where(np.isnan(r) & ~off, np.nan, rr)
        i = np.where(np.isnan(r) & ~off, b - 1, i)
        t = (rr - R[i]) / (R[i + 1] - R[i])
    dead = dead_e[:, None] | np.zeros((1, P), dtype=bool)
    outside = outside_e[:, None] | np.zeros((1, P), dtype=bool)
    return i, t, dead, outside


def model_apply(points, radius_table, coef, L, mode=0, extend=False, values_in=None):
    """points f64[G, P, 3] (or [N, 3]: P = 1), coef f64[NC, m, 2, NLM] -> (out f64[NC, G * P], noutside)."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 2:
        pts = pts[:, None, :]
    G, P, _ = pts.shape
    coef = np.asarray(coef, dtype=np.float64)
    NC = coef.shape[0]
    if G == 0 or NC == 0:
        return np.zeros((NC, G * P)), 0
    i, t, dead, outside = intervals(pts, radius_table, extend)
    i, t, dead, outside = i.reshape(-1), t.reshape(-1), dead.reshape(-1), outside.reshape(-1)
    ct, st, cp, sp = direction(pts.reshape(-1, 3))
    Pl = legendre(ct, st, L)
    C, S = fourier(cp, sp, L)
    with np.errstate(all="ignore"):
        s = (1.0 - t) * lateral(coef, i, Pl, C, S, L) + t * lateral(coef, i + 1, Pl, C, S, L)
        s = np.where(outside[None, :], 0.0, s)
        s = np.where(dead[None, :], np.nan, s)
        if mode == 0:
            out = s
        else:
            vin = np.asarray(values_in, dtype=np.float64).reshape(NC, G * P)
            out = vin + s if mode == 1 else vin + vin * s
    return out, int(outside.sum())


# --------------------------------------------------------------------------------------------------- the case generators
R_CMB, R_670, R_MOHO = 3480000.0, 5701000.0, 6346600.0


def knots(m=7, discontinuity=True):
    """f64[m]: a mantle table from the core-mantle boundary to the Moho, with the 670 as a repeated radius."""
    if not discontinuity:
        return np.linspace(R_CMB, R_MOHO, m)
    lower = m // 2
    return np.concatenate([np.linspace(R_CMB, R_670, lower), np.linspace(R_670, R_MOHO, m - lower)])


def coefficients(L, m, ncomp, seed):
    """f64[ncomp, m, 2, NLM]: random, falling off with the degree like a red spectrum, different on the two sides of a
    repeated radius."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((ncomp, m, 2, nlm(L)))
    for k in range(L + 1):
        for l in range(k, L + 1):
            c[..., idx(l, k, L)] /= (1.0 + l)
    return 0.02 * c


def directions(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def cloud(n, seed, r_lo=R_CMB, r_hi=R_MOHO):
    """f64[n, 3]: random directions at random radii in [r_lo, r_hi]."""
    rng = np.random.default_rng(seed + 1000)
    return directions(n, seed) * rng.uniform(r_lo, r_hi, (n, 1))


def elements(G, P, seed, size=40000.0, r_lo=R_CMB, r_hi=R_MOHO):
    """f64[G, P, 3]: G small elements, P nodes each within a cube of edge ``size`` about a random centre."""
    rng = np.random.default_rng(seed + 2000)
    centres = cloud(G, seed, r_lo, r_hi)
    return centres[:, None, :] + rng.uniform(-0.5 * size, 0.5 * size, (G, P, 3))


def shell_element(P, r_lo, r_hi, seed):
    """f64[P, 3]: one element whose nodes lie at radii spread over [r_lo, r_hi] around one direction (first node at r_lo,
    last at r_hi)."""
    rng = np.random.default_rng(seed + 3000)
    u = directions(1, seed)[0]
    r = np.linspace(r_lo, r_hi, P) if P > 1 else np.array([0.5 * (r_lo + r_hi)])
    side = np.cross(u, [0.3, -0.5, 0.8])
    return r[:, None] * u[None, :] + rng.uniform(-1e3, 1e3, (P, 1)) * side[None, :]
