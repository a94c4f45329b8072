"""The NumPy statements of mm_point_taper, mm_order_statistics and mm_clamp (include/multimesh_hip.h), written from the
header and not from the kernels.  Nothing here imports the code under test.

  taper    per node and centre: d = sqrt((dx*dx + dy*dy) + dz*dz); t = 0 if d <= inner, 1 else if d >= outer, else
           (s*s) * (3 - 2*s) with s = (d - inner) / (outer - inner); w = 1, then for k ascending: if t_k < w: w = t_k --
           a loop over ALL centres, nothing is skipped here; out = w * in
  select   NaNs out; key = sign(u) ? ~u : u | 2^63 of the bits (of |v| with absolute); rank = floor / ceil of
           q * float(nvalid - 1); the value whose key has that rank in the sorted keys
  clamp    where(v < lo, lo, where(v > hi, hi, v)); the count of the replaced values
"""
import numpy as np

from mass_cases import same_bits  # noqa: F401  (re-exported for the tests)
from radial_cases import same_bits_nan  # noqa: F401

SIGN = np.uint64(1) << np.uint64(63)


# --------------------------------------------------------------------------------------------------------- the taper
def smoothstep(s):
    return (s * s) * (3.0 - 2.0 * s)


def taper_weight(points, centres, inner, outer):
    """points f64[..., 3] -> (w f64[n] flat, number of nodes with w < 1)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    ri = np.broadcast_to(np.asarray(inner, dtype=np.float64), (len(c),))
    ro = np.broadcast_to(np.asarray(outer, dtype=np.float64), (len(c),))
    w = np.ones(len(p))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for k in range(len(c)):
            dx, dy, dz = p[:, 0] - c[k, 0], p[:, 1] - c[k, 1], p[:, 2] - c[k, 2]
            d = np.sqrt((dx * dx + dy * dy) + dz * dz)
            s = (d - ri[k]) / (ro[k] - ri[k])
            t = np.where(d <= ri[k], 0.0, np.where(d >= ro[k], 1.0, smoothstep(s)))
            w = np.where(t < w, t, w)
    return w, int(np.count_nonzero(w < 1.0))


def taper_apply(points, centres, inner, outer, values):
    """values f64[C, n] -> (out f64[C, n], w f64[n], count)."""
    w, count = taper_weight(points, centres, inner, outer)
    v = np.asarray(values, dtype=np.float64).reshape(-1, w.size) if w.size else np.zeros((np.shape(values)[0], 0))
    with np.errstate(invalid="ignore", over="ignore"):
        return w[None, :] * v, w, count


# -------------------------------------------------------------------------------------------------------- the select
def keys(values, absolute=False):
    """uint64 keys of the bits of ``values`` (no NaN expected): unsigned order = numeric order, -0.0 before +0.0."""
    u = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64).copy()
    if absolute:
        u &= ~SIGN
    neg = (u & SIGN) != 0
    return np.where(neg, ~u, u | SIGN)


def values_of_keys(k):
    k = np.asarray(k, dtype=np.uint64)
    return np.where((k & SIGN) != 0, k & ~SIGN, ~k).view(np.float64)


def ranks(q, nvalid, method):
    pos = np.asarray(q, dtype=np.float64) * np.float64(nvalid - 1)
    return (np.floor(pos) if method == "lower" else np.ceil(pos)).astype(np.int64)


def order_statistics(values, q, absolute=False, method="lower"):
    """values f64[C, n] -> (out f64[C, m], nvalid int64[C])."""
    v = np.asarray(values, dtype=np.float64)
    v = v.reshape(1, -1) if v.ndim == 1 else v.reshape(v.shape[0], -1)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    out = np.full((v.shape[0], q.size), np.nan)
    nvalid = np.zeros(v.shape[0], dtype=np.int64)
    for c in range(v.shape[0]):
        valid = v[c][~np.isnan(v[c])]
        nvalid[c] = valid.size
        if valid.size:
            k = np.sort(keys(valid, absolute))
            out[c] = values_of_keys(k[ranks(q, valid.size, method)])
    return out, nvalid


# --------------------------------------------------------------------------------------------------------- the clamp
def clamp(values, lower=None, upper=None, symmetric=False):
    """values f64[C, n], bounds f64[C] or None -> (out, changed int64[C])."""
    v = np.asarray(values, dtype=np.float64)
    v = v.reshape(1, -1) if v.ndim == 1 else v.reshape(v.shape[0], -1)
    C = v.shape[0]
    hi = np.full(C, np.inf) if upper is None else np.asarray(upper, dtype=np.float64).reshape(C)
    lo = -hi if symmetric else (np.full(C, -np.inf) if lower is None else np.asarray(lower, dtype=np.float64).reshape(C))
    with np.errstate(invalid="ignore"):
        below, above = v < lo[:, None], v > hi[:, None]
    out = np.where(below, lo[:, None], np.where(above, hi[:, None], v))
    return out, (below | above).sum(axis=1).astype(np.int64)
