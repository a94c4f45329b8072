"""The NumPy statements of mm_radial_bins, mm_binned_weighted_sum and mm_radial_model_apply (include/multimesh_hip.h),
written from the header and not from the kernels.  Nothing here imports the code under test.

  radius   r = sqrt((x*x + y*y) + z*z)
  bins     b = searchsorted(edges, r, side="right") - 1; r == edges[nbins] -> nbins - 1; -1 below, above and for NaN
  sums     per bin b: t = where(bin == b, mass * f, +0.0), padded with +0.0 to whole chunks of 4096; lane l of 256 computes
           (((+0.0 + t[l]) + t[l + 256]) + ...); the lane sums are halved eight times; the chunk sums go through the
           same rule until one value is left -- a loop over the bins, nothing is skipped here
  apply    the element's centre picks the layer, the node's radius is clamped to it, bisected and lerped; five modes
"""
import numpy as np

from mass_cases import CHUNK, LANES, same_bits  # noqa: F401  (same_bits: re-exported for the tests)


def radius(points):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.sqrt((x * x + y * y) + z * z)


def bins(points, edges):
    """-> (bin int32[n], number of -1 entries, radius f64[n])."""
    e = np.asarray(edges, dtype=np.float64)
    nb = e.size - 1
    r = radius(points)
    with np.errstate(invalid="ignore"):
        inside = (r >= e[0]) & (r <= e[nb])
    b = np.searchsorted(e, np.where(inside, r, e[0]), side="right") - 1
    b = np.minimum(b, nb - 1)
    b = np.where(inside, b, -1).astype(np.int32)
    return b, int((b < 0).sum()), r


def _sum_from_zero(t):
    """[..., n] -> [..., nchunk]: one level of the chunk rule, every lane sum started from +0.0."""
    n = t.shape[-1]
    nchunk = max(1, -(-n // CHUNK))
    pad = np.zeros(t.shape[:-1] + (nchunk * CHUNK,))
    pad[..., :n] = t
    pad = pad.reshape(t.shape[:-1] + (nchunk, CHUNK // LANES, LANES))
    s = np.zeros(pad.shape[:-2] + (LANES,))
    for r in range(CHUNK // LANES):
        s = s + pad[..., r, :]
    h = LANES // 2
    while h >= 1:
        s = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def terms(mass, fields=None, square=False):
    """f64[C, n]: mass * f, (mass * f) * f, or the mass alone (C = 1)."""
    m = np.asarray(mass, dtype=np.float64).reshape(-1)
    if fields is None:
        return m[None, :].copy()
    f = np.asarray(fields, dtype=np.float64).reshape(-1, m.size) if m.size else np.zeros((np.shape(fields)[0], 0))
    with np.errstate(invalid="ignore", over="ignore"):
        t = m[None, :] * f
        if square:
            t = t * f
    return t


def binned_weighted_sum(mass, fields, bin_ids, nbins, square=False):
    """-> f64[C, nbins], the statement above: a loop over the bins."""
    t = terms(mass, fields, square)
    b = np.asarray(bin_ids).reshape(-1)
    out = np.zeros((t.shape[0], nbins))
    for k in range(nbins):
        level = np.where((b == k)[None, :], t, 0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            while True:
                level = _sum_from_zero(level)
                if level.shape[-1] == 1:
                    break
        out[:, k] = level[:, 0]
    return out


def bin_counts(bin_ids, nbins):
    b = np.asarray(bin_ids).reshape(-1)
    b = b[(b >= 0) & (b < nbins)]
    return np.bincount(b, minlength=nbins).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the 1-D table
def layers(radius_table):
    """Rows (a, b), inclusive, of the maximal strictly ascending runs; ValueError for what the entry point refuses."""
    R = np.asarray(radius_table, dtype=np.float64)
    if R.ndim != 1 or R.size < 2 or not np.isfinite(R).all():
        raise ValueError("table")
    out, a = [], 0
    for i in range(1, R.size):
        if R[i] < R[i - 1]:
            raise ValueError("descending")
        if R[i] == R[i - 1]:
            out.append((a, i - 1))
            a = i
    out.append((a, R.size - 1))
    if any(b - a < 1 for a, b in out):
        raise ValueError("single row")
    return out


def model_apply(points, radius_table, values, mode=0, values_in=None):
    """points f64[G, P, 3] (or [N, 3]: P = 1), values f64[C, m] -> f64[C, G * P]."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 2:
        pts = pts[:, None, :]
    G, P, _ = pts.shape
    R = np.asarray(radius_table, dtype=np.float64)
    V = np.atleast_2d(np.asarray(values, dtype=np.float64))
    lay = layers(R)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = pts[:, 0, :].copy()
        for p in range(1, P):
            c = c + pts[:, p, :]
        c = c / float(P)
        rc = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        lo = np.array([R[a] for a, _ in lay])
        k = np.clip(np.searchsorted(lo, np.where(np.isnan(rc), lo[0], rc), side="right") - 1, 0, len(lay) - 1)
        a = np.array([x[0] for x in lay])[k][:, None] * np.ones((1, P), dtype=np.int64)      # [G, P]
        b = np.array([x[1] for x in lay])[k][:, None] * np.ones((1, P), dtype=np.int64)
        r = radius(pts).reshape(G, P)
        dead = np.isnan(rc)[:, None] | np.zeros((1, P), dtype=bool)
        rr = np.where(dead, R[a], r)
        rr = np.minimum(np.maximum(rr, R[a]), R[b])
        # upper_bound within the layer's rows: the rows of the other layers never lie strictly between R[a] and R[b]
        i = np.empty((G, P), dtype=np.int64)
        for (la, lb) in lay:
            sel = a == la
            i[sel] = np.clip(la + np.searchsorted(R[la:lb + 1], rr[sel], side="right") - 1, la, lb - 1)
        t = (rr - R[i]) / (R[i + 1] - R[i])
        out = np.empty((V.shape[0], G * P))
        vin = None if values_in is None else np.asarray(values_in, dtype=np.float64).reshape(V.shape[0], G * P)
        for q in range(V.shape[0]):
            ref = ((1.0 - t) * V[q][i] + t * V[q][i + 1])
            ref = np.where(dead, np.nan, ref).reshape(-1)
            if mode == 0:
                out[q] = ref
            elif mode == 1:
                out[q] = vin[q] - ref
            elif mode == 2:
                out[q] = (vin[q] - ref) / ref
            elif mode == 3:
                out[q] = vin[q] + ref
            elif mode == 4:
                out[q] = ref + vin[q] * ref
            else:
                raise ValueError("mode")
    return out


def same_bits_nan(a, b):
    """Bit equality where neither is NaN, and NaN in the same places (a NaN's payload and sign are not part of the
    statement: x86 and the GPU make different default NaNs)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))
