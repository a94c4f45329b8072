"""The NumPy statement of mm_idw_gather (include/multimesh_hip.h), written from the header's text, and the inputs the
scattered-import tests share.  Vectorised over the targets with an explicit loop over j, so the order of every sum is the
statement's; NumPy rounds every quotient, product and sum on its own, as the library is built to."""
import numpy as np

FILL, KEEP = 0, 2


def same_bits(a, b):
    """Equal shapes and equal bits -- except that any NaN equals any NaN: a NaN that arithmetic produced carries the sign the
    processor gives it (x86 and the GPU differ there), and no statement pins it."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]))


def weights(idx, dist, nsrc, power, max_distance):
    """(valid bool[N, k], w f64[N, k], m int32[N], nearest f64[N], hit int64[N] -- the lowest valid j at distance 0.0, or -1)"""
    idx = np.asarray(idx, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.float64)
    n, k = idx.shape
    with np.errstate(invalid="ignore"):
        valid = (idx >= 0) & (idx < nsrc) & (dist <= max_distance)
    m = valid.sum(axis=1).astype(np.int32)
    j0 = np.where(m > 0, valid.argmax(axis=1), 0)
    d0 = dist[np.arange(n), j0] if k else np.zeros(n)
    nearest = np.where(m > 0, d0, np.inf)
    zero = valid & (dist == 0.0)
    hit = np.where(zero.any(axis=1), zero.argmax(axis=1), -1).astype(np.int64)
    w = np.zeros((n, k))
    with np.errstate(all="ignore"):
        for j in range(k):
            r = d0 / dist[:, j]
            q = r.copy()
            for _ in range(power - 1):
                q = q * r
            w[:, j] = np.where(valid[:, j], q, 0.0)
    return valid, w, m, nearest, hit


def idw(fields, idx, dist, nsrc, power=2, max_distance=np.inf, outside=FILL, fill=np.nan, prior=None):
    """(out f64[C, N], noutside, nearest f64[N], nused int32[N]) for fields f64[C, nsrc]; prior f64[C, N]: what out held
    (read for outside == KEEP)"""
    fields = np.asarray(fields, dtype=np.float64).reshape(-1, nsrc)
    idx = np.asarray(idx, dtype=np.int64)
    n, k = idx.shape
    valid, w, m, nearest, hit = weights(idx, dist, nsrc, power, max_distance)
    safe = np.where(valid, idx, 0)
    s = np.zeros(n)
    for j in range(k):
        s = s + w[:, j]
    out = np.empty((len(fields), n))
    rows = np.arange(n)
    for c, f in enumerate(fields):
        num = np.zeros(n)
        with np.errstate(all="ignore"):
            for j in range(k):
                v = np.where(valid[:, j], f[safe[:, j]] if nsrc else 0.0, 0.0)
                num = num + (w[:, j] * v)
            val = num / s
        exact = f[safe[rows, np.maximum(hit, 0)]] if nsrc else np.zeros(n)
        val = np.where(hit >= 0, exact, val)
        if outside == KEEP:
            val = np.where(m == 0, np.asarray(prior, dtype=np.float64).reshape(len(fields), n)[c], val)
        else:
            val = np.where(m == 0, fill, val)
        out[c] = val
    return out, int((m == 0).sum()), nearest, m


def knn(sources, targets, k):
    """Brute-force rows as mm_knn_query states them: ascending by sqrt of the squared distance summed axis by axis, equal
    distances by index, rows of fewer than k sources padded with (nsrc, inf); a source with a NaN coordinate is not listed."""
    src = np.asarray(sources, dtype=np.float64)
    tgt = np.asarray(targets, dtype=np.float64)
    nsrc = len(src)
    idx = np.full((len(tgt), k), nsrc, dtype=np.int64)
    dist = np.full((len(tgt), k), np.inf)
    for i, t in enumerate(tgt):
        d2 = np.zeros(nsrc)
        for a in range(src.shape[1]):
            d2 = d2 + (t[a] - src[:, a]) * (t[a] - src[:, a])
        listed = np.flatnonzero(~np.isnan(d2))
        order = listed[np.lexsort((listed, d2[listed]))][:k]
        idx[i, :len(order)] = order
        dist[i, :len(order)] = np.sqrt(d2[order])
    return idx, dist


def cloud(n, ndim=3, ncomp=3, seed=0, scale=1.0):
    """A seeded general-position cloud: (points f64[n, ndim] in [0, scale)^ndim, fields f64[ncomp, n])"""
    rng = np.random.default_rng(seed)
    return rng.random((n, ndim)) * scale, rng.standard_normal((ncomp, n))


def targets(n, ndim=3, seed=1, scale=1.0):
    """Seeded targets in [-0.1, 1.1)^ndim * scale: some lie outside the cloud's box"""
    rng = np.random.default_rng(seed)
    return (rng.random((n, ndim)) * 1.2 - 0.1) * scale
