"""The NumPy statement of include/multimesh_regions.h (``mm_region_distance``), operation by operation, the polygons and node
sets of tests/test_regions.py and tests/test_regions_gpu.py, and the inputs of tests/test_regions_guarded_gpu.py.  No kernel
runs here."""
import numpy as np

from multimesh_amd import regions as RG

CHUNK = 32                      # MM_REGION_EDGE_CHUNK
EDGE_COUNTS = (0, 1, 3, 12, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7)
R_EARTH = 6371000.0


# ---------------------------------------------------------------------------------------------------------- the statement
def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


MIN_RADIUS = 2.0 ** -500        # the header's floor of r


def region_distance(points, edges, anchor, anchor_inside, cutoff, scale, block=1):
    """(signed f64[n], inside int32[n], ninside, nhit, ninvalid) for points f64[..., 3] read flat.  ``block=1`` is the header's
    loop, edge by edge in ascending order.  A larger ``block`` takes that many edges at once as arrays [block, n] and joins them
    with a minimum and a sum, which change no bit (tests/test_regions.py holds the two forms together): for the large tables."""
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1, 9)
    a = np.asarray(anchor, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        valid = np.isfinite(r) & (r >= MIN_RADIUS)
        p = np.where(valid[:, None], x / r[:, None], 0.0)
        m = cross(p, a[None, :])
        q = np.full(len(x), cutoff * cutoff)
        hit = np.zeros(len(x), dtype=bool)
        ncross = np.zeros(len(x), dtype=np.int64)
        for first in range(0, len(edges), block):
            rows = edges[first:first + block]
            U, V, N = rows[:, None, 0:3], rows[:, None, 3:6], rows[:, None, 6:9]
            su, sv, tp, ta = dot(m[None], U), dot(m[None], V), dot(N, p[None]), dot(N, a[None, None, :])
            crosses = ((su >= 0) != (sv >= 0)) & ((tp >= 0) != (ta >= 0)) & ((ta >= 0) == (su >= 0))
            ncross += crosses.sum(axis=0)
            w1, w2 = dot(cross(U, p[None]), N), dot(cross(p[None], V), N)
            g = 1.0 - tp * tp
            g = np.where(g < 0.0, 0.0, g)
            circle = (2.0 * (tp * tp)) / (1.0 + np.sqrt(g))
            du, dv = p[None] - U, p[None] - V
            qe = np.where((w1 >= 0) & (w2 >= 0), circle, np.minimum(dot(du, du), dot(dv, dv))).min(axis=0)
            less = qe < q
            q = np.where(less, qe, q)
            hit |= less
        inside = np.where(valid, int(anchor_inside) ^ (ncross & 1), 0).astype(np.int32)
        d = np.where(hit, scale * np.sqrt(q), scale * cutoff)
        s = np.where(valid, np.where(inside == 1, d, -d), -(scale * cutoff))
    hit &= valid
    return s, inside, int(inside.sum()), int(hit.sum()), int((~valid).sum())


def taper_weight(d, inner, outer):
    """mm_distance_taper's weight."""
    with np.errstate(all="ignore"):
        s = (d - inner) / (outer - inner)
        return np.where(d <= inner, 0.0, np.where(d >= outer, 1.0, (s * s) * (3.0 - 2.0 * s)))


def blend(w, a, b):
    return np.where(w == 0.0, b, np.where(w == 1.0, a, (w * a) + ((1.0 - w) * b)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------------------ the regions
def wiggly_ring(nedges, lat=20.0, lon=30.0, radius_deg=12.0, wiggle=0.25, lobes=5):
    """A star-like ring of ``nedges`` vertices about (lat, lon), counter-clockwise, as (lat, lon) in degrees."""
    phi = 2.0 * np.pi * np.arange(nedges) / nedges
    rad = radius_deg * (1.0 + wiggle * np.sin(lobes * phi))
    return np.stack([lat + rad * np.sin(phi), lon + rad * np.cos(phi) / np.cos(np.deg2rad(lat))], axis=1)


def region_with(nedges, **kw):
    """A :class:`Region` of ``nedges`` >= 3 edges; for 0 and 1 edges see :func:`edge_table`."""
    return RG.Region(wiggly_ring(nedges, **kw), interior="left")


def edge_table(nedges):
    """(edges f64[E, 9], anchor, anchor_inside) with exactly ``nedges`` edges: a ring of max(nedges, 3) cut short.  A table
    that is no closed ring is still a statement; the flag then means nothing geographic."""
    reg = region_with(max(nedges, 3))
    return np.ascontiguousarray(reg.edges[:nedges]), reg.anchor, reg.anchor_inside


def concave_12gon():
    return wiggly_ring(12, lat=-10.0, lon=100.0, radius_deg=25.0, wiggle=0.5, lobes=3)


def ring_with_hole():
    outer = wiggly_ring(24, lat=35.0, lon=-60.0, radius_deg=20.0, wiggle=0.1)
    hole = wiggly_ring(9, lat=35.0, lon=-60.0, radius_deg=6.0, wiggle=0.0)[::-1]
    return [outer, hole]


def polar_cap(colat=10.0, n=36, clockwise=False):
    lon = np.arange(n) * (360.0 / n) + 0.37
    ring = np.stack([np.full(n, 90.0 - colat), lon], axis=1)
    return ring[::-1] if clockwise else ring


def antimeridian_ring():
    return wiggly_ring(16, lat=-15.0, lon=179.0, radius_deg=14.0, wiggle=0.2)


def named_regions():
    """name -> Region: the polygons of the independent-method tests."""
    return {"concave 12-gon": RG.Region(concave_12gon()), "ring with a hole": RG.Region(ring_with_hole()),
            "cap over a pole": RG.Region(polar_cap()), "across the antimeridian": RG.Region(antimeridian_ring())}


def sphere_points(n, seed, radius=1.0):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return radius * v / np.linalg.norm(v, axis=1)[:, None]


def winding_inside(points, region):
    """The independent inside flag, without the anchor: the winding number of every ring about the point, by summed atan2 angles
    in the point's tangent plane.  A ring that is smaller than a hemisphere winds by o about the points of its smaller side, by
    -o about their antipodes and by 0 elsewhere, o = +-1 its orientation, read off at the ring's centroid (inside, for the
    star-shaped rings here); the region is the even-odd combination of the smaller sides.
    Returns (inside bool[n], near bool[n]): near marks points within 1e-6 rad of the outline (left out)."""
    p = points / np.linalg.norm(points, axis=1)[:, None]
    near = np.zeros(len(p), dtype=bool)
    inside = np.zeros(len(p), dtype=bool)

    def winding(x, edges, mark=None):
        total = np.zeros(len(x))
        for row in edges:
            u, v = row[0:3], row[3:6]
            tu = u[None] - (x @ u)[:, None] * x
            tv = v[None] - (x @ v)[:, None] * x
            total += np.arctan2(np.einsum("ij,ij->i", x, np.cross(tu, tv)), np.einsum("ij,ij->i", tu, tv))
            if mark is not None:
                n = np.cross(u, v)
                n /= np.linalg.norm(n)
                lune = ((np.cross(u[None], x) @ n) >= 0.0) & ((np.cross(x, v[None]) @ n) >= 0.0)
                ends = np.minimum(np.linalg.norm(x - u, axis=1), np.linalg.norm(x - v, axis=1))
                mark |= np.where(lune, np.abs(x @ n), ends) < 1e-6
        return np.rint(total / (2.0 * np.pi)).astype(int)

    for b, e in zip(region._ring_edges[:-1], region._ring_edges[1:]):
        ring = region.edges[b:e]
        centroid = ring[:, 0:3].sum(axis=0)
        centroid /= np.linalg.norm(centroid)
        o = winding(centroid[None], ring)[0]
        assert o in (-1, 1)
        inside ^= winding(p, ring, near) == o
    return inside, near


def sampled_distance(points, region, per_arc=2000):
    """The independent distance: the chord to the nearest of ``per_arc`` + 1 samples of every arc, and the largest sample spacing."""
    p = points / np.linalg.norm(points, axis=1)[:, None]
    best = np.full(len(p), np.inf)
    spacing = 0.0
    t = np.linspace(0.0, 1.0, per_arc + 1)[:, None]
    for row in region.edges:
        u, v = row[0:3], row[3:6]
        theta = np.arccos(np.clip(u @ v, -1.0, 1.0))
        s = (np.sin((1.0 - t) * theta) * u[None] + np.sin(t * theta) * v[None]) / np.sin(theta)
        spacing = max(spacing, theta / per_arc)
        for b in range(0, len(p), 4000):
            d = np.linalg.norm(p[b:b + 4000, None, :] - s[None], axis=2).min(axis=1)
            best[b:b + 4000] = np.minimum(best[b:b + 4000], d)
    return best, spacing


# -------------------------------------------------------------------------------------------------------------- the nodes
def special_nodes(edges, anchor, radius=R_EARTH):
    """Nodes on the statement's edges: on a vertex, on an edge's great circle inside and outside the arc, at the anchor and its
    antipode, at r = 0, with NaN and inf coordinates, and nodes whose arc to the anchor passes exactly through a vertex, built
    from the vertex's own bits (the vertex mirrored in the anchor's direction: 2 (a.v) v - a lies on their great circle beyond
    v; and the vertex's bits scaled by powers of two, which normalise back to the same bits)."""
    out = [anchor * radius, -anchor * radius, np.zeros(3), np.array([np.nan, 1.0, 2.0]), np.array([1.0, np.inf, 2.0]),
           np.array([-np.inf, 0.0, 0.0]), anchor * 2.0 ** -501, anchor * 2.0 ** -499]
    for row in edges[:: max(1, len(edges) // 6)]:
        U, V = row[0:3], row[3:6]
        mid = U + V
        out += [U * radius, U * 4.0, V * 0.5, mid * radius, (2.0 * U - V) * radius, (2.0 * V - U) * radius,
                (2.0 * (anchor @ U)) * U - anchor, ((2.0 * (anchor @ V)) * V - anchor) * radius, -U * radius]
    return np.array(out)


def node_groups(ngroups, P, edges, anchor, seed, spread_deg=40.0, centre=(20.0, 30.0)):
    """f64[ngroups, P, 3] (P = 1: [ngroups, 3]): small elements scattered over a cap about ``centre`` at Earth radii, with
    :func:`special_nodes` written over the leading nodes."""
    rng = np.random.default_rng(seed)
    c = RG.unit_vectors(np.array([centre]))[0]
    cen = c[None] + np.tan(np.deg2rad(spread_deg)) * 0.5 * rng.standard_normal((ngroups, 3))
    cen /= np.linalg.norm(cen, axis=1)[:, None]
    pts = cen[:, None, :] * rng.uniform(0.9, 1.0, (ngroups, 1, 1)) + 0.02 * rng.standard_normal((ngroups, P, 3))
    pts *= R_EARTH
    flat = pts.reshape(-1, 3)
    sp = special_nodes(edges, anchor) if len(edges) else special_nodes(np.zeros((0, 9)), anchor)
    k = min(len(sp), len(flat))
    flat[:k] = sp[:k]
    return np.ascontiguousarray(pts if P > 1 else pts.reshape(ngroups, 3))


# ------------------------------------------------------------------------------------------------------------ the big case
def big_region():
    """2 * 256 * 32 + 7 edges: 513 chunks, three batches of the device's chunk loop (256, 256 and 1)."""
    return region_with(2 * 256 * CHUNK + 7, radius_deg=12.0, wiggle=0.2, lobes=7)


def chunk_balls(edges, anchor):
    """(C f64[K, 3], Rc f64[K], n = a x C f64[K, 3]) of the chunks of 32 edges as multimesh_amd/csrc/mm_regions.hip forms them
    (the centre of the box of the chunk's ends; the largest |M_e - C| + |U_e - V_e| / 2, rounded up): where the rims of the
    device's tile tests lie.  Only the placement of test nodes depends on it, no expected value."""
    K = -(-len(edges) // CHUNK)
    C, Rc = np.zeros((K, 3)), np.zeros(K)
    for k in range(K):
        rows = edges[k * CHUNK:(k + 1) * CHUNK]
        ends = np.concatenate([rows[:, 0:3], rows[:, 3:6]])
        C[k] = 0.5 * (ends.min(axis=0) + ends.max(axis=0))
        mid = 0.5 * (rows[:, 0:3] + rows[:, 3:6])
        Rc[k] = (np.linalg.norm(mid - C[k], axis=1) + 0.5 * np.linalg.norm(rows[:, 0:3] - rows[:, 3:6], axis=1)).max()
    return C, Rc * (1.0 + 2.0 ** -40) + 2.0 ** -45, np.cross(anchor[None], C)


def _bisect(f, lo, hi, target):
    """t in [lo, hi] with f(t) nearest ``target``, f monotone."""
    rising = f(hi) > f(lo)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if (f(mid) < target) == rising:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def tile_rim_groups(edges, anchor, cutoff, nodes=16, chunks=(0, 100, 255, 256, 300, 512)):
    """Groups f64[G, nodes, 3] that are each a whole tile of their own call, a cluster a few ulp wide, so that the tile's ball is
    (the node, ~0): placed where the device's tile tests turn over for one chunk -- |C - T| at Rc + sqrt(cutoff^2 + 2^-20), one
    step inside, on it and one step outside, and T . (a x C) at +-Rc |m| likewise --, by bisection along a great circle."""
    C, Rc, ncap = chunk_balls(edges, anchor)
    reach = np.sqrt(cutoff * cutoff + 2.0 ** -20)
    out = []
    for k in chunks:
        c = C[k] / np.linalg.norm(C[k])
        away = np.cross(np.cross(c, anchor), c)
        away /= np.linalg.norm(away)
        along = lambda t: np.cos(t) * c + np.sin(t) * away               # leaves the chunk along the great circle through the anchor
        t0 = _bisect(lambda t: np.linalg.norm(along(t) - C[k]), 0.0, 1.0, Rc[k] + reach)
        side = np.cross(c, away)
        across = lambda t: np.cos(t) * c + np.sin(t) * side              # leaves the plane of the anchor's great circle sideways
        nk = ncap[k]
        t1 = _bisect(lambda t: abs(across(t) @ nk), 0.0, 0.5, Rc[k])
        for centre in [along(t0 * f) for f in (1.0 - 1e-9, 1.0 - 2e-16, 1.0, 1.0 + 2e-16, 1.0 + 1e-9)] + \
                      [across(s * t1 * f) for s in (1.0, -1.0) for f in (1.0 - 1e-9, 1.0, 1.0 + 1e-9)]:
            group = np.repeat(centre[None], nodes, axis=0)
            group[1::2] *= 1.0 + 2.0 ** -52 * np.arange(1, nodes // 2 + 1)[:, None]      # the same direction within an ulp or two
            out.append(group * R_EARTH)
    return np.array(out)


# ---------------------------------------------------------------------------------------------------------- guarded cases
def guarded_cases():
    """Points, the edge table and the outputs sized to a granule, to neither and to whole pages; the edge count leaves a
    partial last chunk whose LAST edge sets some node's distance and some node's crossing (:func:`guarded_last_edge`)."""
    out = []
    for n, P, nedges in ((8, 1, CHUNK + 2), (101, 1, 2 * CHUNK + 7), (1024, 1, 512), (9 * 27, 27, CHUNK + 1), (2 * 125, 125, 3 * CHUNK + 5),
                         (4096, 1, 2 * CHUNK + 1)):
        reg = region_with(nedges)
        G = n // P
        pts = node_groups(G, P, reg.edges, reg.anchor, seed=n + nedges, spread_deg=25.0)
        flat = pts.reshape(-1, 3)
        U, V = reg.edges[-1, 0:3], reg.edges[-1, 3:6]
        mid = (U + V) / np.linalg.norm(U + V)
        flat[-1] = (mid + 1e-4 * reg.edges[-1, 6:9]) * R_EARTH          # next to the last edge: it sets the distance
        flat[-2] = (2.0 * (reg.anchor @ mid) * mid - reg.anchor) * 3.0  # beyond its midpoint as seen from the anchor: it is crossed
        out.append(dict(name=f"n={n} P={P} E={nedges}", points=pts, edges=reg.edges, anchor=reg.anchor, anchor_inside=reg.anchor_inside,
                        cutoff=0.2, scale=R_EARTH, arrays=dict(points=pts, edges=reg.edges, signed=np.zeros(n), inside=np.zeros(n, np.int32))))
    return out


def guarded_last_edge(case):
    """How many nodes the last edge alone decides: (distance, crossing)."""
    full = region_distance(case["points"], case["edges"], case["anchor"], case["anchor_inside"], case["cutoff"], case["scale"])
    less = region_distance(case["points"], case["edges"][:-1], case["anchor"], case["anchor_inside"], case["cutoff"], case["scale"])
    return int((np.abs(full[0]) != np.abs(less[0])).sum()), int((full[1] != less[1]).sum())
