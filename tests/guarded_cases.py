"""The inputs of the tests/test_*_guarded_gpu.py files that run the model-tool kernels under MM_GUARD_ALLOC=1, stated once in
plain NumPy, and the counts tests/test_guarded_cases.py asserts on them without a GPU.  The builders and the statements are
those of the units' own ``*_cases.py`` modules; the GLL meshes and the Earth chunk come from the package's host-side
generators (multimesh_amd.synth, NumPy alone), as in the units' own tests.  No kernel runs here.

Under MM_GUARD_ALLOC every device array ends at the end of its mapping, rounded up to 16 bytes.  An array whose byte count
is a multiple of 16 has nothing behind its last element; one whose count is not has up to 8 bytes of slack that would hide
an 8-byte over-read.  So every unit's cases span three classes of byte counts (:func:`byte_class`): ``pages`` (a whole
number of 4096-byte pages), ``granule`` (a multiple of 16 that is no whole page) and ``neither``.  The radial tables are
held to at most five knots, so they span ``granule`` (an even count) and ``neither`` only; a coefficient array
f64[NC, m, 2, NLM] is a multiple of 16 bytes whatever its shape.

A case is a dict: ``name``, the inputs, and ``arrays`` = {what the kernel reads through a pointer: the host array}.
"""
import numpy as np

import frames_cases as FC
import grid_adjoint_cases as GA
import grid_import_cases as GI
import harmonic_cases as HC
import layered_cases as LC
import order_cases as OC
import radial_cases as RC
import scattered_cases as SC

PAGE, GRANULE = 4096, 16
# kThreads of multimesh_amd/csrc/mm_stream.h, the lanes of a workgroup: a tile of mm_gll_tile.h holds TILE = kThreads / P
# whole elements (Tile::TILE, "static constexpr int TILE = kThreads / P", and RunTile::tile for a run-time P).  The Python
# layer exposes no constant for it; mass_cases.tile_elems and order_cases.tile_elems state the same quotient.
TILE_LANES = 256
N_POINTS = (8, 101, 1024)            # P = 1 clouds: 24 N bytes of points = granule, neither, six pages
ORDERS = (1, 2, 4)


def byte_class(nbytes):
    return "pages" if nbytes % PAGE == 0 else "granule" if nbytes % GRANULE == 0 else "neither"


def classes(cases, what):
    """The byte classes the array ``what`` takes over the cases that have it."""
    return {byte_class(c["arrays"][what].nbytes) for c in cases if what in c["arrays"]}


def tile(P):
    return TILE_LANES // P


def around_a_tile(P):
    """Element counts of one tile minus one, exactly one tile, and one tile plus one."""
    t = tile(P)
    return [n for n in (t - 1, t, t + 1) if n >= 1]


# ------------------------------------------------------------------------------------------------ radial and harmonics
def table_radii(m):
    """The mantle table of harmonic_cases with the 670 repeated: 4 rows (32 bytes) or 5 (40 bytes)."""
    assert m in (4, 5)
    return HC.knots(m)


def edge_cloud(n, R, seed):
    """n >= 8 points f64[n, 3], generic but for the first six, which lie on a coordinate axis so that |p| is the radius
    itself: the top knot, the bottom knot, the discontinuity, above the top, below the bottom, the discontinuity again."""
    pts = HC.cloud(n, seed, R[0], R[-1])
    pts[0] = [0.0, 0.0, R[-1]]
    pts[1] = [0.0, R[0], 0.0]
    pts[2] = [HC.R_670, 0.0, 0.0]
    pts[3] = [0.0, 0.0, -(R[-1] + 1e5)]
    pts[4] = [R[0] - 1e5, 0.0, 0.0]
    pts[5] = [0.0, -HC.R_670, 0.0]
    return np.ascontiguousarray(pts)


def edge_elements(G, P, R, seed):
    """G elements of P nodes f64[G, P, 3]: generic, but element 0 spans the lower layer and reaches below the table (its
    first node is clamped to the bottom knot) and element 1 spans the upper layer and reaches above it (its last node is
    clamped to the top knot).  The exception to "every edge kind in every case": with G = 1 (one tile minus one at
    P = 125) the one element is the upper one -- its centre picks ONE layer and every node is clamped to it, so a single
    element cannot reach the bottom knot and the top knot both; the top is the row behind which nothing is mapped."""
    pts = HC.elements(G, P, seed, r_lo=R[0], r_hi=R[-1])
    upper = HC.shell_element(P, HC.R_670 + 1e4, R[-1] + 1e5, seed)
    lower = HC.shell_element(P, R[0] - 1e5, HC.R_670 - 1e4, seed + 1)
    if G >= 2:
        pts[0], pts[1] = lower, upper
    else:
        pts[0] = upper
    return np.ascontiguousarray(pts)


def radial_edge_counts(points, R):
    """How many nodes the statement places on each edge: by its own interval index and weight (harmonic_cases.intervals
    with the edge extended is mm_radial_model_apply's rule)."""
    pts = points if points.ndim == 3 else points[:, None, :]
    m = len(R)
    i, t, _, _ = HC.intervals(pts, R, True)
    r = HC.radius(pts).reshape(i.shape)
    return {"top": int(((i == m - 2) & (t == 1.0)).sum()), "bottom": int(((i == 0) & (t == 0.0)).sum()),
            "discontinuity": int((r == HC.R_670).sum()), "above": int((r > R[-1]).sum()), "below": int((r < R[0]).sum())}


def radial_cases():
    """mm_radial_bins, mm_binned_weighted_sum and mm_radial_model_apply."""
    out = []
    for q, n in enumerate(N_POINTS):
        m, nbins = (4, 3) if q % 2 == 0 else (5, 4)          # edges: 4 values (32 bytes) or 5 (40 bytes)
        R = table_radii(m)
        rng = np.random.default_rng(70 + n)
        pts = edge_cloud(n, R, seed=n)
        edges = np.linspace(R[0], R[-1], nbins + 1)
        values = rng.uniform(3000.0, 9000.0, (2, m))
        mass, fields = rng.uniform(0.5, 2.0, n), rng.standard_normal((2 + n % 2, n))
        bins = RC.bins(pts, edges)[0]
        out.append(dict(name=f"cloud n={n} m={m} nbins={nbins}", points=pts, radius=R, values=values, edges=edges, nbins=nbins,
                        mass=mass, fields=fields, values_in=rng.standard_normal((2, n)),
                        arrays=dict(points=pts, radius=R, values=values, edges=edges, mass=mass, fields=fields, bins=bins)))
    for P in (8, 27, 125):
        for G in around_a_tile(P):
            R = table_radii(4 + G % 2)
            rng = np.random.default_rng(G * P)
            pts = edge_elements(G, P, R, seed=G + P)
            values = rng.uniform(3000.0, 9000.0, (3, len(R)))
            out.append(dict(name=f"elements G={G} P={P} m={len(R)}", points=pts, radius=R, values=values,
                            values_in=rng.standard_normal((3, G * P)), arrays=dict(points=pts, radius=R, values=values)))
    return out


def bin_edge_counts(case):
    r, e = RC.radius(case["points"]), case["edges"]
    return {"first edge": int((r == e[0]).sum()), "last edge": int((r == e[-1]).sum()), "below": int((r < e[0]).sum()),
            "above": int((r > e[-1]).sum())}


LMAX = (0, 1, 8, 40)               # 40: the largest degree at which tests/test_harmonics.py validates the statement


def harmonic_cases():
    """mm_harmonic_model_apply: (points, radius, coef, lmax) with 1 to 5 components (5: four and one more launch)."""
    out = []
    for n, L, m, nc in ((8, 0, 4, 1), (101, 1, 5, 2), (1024, 8, 5, 5), (101, 40, 4, 1)):
        R = table_radii(m)
        pts = edge_cloud(n, R, seed=n + L)
        coef = HC.coefficients(L, m, nc, seed=L)
        vin = np.random.default_rng(L).standard_normal((nc, n))
        out.append(dict(name=f"cloud n={n} lmax={L} m={m} nc={nc}", points=pts, radius=R, coef=coef, lmax=L, values_in=vin,
                        arrays=dict(points=pts, radius=R, coef=coef, values_in=vin)))
    for G, L in zip(around_a_tile(27), (8, 1, 8)):
        R = table_radii(4 + G % 2)
        pts = edge_elements(G, 27, R, seed=G)
        coef = HC.coefficients(L, len(R), 3, seed=G)
        vin = np.random.default_rng(G).standard_normal((3, G * 27))
        out.append(dict(name=f"elements G={G} P=27 lmax={L} m={len(R)}", points=pts, radius=R, coef=coef, lmax=L, values_in=vin,
                        arrays=dict(points=pts, radius=R, coef=coef, values_in=vin)))
    return out


def harmonic_adjoint_cases():
    """mm_harmonic_model_transpose: node counts in the low thousands at the most (the statement is a cumulative sum per
    (l, k)).  ``limits``: the scratch limits the case runs at (0: the library's own); the small limit is the slab of ONE
    order-0 pass of one component, 32 (m - 1) (lmax + 1) bytes for one segment, so every order is a pass of its own."""
    out = []
    for n, L, m, nc in ((8, 0, 4, 1), (8, 1, 5, 3), (101, 8, 5, 3), (1024, 1, 4, 2), (101, 40, 4, 1)):
        R = table_radii(m)
        pts = edge_cloud(n, R, seed=n + L)
        rng = np.random.default_rng(n + L)
        values, weight = rng.standard_normal((nc, n)), rng.uniform(0.5, 2.0, n)
        limits = (0, 32 * (m - 1) * (L + 1)) if n == 8 and L == 1 else (0,)
        out.append(dict(name=f"cloud n={n} lmax={L} m={m} nc={nc}", points=pts, radius=R, lmax=L, values=values, weight=weight,
                        limits=limits, arrays=dict(points=pts, radius=R, values=values, weight=weight)))
    for G in around_a_tile(27):
        R = table_radii(4 + G % 2)
        pts = edge_elements(G, 27, R, seed=G)
        rng = np.random.default_rng(G)
        values, weight = rng.standard_normal((2, G * 27)), rng.uniform(0.5, 2.0, G * 27)
        out.append(dict(name=f"elements G={G} P=27 lmax=8 m={len(R)}", points=pts, radius=R, lmax=8, values=values,
                        weight=weight, limits=(0,), arrays=dict(points=pts, radius=R, values=values, weight=weight)))
    return out


# --------------------------------------------------------------------------------------------------------------- layered
BOTTOM = 60000.0                 # the last interface of every column of the layered cases, m: below every other interface


def layered_model(kind, ncomp):
    """(lat, lon, bounds, values, periodic): ``regional`` with even axes (6 and 8 values: the last row and column end a
    granule), ``odd`` (7 and 9), ``global`` (6 latitudes, 12 + 1 longitudes once round).  nb = 5: layer 1 is pinched out
    over the south; the last interface is flat at BOTTOM, so a depth can equal it."""
    if kind == "global":
        lat, lon, bounds, values = LC.global_model(5, ncomp, seed=2)
    elif kind == "regional":
        lat, lon, bounds, values = LC.layered_tables(LC.REGIONAL_LAT[:6], LC.REGIONAL_LON[:8], 5, ncomp, seed=1)
    else:
        lat, lon, bounds, values = LC.regional(5, ncomp, seed=3)
    bounds = bounds.copy()
    bounds[..., -1] = BOTTOM
    assert (np.diff(bounds, axis=2) >= 0.0).all()
    return lat, lon, bounds, values, kind == "global"


def layered_points(kind, G, P, seed):
    """f64[G, P, 3] (P = 1: a cloud f64[G, 3]): past every edge of a regional map, all round a global one; the first
    nodes lie on the x axis (latitude and longitude 0) at depths equal to the last interface, below it and above the top."""
    box = dict(lat=(-89.0, 89.0), lon=(-180.0, 180.0)) if kind == "global" else {}
    pts = LC.elements(G, P, seed=seed, **box) if P > 1 else LC.elements(G, 1, seed=seed, height=0.0, size=0.0, **box).reshape(G, 3)
    flat = pts.reshape(-1, 3)
    for q, depth in enumerate((BOTTOM, BOTTOM + 5000.0, -5000.0)):
        flat[q] = [LC.R_EARTH - depth, 0.0, 0.0]
    # in (or clamped onto) the last row and the last column -- on a global map the cell that closes the round --, and over
    # the south, where layer 1 is pinched out
    flat[3] = LC.xyz(80.0, 179.0, 10000.0) if kind == "global" else LC.xyz(7.5, 7.5, 10000.0)
    flat[4] = LC.xyz(-80.0, -100.0, 10000.0) if kind == "global" else LC.xyz(-5.0, -5.0, 10000.0)
    return np.ascontiguousarray(pts)


def layered_cases():
    """mm_layered_model_apply; the test runs every case in both lateral modes, both picks and fill and clamp."""
    out = []
    for kind, G, P, ncomp in (("regional", 8, 1, 2), ("odd", 101, 1, 3), ("global", 1024, 1, 5), ("global", 101, 1, 1),
                              ("regional", tile(27) - 1, 27, 3), ("odd", tile(27), 27, 4), ("global", tile(27) + 1, 27, 2),
                              ("regional", tile(125) + 1, 125, 1)):
        lat, lon, bounds, values, periodic = layered_model(kind, ncomp)
        pts = layered_points(kind, G, P, seed=G + P)
        out.append(dict(name=f"{kind} G={G} P={P} ncomp={ncomp}", points=pts, lat=lat, lon=lon, bounds=bounds, values=values,
                        periodic=periodic, arrays=dict(points=pts, lat=lat, lon=lon, bounds=bounds, values=values)))
    return out


def layered_edge_counts(case):
    """By the statement's own cells (layered_cases.cell through model_apply's steps) on NumPy's coordinates: the device's
    differ from them by a rounding of acos / atan2, which moves no node across the map's edge by more than that."""
    flat = case["points"].reshape(-1, 3)
    lld = LC.latlondepth(flat)
    lat, lon = case["lat"], case["lon"]
    if case["periodic"]:
        lld[:, 1] = LC.wrap(lld[:, 1], lon[0])
    ca, co = LC.cell(lat, lld[:, 0], True), LC.cell(lon, lld[:, 1], True)
    b = LC.columns(case["bounds"], ca, co, LC.CELL)
    counts = {"last row": int((ca[1] == len(lat) - 1).sum()),
              "last column": int((co[1] == len(lon) - 1).sum()),
              "bottom": int((lld[:, 2] == b[:, -1]).sum()), "below": int((lld[:, 2] > b[:, -1]).sum()),
              "pinched": int((b[:, 1] == b[:, 2]).sum())}
    if case["periodic"]:
        counts["seam"] = int((co[0] == len(lon) - 2).sum())          # the cell that closes the round
    else:
        counts["axis end"] = int(((co[0] == len(lon) - 2) & (co[2] == 1.0)).sum())   # clamped onto the last column
    return counts


# ---------------------------------------------------------------------------------------------------------------- frames
def frames_cases():
    """mm_rotate_points on n points (n odd: 3 n doubles end on no granule), mm_rotate_vectors and mm_local_components on
    planes [3, E, P] and on MODEL/data rows [E, 5, P] whose last row is the last of the array."""
    out = []
    for n in (1, 2, 101, 512):
        out.append(dict(name=f"points n={n}", matrix=FC.matrix(n), points=FC.cloud(n, seed=n), arrays={}))
        out[-1]["arrays"]["points"] = out[-1]["points"]
    for E, P in ((1, 1), (3, 27), (2, 125), (101, 1), (512, 8)):
        v = FC.vectors((E, P), seed=E + P)
        rows = FC.rows_of(v, 5, (3, 0, 4), seed=P)
        pos = FC.cloud(E * P, seed=E * P).reshape(E, P, 3)
        out.append(dict(name=f"vectors E={E} P={P}", matrix=FC.matrix(E + P), planes=v, rows=rows, cols=(3, 0, 4), positions=pos,
                        arrays=dict(planes=v, rows=rows, positions=pos)))
    return out


# ------------------------------------------------------------------------------------------------------------- scattered
NSRC = 5


def scattered_cases():
    """mm_idw_gather on brute-force rows (scattered_cases.knn): k = 1, k = 2 (the paired row reader, whose
    last pair ends no page at odd N), k = nsrc and k > nsrc (padded rows); the last target
    is the last source (an exact hit on index nsrc - 1); ``cut`` lies between the nearest distances, so some targets lose
    every sample."""
    src, fields = SC.cloud(NSRC, ncomp=5, seed=11)
    out = []
    for n in N_POINTS:
        tgt = SC.targets(n, seed=n)
        tgt[-1] = src[-1]
        for k in (1, 2, NSRC, NSRC + 3):
            idx, dist = SC.knn(src, tgt, k)
            cut = float(np.median(dist[:, 0]))
            nc = 1 + (n + k) % 5
            out.append(dict(name=f"n={n} k={k} ncomp={nc}", fields=np.ascontiguousarray(fields[:nc]), idx=idx, dist=dist, k=k, cut=cut,
                            arrays=dict(fields=np.ascontiguousarray(fields[:nc]), idx=idx, dist=dist)))
    return out


# -------------------------------------------------------------------------------------------------- the GLL tile kernels
def gll_points(order, dim, nelem, seed=3):
    """The first ``nelem`` elements of a jittered GLL mesh, f64[nelem, (order + 1)^dim, dim]."""
    from multimesh_amd import synth

    side = 2
    while (side - 1) ** dim < nelem:
        side += 1
    return np.ascontiguousarray(synth.gll_mesh(side, order, seed=seed, dim=dim)[:nelem])


def order_cases():
    """mm_gll_tensor_apply: (order_in, order_out, dim, nelem) with nelem around the tile of 256 // max(P_in, P_out), three
    components; the test runs every case in the three layouts, plain and with the transposed table, scale_in and div_out.
    The last case fills whole pages."""
    out = []
    shapes = [(oi, oo, dim, E) for dim in (2, 3) for oi, oo in ((1, 2), (4, 1), (2, 4))
              for E in around_a_tile(max((oi + 1) ** dim, (oo + 1) ** dim))] + [(1, 2, 3, 512)]
    for oi, oo, dim, E in shapes:
        pin, pout = (oi + 1) ** dim, (oo + 1) ** dim
        rng = np.random.default_rng(100 * oi + 10 * oo + dim + E)
        planes = rng.standard_normal((3, E, pin))
        scale, div = rng.uniform(0.5, 2.0, (E, pin)), rng.uniform(0.5, 2.0, (E, pout))
        out.append(dict(name=f"{oi}->{oo} dim={dim} E={E}", order_in=oi, order_out=oo, dim=dim, planes=planes, scale_in=scale,
                        div_out=div, arrays=dict(values=planes, scale_in=scale, div_out=div, table=OC.table(oi, oo))))
    return out


def deviation_cases():
    """mm_element_deviation: two coordinate arrays f64[E, P, dim] of the same elements."""
    out = []
    for order, dim, E in ((1, 2, 1), (2, 3, 101), (4, 3, 2), (1, 3, 512)):
        b = gll_points(order, dim, E)
        a = b + np.random.default_rng(E).normal(size=b.shape) * 1e-9
        out.append(dict(name=f"order={order} dim={dim} E={E}", a=a, b=b, arrays=dict(a=a, b=b)))
    return out


def gradient_cases():
    """mm_gll_gradient: orders 1, 2, 4 in 2-D and 3-D at one tile minus one, one tile and one tile plus one element, two
    or three components; the last case fills whole pages."""
    out = []
    shapes = [(o, dim, E) for dim in (2, 3) for o in ORDERS for E in around_a_tile((o + 1) ** dim)] + [(1, 3, 512)]
    for order, dim, E in shapes:
        gp = gll_points(order, dim, E)
        u = np.random.default_rng(order + dim + E).standard_normal((2 + E % 2,) + gp.shape[:2])
        out.append(dict(name=f"order={order} dim={dim} E={E}", order=order, dim=dim, points=gp, u=u, arrays=dict(points=gp, u=u)))
    return out


def diffusion_cases():
    """mm_gll_diffusion_apply: orders 1, 2, 4 in 2-D and 3-D around a tile, two or three components, element-nodal
    diffusivities kappa_h (and kappa_r in 3-D); the statement is diffusion_cases.apply.  The last case fills whole pages."""
    out = []
    shapes = [(o, dim, E) for dim in (2, 3) for o in ORDERS for E in around_a_tile((o + 1) ** dim)] + [(1, 3, 512)]
    for order, dim, E in shapes:
        gp = gll_points(order, dim, E, seed=5)
        rng = np.random.default_rng(7 * order + dim + E)
        u = rng.standard_normal((2 + E % 2,) + gp.shape[:2])
        kh, kr = rng.uniform(0.5, 2.0, gp.shape[:2]), rng.uniform(0.0, 2.0, gp.shape[:2])
        out.append(dict(name=f"order={order} dim={dim} E={E}", order=order, dim=dim, points=gp, u=u, kappa_h=kh, kappa_r=kr,
                        arrays=dict(points=gp, u=u, kappa_h=kh, kappa_r=kr)))
    return out


def pcg_cases():
    """The streaming kernels of the PCG loop (mm_pcg_combine, _scalars, _direction, _advance): n values per system, three
    systems whose state block f64[3, 8] ends a granule; the last system is the active one, its slots the block's last."""
    out = []
    for n in N_POINTS:
        rng = np.random.default_rng(n)
        mass = rng.uniform(0.5, 1.5, n)
        p, kp, z, x, r = (rng.standard_normal((3, n)) for _ in range(5))
        out.append(dict(name=f"n={n}", mass=mass, p=p, kp=kp, z=z, x=x, r=r, arrays=dict(mass=mass, p=p, kp=kp, z=z, x=x, r=r)))
    return out


# --------------------------------------------------------------------------------------------------------- grid operator
def grid_operator_cases():
    """mm_grid_operator and its transpose.  ``plain``: ascending axes of even lengths (6, 10, 12: the last node of an axis
    ends a granule), points past every face of the box.  ``global``: the CALLER's axes descend in depth and latitude and go
    once round in longitude without the closing column; ``axes`` are the prepared ones (grid_adjoint_cases.to_prepared's
    layout: ascending, column 0 repeated last), ``flipped`` / ``appended`` what the fold undoes.  Point 0 lies inside the
    last cell of all three axes; on the global map that is the cell that closes the round."""
    out = []
    for n in N_POINTS:
        depth, lat, lon = GI.DEPTH[:6].copy(), np.linspace(-6.0, 6.0, 10), np.linspace(-5.5, 6.5, 12)
        pts = GA.random_points(n, depth, lat, lon, 0.075, seed=n)
        pts[0] = GA.xyz(0.5 * (lat[-2] + lat[-1]), 0.5 * (lon[-2] + lon[-1]), 0.5 * (depth[-2] + depth[-1]))[0]
        pts[1] = GA.xyz(lat[-1] + 1.0, 0.0, 1000.0)[0]          # past the last latitude: outside
        v = np.random.default_rng(n).standard_normal((1 + n % 2 * 2, n))
        out.append(dict(name=f"plain n={n}", axes=(depth, lat, lon), caller=(depth, lat, lon), periodic=False,
                        flipped=(False, False, False), appended=False, points=pts, values=v,
                        arrays=dict(points=pts, depth=depth, lat=lat, lon=lon, values=v)))
        cdepth, clat, clon = np.array([2.0e6, 1.0e6, 3.0e5, -1.0e5]), np.linspace(90.0, -90.0, 7), np.arange(0.0, 360.0, 30.0)
        depth, lat, lon = cdepth[::-1].copy(), clat[::-1].copy(), np.concatenate([clon, [360.0]])
        pts = GI.sphere_points(n, seed=n + 1, rmin=4.2e6)
        pts[0] = GA.xyz(80.0, 345.0, 1.5e6)[0]
        pts[1] = GA.xyz(-30.0, 359.0, 5.0e5)[0]
        pts[2] = GA.xyz(0.0, 100.0, 2.1e6)[0]                   # below the deepest node: outside
        out.append(dict(name=f"global n={n}", axes=(depth, lat, lon), caller=(cdepth, clat, clon), periodic=True,
                        flipped=(True, True, False), appended=True, points=pts, values=v,
                        arrays=dict(points=pts, depth=depth, lat=lat, lon=lon, values=v)))
    return out


def grid_operator_edge_counts(case):
    """By the statement's own corner indices (grid_adjoint_cases.operator) on NumPy's coordinates."""
    depth, lat, lon = case["axes"]
    lld = GI.latlondepth(case["points"])
    ids, w, nout, inside = GA.operator(depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1], False, case["periodic"])
    top = ids[inside, 7]                                         # corner (k1, j1, i1)
    k1, j1, i1 = top // (len(lat) * len(lon)), top // len(lon) % len(lat), top % len(lon)
    counts = {"last depth cell": int((k1 == len(depth) - 1).sum()), "last latitude cell": int((j1 == len(lat) - 1).sum()),
              "last longitude cell": int((i1 == len(lon) - 1).sum()), "last value of the cube": int((top == ids.max()).sum()),
              "outside": nout}
    assert ids.max() <= len(depth) * len(lat) * len(lon) - 1
    if case["periodic"]:
        counts["seam"] = counts.pop("last longitude cell")
        counts["flipped axes"] = sum(case["flipped"])
    else:
        counts["corner of the box"] = int(top[0] == len(depth) * len(lat) * len(lon) - 1)
    return counts


# ---------------------------------------------------------------------------------------------------------------- sphere
def sphere_cases():
    """mm_map_to_sphere, mm_sphere_ratio, mm_scale_points and mm_first_occurrence.  Element-nodal: n points, one radius
    each.  Node layout: n nodes named by a connectivity int64[E, 8] (64 E bytes: a granule or whole pages) whose LAST
    entry is the only one that names the last node, so that node reads rad[nrad - 1], the last radius.  Point 2 is the
    centre (left alone)."""
    out = []
    for n in N_POINTS:
        rng = np.random.default_rng(n)
        pts = rng.uniform(-6.4e6, 6.4e6, (n, 3))
        pts[2] = 0.0
        E = 192 if n == 1024 else -(-(n + 24) // 8)          # 12288 bytes: three pages
        flat = np.concatenate([np.arange(n - 1), rng.integers(0, n - 1, 8 * E - n), [n - 1]])
        conn = np.ascontiguousarray(flat.reshape(E, 8).astype(np.int64))
        rad_en, rad_node = rng.uniform(0.5, 1.0, n), rng.uniform(0.5, 1.0, (E, 8))
        out.append(dict(name=f"n={n}", points=pts, rad=rad_en, connectivity=conn, rad_nodal=rad_node,
                        arrays=dict(points=pts, rad=rad_en, connectivity=conn, rad_nodal=rad_node)))
    return out


# ---------------------------------------------------------------------------------------------------------- regular grid
REGULAR_GRID = dict(lat_extent=(-9.0, 9.0, 5), lon_extent=(-8.5, 9.5, 6), depth_extent=(0.0, 380_000.0, 5))
REGULAR_CHUNK = 64                   # 150 targets: chunks of 64, 64 and 22 -- the last one is partial
SEARCH = 25


def regular_grid_cases():
    """mm_sample_columns_gll through extract_regular_grid on a small Earth chunk, orders 1, 2, 4: 5 x 6 columns past the
    chunk's +-8 degrees (those targets are missing), 5 depths down to 380 km, three fields."""
    from multimesh_amd import synth

    out = []
    for order in ORDERS:
        c = synth.earth_chunk(order, nlat=4, nlon=4, lat=(-8.0, 8.0), lon=(-8.0, 8.0), ellipticity=3.35e-3, topography=3e-4)
        gp = c["points"]
        f = np.ascontiguousarray(np.stack([synth.field_linear(gp / 1e6), np.linalg.norm(gp, axis=-1) / 6371000.0,
                                           synth.field_smooth(gp.reshape(-1, 3) / 1e6).reshape(gp.shape[:2])]))
        lat, lon, depth = (np.linspace(*REGULAR_GRID[k]) for k in ("lat_extent", "lon_extent", "depth_extent"))
        out.append(dict(name=f"order={order}", order=order, points=gp, fields=f, lat=lat, lon=lon, depth=depth,
                        arrays=dict(points=gp, fields=f, depth=depth)))
    return out


def regular_grid_oracle(case, targets):
    """(values f64[3, N], found bool[N], nmissing) of the CPU oracle at the generated targets f64[N, 3]: the centroid as the
    device forms it, its k nearest, the acceptance loop and the weighted sums (as tests/test_regular_grid_gpu.py)."""
    from oracle import oracle as O

    gp = case["points"]
    cen = gp[:, 0].copy()
    for p in range(1, gp.shape[1]):
        cen = cen + gp[:, p]
    cen = cen / gp.shape[1]
    nn, _ = O.knn_ckdtree(cen, targets, SEARCH)
    elem, co, miss = O.locate_gll(case["order"], nn, gp, targets, tolerance=1.05)
    found = elem >= 0
    return O.gather_elem(case["fields"], elem, co).T, found, miss
