"""The four randomised checks (kNN, the fused hex8 pipeline, the GLL locate, unique points): one home for drawing a case
and for checking it.  tools/fuzz_*.py are loops over this module at today's sizes (budget "tool", and "big" for the
pipeline); tests/test_fuzz_gpu.py runs a seeded slice at the "suite" sizes; tests/test_fuzz_cases.py checks the
generators and the oracles on the CPU.

draw_<name>(rng, budget) -> a plain dict of NumPy arrays and parameters; no GPU, no Context.  With budget "tool" (and
"big") the draws from `rng` come in exactly the order of the tools' former loop bodies, the data drawn between the
parameters included, so a seed and a case number name the same case as ever (tests/golden/fuzz_draws.json).
check_<name>(ctx, case) -> runs the entry points, raises AssertionError whose text is the tool's one-line description of
the case and its diagnosis, and returns {"line": that line, "kernels": Context.last_knn_kernels() of the calls, ...}.

The "suite" budget of the kNN draws two things the tools never do (added to that budget only: the tools' sequences do
not move): the kind "far" -- a uniform or lattice cloud at |lo| / cell of 1e7 or 1e9, one random axis negative, as
test_thin_elements_gpu.far_clouds builds them -- and, with probability 0.25, a FOLLOW-UP case: the previous case's nsrc,
ntgt, dim and k with another kind of cloud (what a verdict cached per (npts, ncells) and a replayed sort must survive).
"""
import numpy as np

from dispatch_cases import WORKERS, knn_distances
from multimesh_amd import synth
from oracle import oracle as O

EPS = 2.220446049250313e-16

# ---------------------------------------------------------------------------------------------------------- sizes
KNN_SIZES = {"tool": (((1, 200), (200, 20_000), (20_000, 400_000)), ((1, 300), (300, 120_000))),
             "suite": (((1, 200), (200, 5_000), (5_000, 40_000)), ((1, 300), (300, 12_000)))}
PIPELINE_SIZES = {"tool": ((4, 42), (1, 60_000)), "big": ((60, 121), (200_000, 2_000_000)), "suite": ((4, 14), (1, 8_000))}
GLL_SIZES = {"tool": ({3: (3, 9), 2: (3, 24)}, (1, 6000)), "suite": ({3: (3, 6), 2: (3, 12)}, (1, 2000))}
UNIQUE_SIZES = {"tool": ((1, 50), (50, 5000), (5000, 1_500_000)), "suite": ((1, 50), (50, 5000), (5000, 60_000))}

# ---------------------------------------------------------------------------------------------------- choice lists
KNN_DIMS = [1, 2, 3, 3, 3]
KNN_KINDS = ["uniform", "clustered", "aniso", "lattice", "graded"]
KNN_MARGINS = [0.0, 0.1, 1.0]
KNN_KS = [1, 2, 3, 4, 7, 8, 13, 16, 20, 24, 25, 31, 32, 33, 40, 64]
FAR_RATIOS = [1e7, 1e9]
FAR_CLOUDS = ["uniform", "lattice"]
FOLLOW_UP_SHARE = 0.25
PIPELINE_MARGINS = [0.0, 0.02, 0.3]
PIPELINE_KS = [1, 2, 3, 4, 5, 8, 9, 13, 16, 20, 24, 25, 32, 33, 40, 64]
PIPELINE_NCOMP = [1, 1, 2, 3, 5]
GLL_ORDERS = [1, 2, 4]
GLL_DIMS = [2, 3]
GLL_MARGINS = [0.0, 0.03, 0.4]
GLL_KS = [1, 2, 5, 9, 12, 20, 27]
GLL_TOLS = [1.0, 1.03, 1.05, 1.2]
GLL_NCOMP = [1, 2]
GLL_FUSED_MIN_JITTER = 0.02        # the fused GLL call is compared on meshes in general position only
UNIQUE_KINDS = ["floats", "few_values", "lattice", "signed", "last_bits"]
HEX_EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]   # exodus order


def _one_of(rng, ranges):
    """One integer from one of `ranges`: an integer of each is drawn, then the choice among them (the tools' order)."""
    return int(rng.choice([rng.integers(a, b) for a, b in ranges]))


# =============================================================================================================== kNN
def _knn_cloud(rng, kind, nsrc, dim, case):
    """The sources of one kind of cloud (lattices fix their own count)."""
    if kind == "uniform":
        return rng.uniform(size=(nsrc, dim))
    if kind == "clustered":
        centres = rng.uniform(size=(int(rng.integers(1, 12)), dim))
        return centres[rng.integers(0, len(centres), size=nsrc)] + rng.normal(scale=rng.uniform(1e-3, 0.1), size=(nsrc, dim))
    if kind == "aniso":
        return rng.uniform(size=(nsrc, dim)) * rng.uniform(1e-2, 50.0, size=dim) + rng.uniform(-1e4, 1e4, size=dim)
    if kind == "lattice":
        m = max(2, int(round(nsrc ** (1.0 / dim))))
        g = np.stack(np.meshgrid(*[np.arange(m, dtype=np.float64)] * dim, indexing="ij"), axis=-1).reshape(-1, dim)
        return g + rng.uniform(-0.2, 0.2, size=g.shape)
    if kind == "graded":
        return rng.uniform(size=(nsrc, dim)) ** rng.uniform(1.0, 2.5)
    assert kind == "far"
    # test_thin_elements_gpu.far_clouds: a unit box whose corner lies ratio cells of 1/32 from the origin
    ratio = float(rng.choice(FAR_RATIOS))
    cloud = str(rng.choice(FAR_CLOUDS))
    if case["follow_up"]:
        cloud = "uniform"                       # (a lattice would change nsrc)
    lo = np.full(dim, ratio * (1.0 / 32))
    axis = int(rng.integers(0, dim))
    lo[axis] = -lo[axis]
    case.update(far_ratio=ratio, far_cloud=cloud, far_axis=axis)
    if cloud == "uniform":
        return lo + rng.uniform(size=(nsrc, dim))
    m = max(2, int(round(nsrc ** (1.0 / dim))))
    g = np.arange(m) / (m - 1)
    return lo + np.stack(np.meshgrid(*([g] * dim), indexing="ij"), axis=-1).reshape(-1, dim)


def draw_knn(rng, budget, prev=None):
    """prev: the case drawn before this one from the same rng ("suite" only: a follow-up case reuses its counts)."""
    src_ranges, tgt_ranges = KNN_SIZES[budget]
    suite = budget == "suite"
    case = {"name": "knn", "budget": budget, "follow_up": False, "far_ratio": None, "far_cloud": None}
    if suite and prev is not None and rng.random() < FOLLOW_UP_SHARE:
        # the same counts, another distribution (not a lattice: it would change nsrc)
        case["follow_up"] = True
        dim, nsrc, ntgt = prev["dim"], prev["nsrc"], prev["ntgt"]
        kind = str(rng.choice([kd for kd in KNN_KINDS + ["far"] if kd not in ("lattice", prev["kind"])]))
    else:
        dim = int(rng.choice(KNN_DIMS))
        nsrc = _one_of(rng, src_ranges)
        ntgt = _one_of(rng, tgt_ranges)
        kind = str(rng.choice(KNN_KINDS + ["far"] if suite else KNN_KINDS))
    src = _knn_cloud(rng, kind, nsrc, dim, case)
    nsrc = len(src)
    lo, hi = src.min(axis=0), src.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    margin = rng.choice(KNN_MARGINS)
    tgt = rng.uniform(lo - margin * span, hi + margin * span, size=(ntgt, dim))
    if rng.random() < 0.3:                      # some targets are sources
        take = rng.integers(0, nsrc, size=min(ntgt, 200))
        tgt[: len(take)] = src[take]
    if case["follow_up"]:
        k = prev["k"]
    else:
        k = min(int(rng.choice(KNN_KS)), nsrc)
    want_dist = bool(rng.random() < 0.5)
    case.update(dim=dim, nsrc=nsrc, ntgt=ntgt, kind=kind, margin=float(margin), k=k, want_dist=want_dist,
                src=np.ascontiguousarray(src), tgt=np.ascontiguousarray(tgt))
    return case


def line_knn(c):
    far = f" far={c['far_cloud']}@{c['far_ratio']:g}" if c.get("far_ratio") else ""
    return (f"case {c.get('case', -1):4d} dim={c['dim']} {c['kind']:9s} nsrc={c['nsrc']:6d} ntgt={c['ntgt']:6d} k={c['k']:2d} "
            f"margin={c['margin']}{far}{' follow-up' if c.get('follow_up') else ''}")


def knn_reference(c):
    """cKDTree's lists of a case (the tools' reference) -> (idx int64[ntgt, k], dist f64[ntgt, k])."""
    from scipy.spatial import cKDTree

    d_ref, i_ref = cKDTree(c["src"]).query(c["tgt"], k=c["k"], workers=WORKERS)
    return np.asarray(i_ref, np.int64).reshape(c["ntgt"], c["k"]), np.asarray(d_ref).reshape(c["ntgt"], c["k"])


def knn_judge(idx, dist, c, i_ref):
    """None, or what is wrong with the lists `idx` (and `dist`, if asked for) of case c against the reference lists:
    distances stated bit for bit (dispatch_cases.knn_distances of the returned ids: the reference's at every rank, and the
    returned distances); a row may differ from the reference's only among exactly equidistant sources -- the same
    distance at that rank, and k distinct ids (test_thin_elements_gpu.knn_check)."""
    src, tgt, nsrc, k = c["src"], c["tgt"], c["nsrc"], c["k"]
    if idx.shape != i_ref.shape:
        return f"lists of shape {idx.shape}, expected {i_ref.shape}"
    if ((idx < 0) | (idx >= nsrc)).any():
        return f"ids outside [0, {nsrc}): rows {np.nonzero(((idx < 0) | (idx >= nsrc)).any(axis=1))[0][:5]}"
    d_ours, d_want = knn_distances(src, tgt, idx), knn_distances(src, tgt, i_ref)
    bad = np.nonzero((idx != i_ref).any(axis=1))[0]
    wrong = np.nonzero((d_ours != d_want).any(axis=1))[0]
    dup = [r for r in bad if len(set(idx[r])) != k]
    if len(wrong) or dup:
        out = [f"rows differing: {len(bad)} first: {bad[:5]}; with another distance at some rank: {len(wrong)}; "
               f"with a repeated id: {len(dup)}"]
        for r in list(wrong[:3]) + dup[:2]:
            pos = np.nonzero(idx[r] != i_ref[r])[0]
            out.append(f"   row {r} at {pos[:6]} ours {idx[r][pos][:6]} ref {i_ref[r][pos][:6]} same set "
                       f"{set(idx[r]) == set(i_ref[r])} d ours {d_ours[r][pos][:4]} d ref {d_want[r][pos][:4]}")
        return "\n".join(out)
    if dist is not None and not np.array_equal(dist, d_ours):
        rows = np.nonzero((dist != d_ours).any(axis=1))[0]
        return (f"distances not bit-equal to sqrt(sum of squares) of the returned ids: {len(rows)} rows, first {rows[:5]}, "
                f"e.g. {dist[rows[0]][:4]} for {d_ours[rows[0]][:4]}")
    return None


def check_knn(ctx, c):
    line = line_knn(c)
    ntgt, k = c["ntgt"], c["k"]
    tree = ctx.knn_build(c["src"])
    try:
        res = tree.query(c["tgt"], k, want_dist=True) if c["want_dist"] else (tree.query(c["tgt"], k), None)
        kernels = ctx.last_knn_kernels()
        idx = res[0].numpy().reshape(ntgt, k)
        dist = res[1].numpy().reshape(ntgt, k) if res[1] is not None else None
    finally:
        tree.free()
    i_ref, _ = knn_reference(c)
    what = knn_judge(idx, dist, c, i_ref)
    if what is not None:
        raise AssertionError(f"{line} -> MISMATCH\n  {what}")
    ties = int((idx != i_ref).any(axis=1).sum())
    note = f"  ({ties} row(s) differ only in the order of equidistant sources)\n" if ties else ""
    return {"line": f"{note}{line} -> ok", "kernels": kernels, "tie_rows": ties}


# ========================================================================================================== pipeline
def pipeline_tolerance(pa, ca):
    """MM_FP_TOL's stated bound: max(1e-12, 64 eps max|x| / shortest element edge)."""
    v = pa[ca]
    hmin = min(np.linalg.norm(v[:, a] - v[:, b], axis=1).min() for a, b in HEX_EDGES)
    return max(1e-12, 64 * EPS * np.abs(pa).max() / hmin)


def draw_pipeline(rng, budget):
    (n0, n1), (p0, p1) = PIPELINE_SIZES[budget]
    n = int(rng.integers(n0, n1))
    mesh_seed, jitter = int(rng.integers(1, 1 << 30)), float(rng.uniform(0.0, 0.3)) + 1e-3
    pa, ca = synth.hex_mesh(n, seed=mesh_seed, jitter=jitter)
    pa = pa.copy()
    sheared = bool(rng.random() < 0.5)
    if sheared:                                              # anisotropy / shear / offset
        pa *= rng.uniform(0.2, 5.0, size=3)
        pa[:, 0] += rng.uniform(-0.6, 0.6) * pa[:, 1]
        pa += rng.uniform(-1e3, 1e3, size=3)
    # general position (no exact kNN ties): a tiny random perturbation of every node
    pa += rng.normal(scale=1e-9 * np.ptp(pa, axis=0).max(), size=pa.shape)
    lo, hi = pa.min(axis=0), pa.max(axis=0)
    npts = int(rng.integers(p0, p1))
    margin = rng.choice(PIPELINE_MARGINS)
    pb = rng.uniform(lo - margin * (hi - lo), hi + margin * (hi - lo), size=(npts, 3))
    if rng.random() < 0.3:                                   # some targets exactly on mesh nodes
        take = rng.integers(0, len(pa), size=min(npts, 500))
        pb[: len(take)] = pa[take]
    k = min(int(rng.choice(PIPELINE_KS)), len(ca))
    ncomp = int(rng.choice(PIPELINE_NCOMP))
    fields = rng.normal(size=(ncomp, len(pa)))
    lazy = bool(rng.random() < 0.7)
    return {"name": "pipeline", "budget": budget, "n": n, "mesh_seed": mesh_seed, "jitter": jitter, "sheared": sheared,
            "npts": npts, "margin": float(margin), "k": k, "ncomp": ncomp, "lazy": lazy,
            "pa": np.ascontiguousarray(pa), "ca": ca, "pb": np.ascontiguousarray(pb), "fields": fields}


def line_pipeline(c):
    return (f"case {c.get('case', -1):3d} n={c['n']:2d} N={c['npts']:6d} k={c['k']:2d} C={c['ncomp']} lazy={int(c['lazy'])} "
            f"margin={c['margin']}")


def pipeline_oracle(c):
    """(lists, enc, w, nfailed, status, values with the failed rows zero) of the oracle: cKDTree, the C restatement of the
    reference's locate, the NumPy-order gather."""
    pa, ca, pb, k = c["pa"], c["ca"], c["pb"], c["k"]
    nn, _ = O.knn_ckdtree(O.centroid(ca, pa), pb, k, workers=WORKERS)
    nn = nn.reshape(c["npts"], k)
    enc_o, w_o, nf_o, status = O.locate_hex8(nn, synth.reorder_hex8(ca), pa, pb, want_status=True)
    ok = status >= 0
    enc_z, w_z = enc_o.copy(), w_o.copy()
    enc_z[~ok] = 0
    w_z[~ok] = 0
    return nn, enc_o, w_o, nf_o, status, O.gather(c["fields"], enc_z, w_z)


def check_pipeline(ctx, c):
    """In the context's arithmetic (Context.fp_mode): "exact" bit for bit; "tol" ids, failed counts and failed rows exactly,
    weights to max(1e-12, 64 eps max|x| / hmin), values to 8 times that times max|fields|."""
    pa, ca, pb, fields, k, npts = c["pa"], c["ca"], c["pb"], c["fields"], c["k"], c["npts"]
    TOL = ctx.fp_mode() == "tol"
    ctx.set_lazy_lists(c["lazy"])
    try:
        vals, enc, w, nf = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k, want_operator=True)
        kernels = ctx.last_knn_kernels()
        redone = ctx.last_locate_stats()["redone_exact"] if TOL else 0
        vals2, nf2 = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k)
        kernels = kernels | ctx.last_knn_kernels()
    finally:
        ctx.set_lazy_lists(True)
    e, ww, v1, v2 = enc.numpy(), w.numpy(), vals.numpy(), vals2.numpy()
    nn, enc_o, w_o, nf_o, status, ref_vals = pipeline_oracle(c)
    ok = status >= 0
    tol = pipeline_tolerance(pa, ca) if TOL else 0.0
    same_w = (np.abs(ww[ok] - w_o[ok]).max(initial=0.0) <= tol) if TOL else np.array_equal(ww[ok], w_o[ok])
    good = (nf == nf_o == nf2 and e.shape == enc_o.shape and np.array_equal(e[ok], enc_o[ok]) and same_w
            and not e[~ok].any() and not ww[~ok].any())
    if TOL:
        vtol = tol * 8 * np.abs(fields).max()
        good = good and np.abs(v1 - ref_vals).max(initial=0.0) <= vtol and np.abs(v2 - ref_vals).max(initial=0.0) <= vtol
        # rows of failed points are produced by the exact kernel: bit-equal, sign of zero included
        good = good and v1[~ok].tobytes() == ref_vals[~ok].tobytes() and v2[~ok].tobytes() == ref_vals[~ok].tobytes()
    else:
        good = good and v1.tobytes() == ref_vals.tobytes() and v2.tobytes() == ref_vals.tobytes()
    line = f"{line_pipeline(c)} nfailed={nf:6d} fallback={(status >= k).sum():5d}"
    if good:
        return {"line": f"{line} -> ok", "kernels": kernels, "redone": redone, "nfailed": nf}
    out = [f"{line} -> MISMATCH", f"  nfailed gpu/oracle/values-only: {nf} {nf_o} {nf2}"]
    bad_e = np.nonzero((e[ok] != enc_o[ok]).any(axis=1))[0]
    bad_w = np.nonzero((ww[ok] != w_o[ok]).any(axis=1))[0]
    out.append(f"  rows with different ids: {len(bad_e)} weights: {len(bad_w)} failed rows non-zero: "
               f"{int(e[~ok].any(axis=1).sum())} {int(ww[~ok].any(axis=1).sum())}")
    if TOL:
        out.append(f"  max |dw| {np.abs(ww[ok] - w_o[ok]).max(initial=0.0):.3e} (bound {tol:.3e}) max |dv| "
                   f"{max(np.abs(v1 - ref_vals).max(initial=0.0), np.abs(v2 - ref_vals).max(initial=0.0)):.3e} (bound {vtol:.3e})")
    bv1 = np.nonzero((v1.view(np.int64) != ref_vals.view(np.int64)).any(axis=1))[0]
    bv2 = np.nonzero((v2.view(np.int64) != ref_vals.view(np.int64)).any(axis=1))[0]
    out.append(f"  value rows differing (operator call / values-only call): {len(bv1)} {len(bv2)}")
    for r in list(bv1[:5]) + list(bv2[:5]):
        out.append(f"   row {r} status {status[r]} gpu {v1[r]} {v2[r]} ref {ref_vals[r]}")
    # is it the kNN stage?  (public int64 lists against cKDTree, three runs: a race shows as varying counts)
    tree = ctx.knn_build(O.centroid(ca, pa))
    for rep in range(3):
        got = tree.query(pb, k).numpy().reshape(npts, k)
        badr = np.nonzero((got != nn).any(axis=1))[0]
        out.append(f"   kNN run {rep} rows differing from cKDTree: {len(badr)}")
        for r in badr[:3]:
            pos = np.nonzero(got[r] != nn[r])[0]
            out.append(f"     row {r} differs at {pos} ours {got[r][pos]} ref {nn[r][pos]} same set {set(got[r]) == set(nn[r])}")
    tree.free()
    idx_ok = np.nonzero(ok)[0]
    for r in bad_e[:5]:
        t = idx_ok[r]
        out.append(f"   target {t} status {status[t]} gpu ids {e[t]} ref ids {enc_o[t]}")
    raise AssertionError("\n".join(out))


# =============================================================================================================== GLL
def draw_gll(rng, budget):
    n_ranges, (p0, p1) = GLL_SIZES[budget]
    order = int(rng.choice(GLL_ORDERS))
    dim = int(rng.choice(GLL_DIMS))
    n = int(rng.integers(*n_ranges[dim]))
    jitter = float(rng.uniform(0.0, 0.3))
    mesh_seed = int(rng.integers(1, 1 << 30))
    src = synth.gll_mesh(n, order, seed=mesh_seed, dim=dim, jitter=jitter)
    sheared = bool(rng.random() < 0.5)
    if sheared:
        src = src * rng.uniform(0.3, 4.0, size=dim) + rng.uniform(-50, 50, size=dim)
        src[..., 0] += rng.uniform(-0.4, 0.4) * src[..., 1]
    lo, hi = src.reshape(-1, dim).min(axis=0), src.reshape(-1, dim).max(axis=0)
    npts = int(rng.integers(p0, p1))
    margin = rng.choice(GLL_MARGINS)
    pts = rng.uniform(lo - margin * (hi - lo), hi + margin * (hi - lo), size=(npts, dim))
    k = min(int(rng.choice(GLL_KS)), len(src))
    cen = src.mean(axis=1) + rng.normal(scale=1e-9, size=(len(src), dim))     # general position
    tol = float(rng.choice(GLL_TOLS))
    snap = bool(rng.random() < 0.5)
    ncomp = int(rng.choice(GLL_NCOMP))
    fields = rng.normal(size=(ncomp,) + src.shape[:2])
    # the fused entry (own centroids and kNN; lists lazy or eager; with or without the operator) -- on meshes in general
    # position only: tied centroid distances are ordered differently by cKDTree
    fused = jitter > GLL_FUSED_MIN_JITTER
    lazy, want_op = (bool(rng.random() < 0.7), bool(rng.random() < 0.3)) if fused else (None, None)
    return {"name": "gll", "budget": budget, "order": order, "dim": dim, "n": n, "jitter": jitter, "mesh_seed": mesh_seed,
            "sheared": sheared, "npts": npts, "margin": float(margin), "k": k, "tol": tol, "snap": snap, "ncomp": ncomp,
            "fused": fused, "lazy": lazy, "want_operator": want_op,
            "src": np.ascontiguousarray(src), "pts": np.ascontiguousarray(pts), "cen": cen, "fields": fields}


def line_gll(c):
    return (f"case {c.get('case', -1):3d} order={c['order']} dim={c['dim']} n={c['n']:2d} N={c['npts']:5d} k={c['k']:2d} "
            f"tol={c['tol']} snap={int(c['snap'])} margin={c['margin']}")


def check_gll(ctx, c):
    order, src, pts, fields, k, npts, tol, snap = c["order"], c["src"], c["pts"], c["fields"], c["k"], c["npts"], c["tol"], c["snap"]
    nn, _ = O.knn_ckdtree(c["cen"], pts, k, workers=WORKERS)
    nn = nn.reshape(npts, k)
    e_g, c_g, m_g = ctx.locate_gll(order, nn, src, pts, tol, snap)
    e_o, c_o, m_o = O.locate_gll(order, nn, src, pts, tol, snap)
    good = m_g == m_o and np.array_equal(e_g.numpy(), e_o) and np.array_equal(c_g.numpy(), c_o)
    v_g = ctx.gather_elem(fields, e_g, c_g).numpy()
    good = good and v_g.tobytes() == O.gather_elem(fields, e_o, c_o).tobytes()
    e_b, c_b, h_b = ctx.locate_gll_bbox(order, nn, src, pts)
    e_bo, c_bo, h_bo = O.locate_gll_v1(order, nn, src, pts)
    good_b = h_b == h_bo and np.array_equal(e_b.numpy(), e_bo) and np.array_equal(c_b.numpy(), c_bo)
    good_f, kernels = True, set()
    if c["fused"]:
        nn_f = O.knn_ckdtree(src.mean(axis=1), pts, k, workers=WORKERS)[0].reshape(npts, k)
        e_f, c_f, m_f = O.locate_gll(order, nn_f, src, pts, tol, snap)
        v_f = O.gather_elem(fields, e_f, c_f)
        ctx.set_lazy_lists(c["lazy"])
        try:
            r = ctx.interpolate_gll(order, src, pts, fields, nelem_to_search=k, tolerance=tol, snap_to_nearest=snap,
                                    want_operator=c["want_operator"])
            kernels = ctx.last_knn_kernels()
        finally:
            ctx.set_lazy_lists(True)
        good_f = r[-1] == m_f and r[0].numpy().tobytes() == v_f.tobytes()
        if c["want_operator"]:
            good_f = good_f and np.array_equal(r[1].numpy(), e_f) and np.array_equal(r[2].numpy(), c_f)
    good = good and good_f
    line = f"{line_gll(c)} missing={m_g:5d} hard={h_b:4d}"
    if not (good and good_b):
        raise AssertionError(f"{line} -> MISMATCH\n  tolerance loop + fused ok: {good} (fused: {good_f} ) bbox loop ok: {good_b}"
                             f"\n  missing gpu/oracle: {m_g} {m_o}  hard gpu/oracle: {h_b} {h_bo}")
    return {"line": f"{line} -> ok", "kernels": kernels, "fused": c["fused"]}


# ============================================================================================================ unique
def draw_unique(rng, budget):
    dim = int(rng.integers(1, 4))
    n = _one_of(rng, UNIQUE_SIZES[budget])
    kind = str(rng.choice(UNIQUE_KINDS))
    if kind == "floats":
        base = rng.normal(size=(max(1, n // int(rng.integers(1, 6))), dim))
        pts = base[rng.integers(0, len(base), size=n)]
    elif kind == "few_values":
        pts = rng.integers(-3, 4, size=(n, dim)).astype(np.float64)
    elif kind == "lattice":
        pts = np.round(rng.uniform(-5, 5, size=(n, dim)), int(rng.integers(0, 3)))
    elif kind == "last_bits":
        # few values of x, each spread over its last bits (the main sort orders by the top 48 bits of x only)
        pts = rng.uniform(-2, 2, size=(n, dim))
        vals = rng.uniform(-2, 2, size=int(rng.integers(1, 40)))
        pts[:, 0] = vals[rng.integers(0, len(vals), size=n)] * (1.0 + rng.integers(0, int(rng.choice([2, 50, 70000])), size=n) * 2.0 ** -52)
        pts = pts[rng.integers(0, n, size=n)]
    else:
        pts = rng.integers(-2, 3, size=(n, dim)).astype(np.float64) * rng.choice([1.0, -0.0, 1e-300, 1e300], size=(n, dim))
    return {"name": "unique", "budget": budget, "dim": dim, "n": n, "kind": kind, "pts": np.ascontiguousarray(pts)}


def line_unique(c):
    return f"case {c.get('case', -1):3d} dim={c['dim']} n={c['n']:7d} {c['kind']:10s}"


def unique_by_sort(pts):
    """np.unique(pts, axis=0, return_inverse=True) restated by a plain lexicographic sort of the rows."""
    order = np.lexsort(pts.T[::-1])
    s = pts[order]
    new = np.ones(len(s), bool)
    new[1:] = (s[1:] != s[:-1]).any(axis=1)
    inv = np.empty(len(s), np.int64)
    inv[order] = np.cumsum(new) - 1
    return s[new], inv


def check_unique(ctx, c):
    pts, n = c["pts"], c["n"]
    u, inv = ctx.unique_points(pts)
    u, inv = u.numpy(), inv.numpy()
    ru, rinv = np.unique(pts, axis=0, return_inverse=True)
    rinv = rinv.reshape(-1)
    good = u.shape == ru.shape and np.array_equal(u, ru) and np.array_equal(inv, rinv) and np.array_equal(u[inv], pts)
    # the order-free form: first occurrences, ascending
    u2, inv2 = ctx.unique_points(pts, ordered=False)
    u2, inv2 = u2.numpy(), inv2.numpy()
    first = np.full(len(ru), n, dtype=np.int64)
    np.minimum.at(first, rinv, np.arange(n))
    order = np.argsort(first)                       # np.unique's classes by first occurrence
    want_u2 = pts[first[order]] + 0.0               # (-0.0 is stored as +0.0)
    pos = np.empty(len(ru), dtype=np.int64)
    pos[order] = np.arange(len(ru))
    good2 = (u2.shape == ru.shape and np.array_equal(u2, want_u2) and not np.signbit(u2[u2 == 0]).any()
             and np.array_equal(inv2, pos[rinv]) and np.array_equal(u2[inv2], pts))
    line = f"{line_unique(c)} unique={len(ru):7d}"
    if not (good and good2):
        raise AssertionError(f"{line} -> MISMATCH\n  ordered form ok: {bool(good)} (unique gpu/numpy: {len(u)} {len(ru)}) "
                             f"order-free form ok: {bool(good2)} (unique: {len(u2)})")
    return {"line": f"{line} -> ok", "kernels": set()}


# ============================================================================================================ the loop
DRAW = {"knn": draw_knn, "pipeline": draw_pipeline, "gll": draw_gll, "unique": draw_unique}
CHECK = {"knn": check_knn, "pipeline": check_pipeline, "gll": check_gll, "unique": check_unique}
LINE = {"knn": line_knn, "pipeline": line_pipeline, "gll": line_gll, "unique": line_unique}


def cases(name, seed, ncases, budget):
    """Cases 0 .. ncases-1 of np.random.default_rng(seed), numbered (case["case"], case["seed"])."""
    rng = np.random.default_rng(seed)
    prev = None
    for number in range(ncases):
        c = draw_knn(rng, budget, prev) if name == "knn" else DRAW[name](rng, budget)
        c["case"], c["seed"] = number, seed
        prev = c
        yield c


def replay_line(c):
    return f"replay: fuzz_cases.cases({c['name']!r}, seed={c['seed']}, ncases={c['case'] + 1}, budget={c['budget']!r}) -> " \
           f"draw_{c['name']} seed {c['seed']} case {c['case']} budget {c['budget']}"


def run_batch(ctx, name, seed, ncases, budget="suite"):
    """Cases 0 .. ncases-1 of a seed, in order on one context -> (kernels launched, the checks' results).  A failure's
    message ends with the line that draws the case again."""
    kernels, infos = set(), []
    for c in cases(name, seed, ncases, budget):
        try:
            info = CHECK[name](ctx, c)
        except AssertionError as e:
            raise AssertionError(f"{e}\n{replay_line(c)}") from None
        except Exception as e:
            raise AssertionError(f"{LINE[name](c)} -> {type(e).__name__}: {e}\n{replay_line(c)}") from e
        kernels |= info["kernels"]
        infos.append(info)
    return kernels, infos


# ================================================================================================= the suite's corpus
# (route, seed, cases) of every batch tests/test_fuzz_gpu.py runs at the "suite" budget; tests/test_fuzz_cases.py checks on
# the CPU that these seeds draw every entry of every choice list and keep both caps (see there).  Routes of the kNN:
# default dispatch, MM_KNN_TREE=1, MM_KNN_FORCE_LIST=1 (in process), MM_KNN_KERNEL=strip / lane (a child process each);
# of the pipeline: the context's arithmetic; "guarded": the child process under MM_GUARD_ALLOC=1.
BATCH = 10
GUARDED_BATCH = 6
SUITE_CORPUS = {
    # (the seeds of the tree, strip and lane routes were picked, from the generator alone, for many 3-D clouds with
    # k <= 20 and, the tree's, at least 4096 sources: the cases those routes can take)
    "knn": [("default", 124, BATCH), ("default", 127, BATCH), ("default", 185, BATCH), ("default", 1, BATCH),
            ("tree", 181, BATCH), ("tree", 265, BATCH), ("list", 42, BATCH), ("strip", 194, BATCH), ("lane", 114, BATCH),
            ("guarded", 27, GUARDED_BATCH)],
    "pipeline": [("exact", 111, BATCH), ("exact", 112, BATCH), ("exact", 113, BATCH), ("exact", 114, BATCH),
                 ("tol", 121, BATCH), ("tol", 122, BATCH), ("tol", 123, BATCH), ("tol", 124, BATCH),
                 ("guarded", 161, GUARDED_BATCH)],
    "gll": [("default", 1211, BATCH), ("default", 1212, BATCH), ("default", 1213, BATCH), ("default", 1214, BATCH),
            ("guarded", 1261, GUARDED_BATCH)],
    "unique": [("default", 311, BATCH), ("default", 312, BATCH), ("default", 313, BATCH), ("default", 314, BATCH),
               ("guarded", 361, GUARDED_BATCH)],
}


def batches(name, route):
    return [(seed, n) for r, seed, n in SUITE_CORPUS[name] if r == route]


def corpus(name):
    """Every case of the suite's corpus of one fuzzer, with case["route"]."""
    for route, seed, n in SUITE_CORPUS[name]:
        for c in cases(name, seed, n, "suite"):
            c["route"] = route
            yield c
