"""Thin elements at Earth scale on the GPU: what a Salvus Earth mesh looks like after make_spherical.

Radial layers are 10 to 1000 times wider than tall, and every coordinate is in metres at |x| ~ 6.4e6.  There the
MM_FP_TOL Newton solve certifies nothing (tests/test_newton_host.py: its residual band exceeds the reference's tolerance),
so every solve of every wave goes to locate_pass_kernel's tier-1 queue and is repeated in the reference's arithmetic --
the saturated-queue path.  Everything here is compared with the CPU oracle: the hex8 pipeline (cKDTree -> the C
restatement of the reference's locate -> gather), the GLL locate on a thin-layered spherical chunk, and the kNN on the
meshes' centroids and on clouds far from the origin."""
import os
import subprocess
import sys

import numpy as np
import pytest

from multimesh_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
CENTRE = 6.4e6 * np.array([0.36, -0.48, 0.8])   # |CENTRE| = 6.4e6 m
FLATS = (1e-1, 1e-2, 1e-3)                       # element thickness / width
NODES = 33                                       # 32^3 elements, 1 km wide
WIDTH = 32e3


@pytest.fixture(scope="module")
def ctx():
    from multimesh_amd.device import Context

    c = Context(0)
    yield c
    c.close()


def radial_frame():
    """An orthonormal frame whose third axis points along CENTRE (the mesh's thin axis becomes radial)."""
    r = CENTRE / np.linalg.norm(CENTRE)
    a = np.cross(r, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    return np.stack([a, np.cross(r, a), r], axis=1)


def to_earth(u, flat):
    """Unit-cube coordinates -> metres: 32 km wide, 32 km * flat tall, thin axis radial, centred on CENTRE."""
    s = (u - 0.5) * np.array([WIDTH, WIDTH, WIDTH * flat])
    return np.ascontiguousarray(s @ radial_frame().T + CENTRE)


_MESHES = {}


def thin_mesh(flat):
    """(nodes, exodus connectivity, targets, fields, reordered connectivity) -- cached per flatness."""
    if flat not in _MESHES:
        # radial node lines, as in an Earth mesh: the in-plane jitter is shared by a column of nodes, the radial one is not
        ua, ca = synth.hex_mesh(NODES, jitter=0.0)
        jrng = np.random.default_rng(31)
        g = ua.reshape(NODES, NODES, NODES, 3)
        g[1:-1, 1:-1, :, :2] += jrng.uniform(-0.25, 0.25, size=(NODES - 2, NODES - 2, 1, 2)) / (NODES - 1)
        g[:, :, 1:-1, 2] += jrng.uniform(-0.25, 0.25, size=(NODES, NODES, NODES - 2)) / (NODES - 1)
        ua = np.ascontiguousarray(g.reshape(-1, 3))
        pa = to_earth(ua, flat)
        rng = np.random.default_rng(int(1 / flat))
        ub = rng.uniform(0.0, 1.0, size=(60_000, 3))
        ub[:2000] = ua[rng.integers(0, len(ua), 2000)]                                  # on nodes: max|xi| = 1
        ub[2000:5000, 2] = rng.choice([-1.0, 1.0], 3000) * rng.uniform(1e-3, 2e-2, 3000) + (ub[2000:5000, 2] > 0.5)
        ub[5000:6000] = rng.uniform(-1.0, 2.0, size=(1000, 3))                          # mostly outside the box
        pb = to_earth(ub, flat)
        pb[:2000] = pa[rng.integers(0, len(pa), 2000)]                                  # nodes, bit for bit
        fields = np.ascontiguousarray(synth.vector_field(ua)[:2])
        conn = synth.reorder_hex8(ca)
        _MESHES[flat] = (pa, ca, pb, fields, conn)
    return _MESHES[flat]


RST = np.array([[-1, -1, -1], [-1, 1, -1], [1, 1, -1], [1, -1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]])
EDGES = [(a, b) for a in range(8) for b in range(a + 1, 8) if (RST[a] != RST[b]).sum() == 1]


def row_bounds(pa, pb, enc):
    """MM_FP_TOL's stated tolerance per target, for the element the oracle located it in (enc: its corner node ids, in
    the reordered corner order): max(1e-12, 64 eps max|x| / shortest edge), max|x| over the corners and the target."""
    h = np.min([np.linalg.norm(pa[enc[:, a]] - pa[enc[:, b]], axis=1) for a, b in EDGES], axis=0)
    xmax = np.maximum(np.abs(pa[enc]).max(axis=(1, 2)), np.abs(pb).max(1))
    return np.maximum(1e-12, 64 * EPS * xmax / h)


def within_bounds(w, w_o, vals, vals_o, fields, pa, pb, enc_o):
    """Weights (absolutely) and values (relative to 8 max|field|) of every located target within its element's bound."""
    ok = w_o.any(axis=1)
    b = row_bounds(pa, pb[ok], enc_o[ok])
    assert (np.abs(w[ok] - w_o[ok]).max(1) <= b).all()
    if vals is not None:
        assert (np.abs(vals[ok] - vals_o[ok]).max(1) <= b * 8 * np.abs(fields).max()).all()


_ORACLE = {}


def oracle(flat, k):
    if (flat, k) not in _ORACLE:
        pa, ca, pb, fields, conn = thin_mesh(flat)
        nn, _ = O.knn_ckdtree(O.centroid(ca, pa), pb, k, workers=-1)
        enc, w, nf = O.locate_hex8(nn, conn, pa, pb)
        _ORACLE[flat, k] = (nn, enc, w, nf, O.gather(fields, enc, w))
    return _ORACLE[flat, k]


@pytest.mark.parametrize("flat", FLATS)
@pytest.mark.parametrize("k", [1, 20, 64])
def test_exact_mode_is_bit_identical_to_the_oracle(ctx, flat, k):
    pa, ca, pb, fields, conn = thin_mesh(flat)
    nn, enc_o, w_o, nf_o, vals_o = oracle(flat, k)
    failed = ~w_o.any(axis=1)
    assert 0 < nf_o < (0.5 if k == 1 else 0.1) * len(pb) and failed.sum() == nf_o
    ctx.set_fp_mode("exact")
    for lazy in (True, False):
        ctx.set_lazy_lists(lazy)
        try:
            vals, enc, w, nf = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k, want_operator=True)
            vals2, nf2 = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k)
        finally:
            ctx.set_lazy_lists(True)
        assert nf == nf2 == nf_o, (lazy, nf, nf2, nf_o)
        assert np.array_equal(enc.numpy(), enc_o) and np.array_equal(w.numpy(), w_o)
        assert vals.numpy().tobytes() == vals_o.tobytes() == vals2.numpy().tobytes()
    # the staged call with the oracle's lists, into arrays the caller filled: failed rows untouched
    enc0, w0 = np.full((len(pb), 8), 7, np.int64), np.full((len(pb), 8), 0.25)
    enc, w, nf = ctx.locate_hex8(nn, conn, pa, pb, enc=ctx.to_device(enc0), weights=ctx.to_device(w0))
    enc, w = enc.numpy(), w.numpy()
    assert nf == nf_o
    assert np.array_equal(enc[~failed], enc_o[~failed]) and np.array_equal(w[~failed], w_o[~failed])
    assert np.array_equal(enc[failed], enc0[failed]) and np.array_equal(w[failed], w0[failed])


@pytest.mark.parametrize("flat", FLATS)
@pytest.mark.parametrize("k", [1, 20, 64])
def test_tol_mode_ids_exact_weights_within_the_stated_bound(ctx, flat, k):
    # measured redone_exact / located targets: >= 1 on every case (every solve that located a target, and more, was
    # repeated in the reference's arithmetic; the fast solve certifies nothing at these coordinates)
    pa, ca, pb, fields, conn = thin_mesh(flat)
    nn, enc_o, w_o, nf_o, vals_o = oracle(flat, k)
    located = len(pb) - nf_o
    ctx.set_fp_mode("tol")
    try:
        for lazy in (True, False):
            ctx.set_lazy_lists(lazy)
            try:
                vals, enc, w, nf = ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k, want_operator=True)
                stats = ctx.last_locate_stats()
            finally:
                ctx.set_lazy_lists(True)
            assert nf == nf_o and np.array_equal(enc.numpy(), enc_o)
            within_bounds(w.numpy(), w_o, vals.numpy(), vals_o, fields, pa, pb, enc_o)
            assert not w.numpy()[~w_o.any(axis=1)].any()
            # the saturated queue: (nearly) every solve was repeated exactly
            assert stats["redone_exact"] >= 0.99 * located, (lazy, stats, located)
            print(f"flat {flat:g} k {k} lazy {lazy}: redone_exact {stats['redone_exact']} / {located} located targets")
        enc, w, nf = ctx.locate_hex8(nn, conn, pa, pb)
        assert nf == nf_o and np.array_equal(enc.numpy(), enc_o)
        within_bounds(w.numpy(), w_o, None, None, fields, pa, pb, enc_o)
        assert ctx.last_locate_stats()["redone_exact"] >= 0.99 * located
    finally:
        ctx.set_fp_mode("exact")


@pytest.mark.parametrize("flat", FLATS)
def test_resident_source_on_thin_elements(ctx, flat):
    pa, ca, pb, fields, conn = thin_mesh(flat)
    _, enc_o, w_o, nf_o, vals_o = oracle(flat, 20)
    src = ctx.source(pa, ca)
    try:
        for mode in ("exact", "tol"):
            ctx.set_fp_mode(mode)
            for lazy in (True, False):
                ctx.set_lazy_lists(lazy)
                try:
                    vals, enc, w, nf = src.interpolate(pb, fields, nelem_to_search=20, want_operator=True)
                    vals2, nf2 = src.interpolate(pb, fields, nelem_to_search=20)
                finally:
                    ctx.set_lazy_lists(True)
                assert nf == nf2 == nf_o and np.array_equal(enc.numpy(), enc_o)
                if mode == "exact":
                    assert np.array_equal(w.numpy(), w_o)
                    assert vals.numpy().tobytes() == vals_o.tobytes() == vals2.numpy().tobytes()
                else:
                    within_bounds(w.numpy(), w_o, vals2.numpy(), vals_o, fields, pa, pb, enc_o)
    finally:
        ctx.set_fp_mode("exact")
        src.free()


# ---------------------------------------------------------------------------------------------------------------------
# GLL locate on a spherical chunk with thin radial layers, ellipticity and topography
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 4])
def test_gll_locate_on_thin_radial_layers_equals_the_oracle(ctx, order):
    r0 = synth.R_EARTH - 400.0
    chunk = synth.earth_chunk(order=order, nlat=6, nlon=6, lat=(-0.05, 0.05), lon=(-0.05, 0.05),
                              radii=(r0, r0 + 100.0, r0 + 160.0, r0 + 240.0, synth.R_EARTH), nrad=(2, 1, 2, 3),
                              ellipticity=3.35e-3, topography=3e-6, taper_radius=r0 + 50.0, topo_seed=3)
    gp = np.ascontiguousarray(chunk["points"])
    cen = gp.mean(axis=1)
    pts_all = gp.reshape(-1, 3)
    rng = np.random.default_rng(order)
    # targets: random convex combinations of an element's nodes (inside or near it), nodes themselves, a few far away
    e = rng.integers(0, len(gp), 20_000)
    wts = rng.dirichlet(np.full(gp.shape[1], 0.3), size=len(e))
    pts = np.einsum("np,npj->nj", wts, gp[e])
    pts[:2000] = pts_all[rng.integers(0, len(pts_all), 2000)]
    radial = pts[2000:3000] / np.linalg.norm(pts[2000:3000], axis=1, keepdims=True)
    pts[2000:3000] += radial * rng.uniform(-30.0, 30.0, size=(1000, 1))              # moved across the layers
    pts = np.ascontiguousarray(pts)
    k = 20
    # (targets on nodes are equidistant from several centroids: cKDTree orders such ties its own way, so the lists are
    # checked against brute force with ties allowed, and the oracle locates from the same lists as the kernel)
    nn, dist = ctx.knn_build(cen).query(pts, k, want_dist=True)
    nn = nn.numpy()
    knn_check(nn, dist.numpy(), cen, pts, k)
    fields = np.stack([synth.field_linear((gp - cen.min(0)) / 1e3), chunk["z_node_1D"]])
    for tol, snap in ((1.05, False), (1.05, True)):
        elem, co, miss = ctx.locate_gll(order, nn, gp, pts, tolerance=tol, snap_to_nearest=snap)
        elem_o, co_o, miss_o = O.locate_gll(order, nn, gp, pts, tolerance=tol, snap_to_nearest=snap)
        assert miss == miss_o and np.array_equal(elem.numpy(), elem_o) and np.array_equal(co.numpy(), co_o)
        vals_o = O.gather_elem(fields, elem_o, co_o)
        assert np.array_equal(ctx.gather_elem(fields, elem, co).numpy(), vals_o)
        for lazy in (True, False):
            ctx.set_lazy_lists(lazy)
            try:
                v, el, c2, m2 = ctx.interpolate_gll(order, gp, pts, fields, nelem_to_search=k, tolerance=tol,
                                                    snap_to_nearest=snap, want_operator=True)
            finally:
                ctx.set_lazy_lists(True)
            assert m2 == miss_o and np.array_equal(el.numpy(), elem_o) and np.array_equal(c2.numpy(), co_o)
            assert np.array_equal(v.numpy(), vals_o) and np.array_equal(np.signbit(v.numpy()), np.signbit(vals_o))
    assert (elem_o >= 0).mean() > 0.9
    elem, co, hard = ctx.locate_gll_bbox(order, nn, gp, pts)
    elem_o, co_o, hard_o = O.locate_gll_v1(order, nn, gp, pts)
    assert hard == hard_o and np.array_equal(elem.numpy(), elem_o) and np.array_equal(co.numpy(), co_o)


# ---------------------------------------------------------------------------------------------------------------------
# kNN on thin-mesh centroids and far from the origin
# ---------------------------------------------------------------------------------------------------------------------
_BRUTE = {}


def knn_check(idx, dist, src, q, k):
    """idx / dist against brute force in fp64: distances bit-equal to sqrt of the reference's sum of squares, indices
    equal except for reorderings among equal distances."""
    key = (src.shape, src[:4].tobytes(), q.shape, q[:4].tobytes())
    if key not in _BRUTE:
        _BRUTE[key] = O.knn_brute(src, q, 20)
    ref = np.ascontiguousarray(_BRUTE[key][:, :k])
    diff = src[ref] - q[:, None, :]
    d2 = (diff * diff).sum(axis=2) if src.shape[1] == 2 else (diff[..., 0] ** 2 + diff[..., 1] ** 2) + diff[..., 2] ** 2
    refd = np.sqrt(d2)
    assert np.array_equal(dist, refd), np.argwhere(dist != refd)[:5]
    differ = idx != ref
    if differ.any():
        # a different index is allowed only where its distance equals the reference's at that rank
        got = src[idx] - q[:, None, :]
        gd = np.sqrt((got[..., 0] ** 2 + got[..., 1] ** 2) + (got[..., 2] ** 2 if src.shape[1] == 3 else 0.0))
        assert np.array_equal(gd[differ], refd[differ])
        assert all(len(set(r)) == k for r in idx[differ.any(axis=1)])


def far_clouds(dim):
    """(name, sources, queries): thin-mesh centroids at Earth scale, uniform and lattice clouds at |lo| / cell of
    1e3, 1e7 and 1e9."""
    rng = np.random.default_rng(dim)
    out = []
    if dim == 3:
        for flat in (1e-1, 1e-3):
            pa, ca, pb, _, _ = thin_mesh(flat)
            out.append((f"centroids{flat:g}", O.centroid(ca, pa), pb[rng.integers(0, len(pb), 6000)]))
    for ratio in (1e3, 1e7, 1e9):
        cell = 1.0 / 32
        lo = np.full(dim, ratio * cell)
        lo[0] = -lo[0]
        src = lo + rng.uniform(size=(30_000, dim))
        g = np.arange(20) / 19
        lat = lo + np.stack(np.meshgrid(*([g] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
        q = lo + rng.uniform(-0.05, 1.05, size=(4000, dim))
        out.append((f"uniform{ratio:g}", src, q))
        out.append((f"lattice{ratio:g}", lat, np.concatenate([q[:2000], lat[rng.integers(0, len(lat), 500)]])))
    return [(n, np.ascontiguousarray(s), np.ascontiguousarray(q)) for n, s, q in out]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("route", ["default", "tree", "list"])
def test_knn_far_from_the_origin_equals_brute_force(ctx, monkeypatch, dim, route):
    if route == "tree":
        monkeypatch.setenv("MM_KNN_TREE", "1")
    elif route == "list":
        monkeypatch.setenv("MM_KNN_FORCE_LIST", "1")
    for name, src, q in far_clouds(dim):
        index = ctx.knn_build(src)
        for k in (1, 8, 20):
            idx, dist = index.query(q, k, want_dist=True)
            try:
                knn_check(idx.numpy(), dist.numpy(), src, q, k)
            except AssertionError as e:
                raise AssertionError(f"{name} k={k}: {e}") from None
        index.free()


_FORCED_CHECK = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_thin_elements_gpu as T
from multimesh_amd.device import Context
with Context(0) as ctx:
    for dim in (2, 3):
        for name, src, q in T.far_clouds(dim):
            index = ctx.knn_build(src)
            for k in (1, 8, 20):
                idx, dist = index.query(q, k, want_dist=True)
                try:
                    T.knn_check(idx.numpy(), dist.numpy(), src, q, k)
                except AssertionError as e:
                    raise AssertionError(f"{dim}-D {name} k={k}: {e}") from None
            index.free()
print("ok")
"""


@pytest.mark.parametrize("kernel", ["strip", "lane"])
def test_knn_far_from_the_origin_forced_kernels(kernel):
    # MM_KNN_KERNEL is read once per process: a fresh child process per kernel
    env = dict(os.environ, MM_KNN_KERNEL=kernel)
    code = _FORCED_CHECK % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-3000:]
