"""The GLL mass matrix, the volume integrals and the mass-weighted adjoint on the GPU.  mm_gll_mass and mm_weighted_sum
are compared BIT for bit with their NumPy statements (tests/mass_cases.py); integrals, the adjoint identity and the
conservation of int K dV are asserted within term-count bounds (n terms added in any order: n * 2^-52 * sum|t|), derived
where they are asserted.

A 256-thread block of mm_gll_mass takes a tile of 256 // P whole elements (mass_cases.tile_elems): the element counts
below include one below, exactly and one above a tile, counts that leave a broken last tile, and two
(mass_cases.MULTI_TILE) with more tiles than twice the blocks of a launch, where a block takes a tile, a prefetched second
one and a third."""
import math

import numpy as np
import pytest

import mass_cases as M
import transpose_cases as T
from multimesh_amd import api, helpers, synth
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

EPS = M.EPS
MM_ERR_ARG = -1
R0, R1 = 5_971_000.0, 6_371_000.0
SHAPES = [(1, 2), (2, 2), (4, 2), (1, 3), (2, 3), (4, 3)]


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def _check_mass(ctx, gp, order, what=""):
    _, w, D = api.gll_quadrature(order)
    ref_mass, ref_det = M.mass(gp, order, w, D)
    mass, n_bad, det = ctx.gll_mass(order, gp, want_det=True)
    assert mass.shape == det.shape == gp.shape[:2]
    assert M.same_bits(mass.numpy(), ref_mass), (what, "mass")
    assert M.same_bits(det.numpy(), ref_det), (what, "det")
    assert n_bad == M.n_bad(ref_det), what
    mass2, n_bad2 = ctx.gll_mass(order, gp)                      # without the determinant
    assert M.same_bits(mass2.numpy(), ref_mass) and n_bad2 == n_bad
    return ref_mass, n_bad


# ---------------------------------------------------------------------------------------------- mm_gll_mass
@pytest.mark.parametrize("order,dim", SHAPES)
def test_mass_bit_for_bit_on_gll_meshes(ctx, order, dim):
    gp = synth.gll_mesh(9 if dim == 3 else 30, order, seed=3, dim=dim)
    _, n_bad = _check_mass(ctx, gp, order, (order, dim))
    assert n_bad == 0


@pytest.mark.parametrize("order,dim", SHAPES)
def test_mass_element_counts_around_a_tile(ctx, order, dim):
    tile = M.tile_elems(order, dim)
    gp = synth.gll_mesh(13 if dim == 3 else 48, order, seed=5, dim=dim)        # 1728 / 2209 elements
    for nelem in (0, 1, tile - 1, tile, tile + 1, 3 * tile + max(tile // 2, 1), len(gp)):
        if 0 <= nelem <= len(gp):
            _check_mass(ctx, np.ascontiguousarray(gp[:nelem]), order, (order, dim, nelem))


@pytest.mark.parametrize("order,side,nelem", M.MULTI_TILE)
def test_mass_blocks_that_take_three_tiles(ctx, order, side, nelem):
    gp = np.ascontiguousarray(synth.gll_mesh(side, order, seed=5)[:nelem])
    assert len(gp) == nelem > 2 * M.MAX_BLOCKS * M.tile_elems(order, 3)
    _, n_bad = _check_mass(ctx, gp, order, ("multi-tile", order, nelem))
    assert n_bad == 0


@pytest.mark.parametrize("order", [1, 2, 4])
def test_mass_at_earth_scale(ctx, order):
    chunk = synth.earth_chunk(order, nlat=5, nlon=6, ellipticity=3.3e-3, topography=3e-4)
    _, n_bad = _check_mass(ctx, chunk["points"], order, ("earth", order))
    assert n_bad == 0


@pytest.mark.parametrize("order,dim", SHAPES)
def test_mirrored_element_is_counted(ctx, order, dim):
    gp = synth.gll_mesh(6, order, seed=3, dim=dim)
    ref, n_bad = _check_mass(ctx, M.mirrored(gp, len(gp) // 2), order, ("mirrored", order, dim))
    assert n_bad == gp.shape[1] and (ref > 0).all()
    # a left-handed mesh: every node
    flipped = gp.copy()
    flipped[..., 0] = -flipped[..., 0]
    assert _check_mass(ctx, flipped, order, ("left-handed", order, dim))[1] == gp.shape[0] * gp.shape[1]


# ---------------------------------------------------------------------------------------------- mm_weighted_sum
@pytest.mark.parametrize("n", [0, 1, 255, 256, 4095, 4096, 4097, 125 * 1331, 4096 * 4096 + 5])
def test_weighted_sum_bit_for_bit(ctx, n):
    rng = np.random.default_rng(n % 1000)
    mass = rng.uniform(0.5, 1.5, size=n)
    ncomp = 3 if n < 10 ** 7 else 1
    f = T.wide(rng, (ncomp, n))
    ref = M.weighted_sum(mass, f)
    got = ctx.weighted_sum(mass, f)
    assert got.shape == (ncomp,) and M.same_bits(got, ref)
    for c in range(ncomp):
        assert abs(got[c] - math.fsum(mass * f[c])) <= M.term_bound(mass * f[c])
    vol = ctx.weighted_sum(mass)
    assert vol.shape == (1,) and M.same_bits(vol, M.weighted_sum(mass)) and abs(vol[0] - math.fsum(mass)) <= M.term_bound(mass)
    # the same bits again, and from another context
    assert M.same_bits(ctx.weighted_sum(mass, f), ref)
    with Context(0) as other:
        assert M.same_bits(other.weighted_sum(mass, f), ref)


def test_weighted_sum_field_shapes(ctx):
    gp = synth.gll_mesh(6, 2, seed=3)
    mass, _ = ctx.gll_mass(2, gp)
    f = np.stack([synth.field_linear(gp), gp[..., 0] * gp[..., 1]])               # [C, E, P]
    ref = M.weighted_sum(mass.numpy(), f.reshape(2, -1))
    assert M.same_bits(ctx.weighted_sum(mass, f), ref)
    assert M.same_bits(ctx.weighted_sum(mass, f[0]), ref[:1])                     # [E, P]: one field
    with pytest.raises(ValueError):
        ctx.weighted_sum(mass, f[:, :-1])


# ---------------------------------------------------------------------------------------------- api.integrate
@pytest.mark.parametrize("order,n", [(2, 5), (4, 5), (2, 9), (4, 9)])
def test_integrate_cube(ctx, order, n):
    gp = synth.gll_mesh(n, order, seed=3)
    mesh = GllMesh(gp, order, {"f": synth.field_linear(gp)})
    mass = api.gll_mass_matrix(mesh, context=ctx)
    vol = api.integrate(mesh, context=ctx)
    assert isinstance(vol, float) and abs(vol - 1.0) <= M.term_bound(mass)
    got = api.integrate(mesh, ["f"], context=ctx)
    assert got.shape == (1,) and abs(got[0] - 0.75) <= M.term_bound(mass * mesh.element_nodal_fields["f"])


def test_integrate_order_1_is_not_exact(ctx):
    gp = synth.gll_mesh(5, 1, seed=3)
    assert abs(api.integrate(GllMesh(gp, 1), context=ctx) - 1.0) > 1e-7


def _chunk_bound(npoints, thinnest):
    """The term-count bound, relative (all terms are positive), times |x| / h (tests/test_mass.py)."""
    return npoints * EPS * (R1 / thinnest)


@pytest.mark.parametrize("nl", [4, 8])
def test_integrate_chunk_and_layer(ctx, nl):
    chunk = synth.earth_chunk(4, nlat=nl, nlon=nl)                                # layers 1 and 2, two elements thick each
    mesh = GllMesh(chunk["points"], 4)
    exact = M.chunk_volume(R0, R1, 8.0, 16.0)
    vol = api.integrate(mesh, context=ctx)
    assert abs(vol - exact) <= _chunk_bound(chunk["points"].size // 3, 100_000.0) * exact
    shell = M.chunk_volume(6_171_000.0, R1, 8.0, 16.0)
    got = api.integrate(mesh, layers=[2], layer_ids=chunk["layer"], context=ctx)
    assert abs(got - shell) <= _chunk_bound(chunk["points"].size // 6, 100_000.0) * shell
    both = api.integrate(mesh, layers="all", layer_ids=chunk["layer"], context=ctx)
    assert both == vol


# ---------------------------------------------------------------------------------------------- hex8 and assembly
def test_hex8_mass_matrix(ctx):
    pts, conn = synth.hex_mesh(11, seed=3)
    mesh = HexMesh(pts, conn)
    lumped = api.hex8_mass_matrix(mesh, context=ctx)
    _, w, D = api.gll_quadrature(1)
    conn_t = conn[:, [0, 1, 3, 2, 4, 5, 7, 6]]
    elem_mass, det = M.mass(pts[conn_t], 1, w, D)
    ref = np.zeros(len(pts))
    np.add.at(ref, conn_t, elem_mass)
    assert M.n_bad(det) == 0 and M.same_bits(lumped, ref) and (lumped > 0).all()
    # the sum is the order-1 volume of the same mesh
    assert abs(math.fsum(lumped) - math.fsum(elem_mass.ravel())) <= M.term_bound(elem_mass)
    assert M.same_bits(ctx.weighted_sum(lumped), M.weighted_sum(ref))


@pytest.mark.parametrize("order,dim", [(2, 3), (4, 3), (4, 2)])
def test_assemble_gll(ctx, order, dim):
    gp = synth.gll_mesh(5 if dim == 3 else 9, order, seed=3, dim=dim)
    rng = np.random.default_rng(order)
    vals = rng.uniform(0.5, 1.5, size=(2,) + gp.shape[:2])
    out = api.assemble_gll(vals, gp, context=ctx)
    assert out.shape == vals.shape
    uniq, inv = np.unique(gp.reshape(-1, dim), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    flat = out.reshape(2, -1)
    for c in range(2):
        per_node = np.zeros(len(uniq))
        per_node[inv] = flat[c]                                                   # (any copy)
        assert M.same_bits(per_node[inv], flat[c]), "copies of a node differ"
        # the sum over the unique nodes is the sum of the input: the same terms in another order
        assert abs(math.fsum(per_node) - math.fsum(vals[c].ravel())) <= M.term_bound(vals[c])
    assert (np.bincount(inv) > 1).any()
    one = api.assemble_gll(vals[0], gp, context=ctx)                              # [E, P] -> [1, E, P]
    assert one.shape == (1,) + gp.shape[:2] and M.same_bits(one[0], out[0])


# ---------------------------------------------------------------------------------------------- the weighted adjoint
def _shrunk(n, order, seed=7):
    """A fine mesh inside the unit cube, shrunk about its centre so that no point lies on the source's boundary."""
    return 0.5 + 0.9 * (synth.gll_mesh(n, order, seed=seed) - 0.5)


def _targets(ctx, fine, order):
    """(unique points f64[U, 3], their assembled mass f64[U]) of a fine GLL mesh, as apply_gll_operator_adjoint documents."""
    uniq, inv = api.get_unique_points(fine, context=ctx)
    mass = api.gll_mass_matrix(GllMesh(fine, order), context=ctx)
    tm = np.empty(len(uniq))
    tm[inv] = api.assemble_gll(mass, fine, context=ctx).reshape(-1)
    return uniq, tm, mass


def _operator(ctx, src, order, pts):
    f = np.zeros((1,) + src.shape[:2])
    _, elem, co, missing = ctx.interpolate_gll(order, src, pts, f, nelem_to_search=20, want_operator=True)
    assert missing == 0, "every target must be found"
    return elem.numpy(), co.numpy()


@pytest.mark.parametrize("order_c,order_f", [(4, 2), (2, 4)])
def test_adjoint_identity_gll(ctx, order_c, order_f):
    """<P m, g> in the targets' mass = <m, b> with b = P^T (M_f * g).  Both sides are sums of the N * P products
    M_f[n] g[n] coeffs[n][p] m[elem[n]][p] (the left one through N sums of P terms, then N terms): within
    (N * P + N) * 2^-52 * sum of their magnitudes."""
    src = synth.gll_mesh(4, order_c, seed=1)
    fine = _shrunk(5, order_f)
    pts, tm, _ = _targets(ctx, fine, order_f)
    elem, co = _operator(ctx, src, order_c, pts)
    rng = np.random.default_rng(order_c)
    m, g = T.wide(rng, src.shape[:2]), T.wide(rng, len(pts))
    N, P = co.shape
    pm = ctx.gather_elem(m, elem, co).numpy()[:, 0]
    b = api.apply_gll_operator_transpose(elem, co, tm * g, len(src), context=ctx)[0]
    lhs, rhs = math.fsum(tm * g * pm), math.fsum((b * m).ravel())
    bound = (N * P + N) * EPS * math.fsum((np.abs(tm * g)[:, None] * np.abs(co) * np.abs(m[elem])).ravel())
    print(f"adjoint {order_c}->{order_f}: difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    # the weighted adjoint is that b over the source's mass: one division, undone by one product
    K = api.apply_gll_operator_adjoint(elem, co, g, tm, GllMesh(src, order_c), assemble=False, context=ctx)[0]
    mc = api.gll_mass_matrix(GllMesh(src, order_c), context=ctx)
    assert (np.abs(K * mc - b) <= 2 * EPS * np.abs(b)).all()


def test_adjoint_identity_hex8(ctx):
    pa, ca = synth.hex_mesh(9, seed=1)
    pb, cb = synth.hex_mesh(12, seed=7)
    mesh_a = HexMesh(pa, ca)
    enc, w, nfailed = api.interpolate_operator(mesh_a, pb, context=ctx)
    assert nfailed == 0
    tm = api.hex8_mass_matrix(HexMesh(pb, cb), context=ctx)
    rng = np.random.default_rng(8)
    m, g = T.wide(rng, len(pa)), T.wide(rng, len(pb))
    N, P = w.shape
    pm = ctx.gather(m, enc, w).numpy()[:, 0]
    b = api.apply_operator_transpose(mesh_a, enc, w, tm * g, context=ctx)[0]
    bound = (N * P + N) * EPS * math.fsum((np.abs(tm * g)[:, None] * np.abs(w) * np.abs(m[enc])).ravel())
    assert abs(math.fsum(tm * g * pm) - math.fsum(b * m)) <= bound
    K = api.apply_operator_adjoint(mesh_a, enc, w, g, tm, context=ctx)
    ma = api.hex8_mass_matrix(mesh_a, context=ctx)
    assert K.shape == (1, len(pa)) and (np.abs(K[0] * ma - b) <= 2 * EPS * np.abs(b)).all()
    # conservation: K_f = 1 and every weight row sums to 1
    K1 = api.apply_operator_adjoint(mesh_a, enc, w, np.ones(len(pb)), tm, context=ctx)[0]
    terms = tm[:, None] * np.abs(w)
    assert abs(math.fsum(ma * K1) - math.fsum(tm)) <= (N * P + N + 2 * len(pa)) * EPS * math.fsum(terms.ravel())


def test_conservation_and_refinement(ctx):
    """K_f = 1 on a fine mesh of N1 unique targets and on one of twice the resolution with N2: sum(M_c * K_c) stays at
    the fine meshes' (equal) volume, while the plain transpose P^T 1 sums to N1 and then N2 -- it grows with the number
    of targets per element, the weighted adjoint does not.

    Bounds.  sum(M_c * K_c) = sum_n M_f[n] * sum_p coeffs[n][p] up to the rounding of N * P products and adds, of the
    E * P divisions by M_c and products with it (twice that when assembled: the scatter-sums and the sum over the
    copies), and of the N adds of sum(M_f); the coefficients of a found target sum to 1 within P * 2^-52 * sum|coeffs|.
    All of it is covered by (N * P + N + 4 * E * P) * 2^-52 * sum_n M_f[n] sum_p |coeffs[n][p]|."""
    order_c = 4
    src = synth.gll_mesh(4, order_c, seed=1)
    mesh_c = GllMesh(src, order_c)
    mc = api.gll_mass_matrix(mesh_c, context=ctx)
    totals, counts = [], []
    for n_fine in (5, 9):
        fine = _shrunk(n_fine, 2)
        pts, tm, fine_mass = _targets(ctx, fine, 2)
        elem, co = _operator(ctx, src, order_c, pts)
        N, P = co.shape
        volume = math.fsum(fine_mass.ravel())
        assert abs(volume - 0.9 ** 3) <= M.term_bound(fine_mass)
        assert abs(math.fsum(tm) - volume) <= M.term_bound(fine_mass)
        bound = (N * P + N + 4 * src.shape[0] * src.shape[1]) * EPS * math.fsum((tm[:, None] * np.abs(co)).ravel())
        for assemble in (False, True):
            K = api.apply_gll_operator_adjoint(elem, co, np.ones(N), tm, mesh_c, assemble=assemble, context=ctx)
            assert K.shape == (1,) + src.shape[:2]
            total = math.fsum((mc * K[0]).ravel())
            print(f"fine {n_fine} assemble {assemble}: sum(M_c K_c) - sum(M_f) = {total - math.fsum(tm):.3e}, bound {bound:.3e}")
            assert abs(total - math.fsum(tm)) <= bound
            if assemble:                                                          # continuous: copies of a node agree
                again = api.assemble_gll(K[0], src, context=ctx)
                mult = api.assemble_gll(np.ones(src.shape[:2]), src, context=ctx)
                assert (np.abs(again[0] - mult[0] * K[0]) <= 8 * EPS * np.abs(mult[0] * K[0])).all()
            totals.append(total)
        cover = api.apply_gll_operator_transpose(elem, co, np.ones(N), len(src), context=ctx)[0]
        assert abs(math.fsum(cover.ravel()) - N) <= (N * P) * EPS * math.fsum(np.abs(co).ravel())
        counts.append(N)
    assert counts[1] > 6 * counts[0]                                              # P^T 1 grew by N2 / N1 ...
    assert max(totals) - min(totals) <= 4 * bound                                 # ... the weighted adjoint did not


# ---------------------------------------------------------------------------------------------- error paths
def test_error_paths(ctx):
    lib = helpers.load_lib()
    gp = synth.gll_mesh(4, 2, seed=3)
    with pytest.raises(ValueError):
        ctx.gll_mass(3, np.zeros((2, 64, 3)))                   # an order without tables
    with pytest.raises(ValueError):
        ctx.gll_mass(4, gp)                                     # P = 27 is not (4 + 1)^3
    with pytest.raises(ValueError):
        ctx.gll_mass(2, np.zeros((5, 3, 1)))                    # dim 1
    # straight at the ABI: nothing is written
    sentinel = np.full(gp.shape[:2], -7.0)
    mass = ctx.to_device(sentinel)
    gp_d = ctx.to_device(gp)
    _, w, D = api.gll_quadrature(2)
    w_d, D_d = ctx.to_device(w), ctx.to_device(D)
    for order, dim, d_ptr, w_ptr in ((3, 3, D_d.ptr, w_d.ptr), (2, 1, D_d.ptr, w_d.ptr), (2, 4, D_d.ptr, w_d.ptr),
                                     (2, 3, None, w_d.ptr), (2, 3, D_d.ptr, None)):
        rc = lib.mm_gll_mass(ctx.handle, order, dim, gp_d.ptr, len(gp), d_ptr, w_ptr, mass.ptr, None)
        assert rc == MM_ERR_ARG, (order, dim)
        assert M.same_bits(mass.numpy(), sentinel)
    assert lib.mm_gll_mass(ctx.handle, 2, 3, gp_d.ptr, -1, D_d.ptr, w_d.ptr, mass.ptr, None) == MM_ERR_ARG
    assert lib.mm_weighted_sum(ctx.handle, mass.ptr, None, mass.size, 2, mass.ptr) == MM_ERR_ARG   # two sums need fields
    # target_mass of the wrong length
    src = synth.gll_mesh(3, 2, seed=1)
    elem, co = np.zeros(5, np.int64), np.zeros((5, 27))
    with pytest.raises(ValueError):
        api.apply_gll_operator_adjoint(elem, co, np.ones(5), np.ones(4), GllMesh(src, 2), context=ctx)
    pa, ca = synth.hex_mesh(4, seed=1)
    with pytest.raises(ValueError):
        api.apply_operator_adjoint(HexMesh(pa, ca), np.zeros((5, 8), np.int64), np.zeros((5, 8)), np.ones(5), np.ones(6),
                                   context=ctx)
    with pytest.raises(ValueError):
        api.assemble_gll(np.ones((3, 4)), src, context=ctx)
