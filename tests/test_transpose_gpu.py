"""The operator transpose on the GPU (mm_transpose_create_nodes / _elem, mm_transpose_apply): every comparison is BIT
equality with the NumPy statement of tests/transpose_cases.py (np.add.at on zeros = the sequential loop in ascending flat
index), except the adjoint identity, whose bound is derived where it is asserted.

Bins of the node-form apply (mm_transpose.hip): rows of up to LONG_ROW = 32 contributions are summed by one lane, longer
rows by one wave in steps of WAVE = 64 products; the element form gives every element a group of 4 .. 64 lanes and walks
its targets a group's width at a time.  The straddle cases hold a row of every length around those edges."""
import ctypes as C

import numpy as np
import pytest

import transpose_cases as T
from multimesh_amd import api, helpers, synth
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

MM_ERR_ARG, MM_ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def _check_nodes(ctx, ids, w, nsrc, comps=(1, 3, 4), name=""):
    op = ctx.transpose_nodes(ids, w, nsrc)
    for ncomp in comps:
        v = T.case_values(name or "nodes", len(ids), ncomp)
        ref = T.transpose_nodes(ids, w, v, nsrc)
        got = op.apply(v).numpy()
        assert got.shape == (ncomp, nsrc)
        assert T.same_bits(got, ref), (name, ncomp, "point-major")
        got_cm = op.apply(np.ascontiguousarray(v.T), point_major=False).numpy()
        assert T.same_bits(got_cm, ref), (name, ncomp, "component-major")
    op.free()
    return ref


def _check_elem(ctx, elem, co, nelem, comps=(1, 3, 4), name=""):
    op = ctx.transpose_elem(elem, co, nelem)
    for ncomp in comps:
        v = T.case_values(name or "elem", len(elem), ncomp)
        ref = T.transpose_elem(elem, co, v, nelem)
        got = op.apply(v).numpy()
        assert got.shape == (ncomp, nelem, co.shape[1])
        assert T.same_bits(got, ref), (name, ncomp, "point-major")
        got_cm = op.apply(np.ascontiguousarray(v.T), point_major=False).numpy()
        assert T.same_bits(got_cm, ref), (name, ncomp, "component-major")
    op.free()
    return ref


# ---------------------------------------------------------------------------------------------- fixture operators
@pytest.mark.parametrize("name", ["hex8_small", "hex8_hard_k20", "hex8_hard_k1"])
def test_fixture_operators(ctx, golden, name):
    enc, w, nsrc = T.golden_operator(golden, name)
    _check_nodes(ctx, enc, w, nsrc, name=name)


# ---------------------------------------------------------------------------------------------- pipeline operators
@pytest.mark.parametrize("n_src,n_tgt", [(17, 23), (101, 100)])
def test_pipeline_operators(ctx, n_src, n_tgt):
    """Operators as the device produces them (k = 20); 101^3 -> 100^3 is about 1 M -> 1 M."""
    pa, ca = synth.hex_mesh(n_src, seed=1)
    pb, _ = synth.hex_mesh(n_tgt, seed=7)
    _, enc_d, w_d, nfailed = ctx.interpolate_hex8(pa, ca, pb, np.zeros((1, len(pa))), nelem_to_search=20, want_operator=True)
    assert nfailed == 0
    enc, w = enc_d.numpy(), w_d.numpy()
    op = ctx.transpose_nodes(enc_d, w_d, len(pa))          # the resident operator, as a workflow holds it
    for ncomp in (1, 3):
        v = T.case_values(f"pipeline{n_src}", len(pb), ncomp)
        ref = T.transpose_nodes(enc, w, v, len(pa))
        assert T.same_bits(op.apply(v).numpy(), ref), ncomp
        if ncomp == 1:   # not vacuous: the order of a row's terms shows in the reference's bits
            assert not T.same_bits(ref, T.transpose_nodes_reversed(enc, w, v, len(pa)))
    # P^T 1: the coverage map; every weight row sums to 1, so the map sums to the number of targets
    cover = op.apply(np.ones(len(pb))).numpy()
    assert T.same_bits(cover, T.transpose_nodes(enc, w, np.ones(len(pb)), len(pa)))
    assert abs(cover.sum() - len(pb)) < 1e-6 * len(pb)
    op.free()


@pytest.mark.parametrize("order,dim,n_src,n_tgt", [(1, 2, 12, 40), (2, 2, 9, 30), (4, 2, 7, 25), (1, 3, 7, 11),
                                                   (2, 3, 6, 9), (4, 3, 5, 8)])
def test_gll_pipeline_operators(ctx, order, dim, n_src, n_tgt):
    """Operators of interpolate_gll on 2-D and 3-D GLL meshes (P = 4, 9, 25, 8, 27, 125), some targets outside."""
    src = synth.gll_mesh(n_src, order, seed=1, dim=dim)
    rng = np.random.default_rng(order * 10 + dim)
    inside = synth.gll_mesh(n_tgt, 1, seed=7, dim=dim).reshape(-1, dim)
    pts = np.concatenate([inside, rng.uniform(1.2, 1.5, size=(50, dim))])[rng.permutation(len(inside) + 50)]
    f = np.zeros((1,) + src.shape[:2])
    _, elem_d, co_d, missing = ctx.interpolate_gll(order, src, pts, f, nelem_to_search=20, want_operator=True)
    elem, co = elem_d.numpy(), co_d.numpy()
    assert missing >= 50 and (elem == -1).sum() == missing and co.shape[1] == (order + 1) ** dim
    op = ctx.transpose_elem(elem_d, co_d, len(src))
    for ncomp in (1, 3):
        v = T.case_values(f"gll{order}{dim}", len(pts), ncomp)
        ref = T.transpose_elem(elem, co, v, len(src))
        assert T.same_bits(op.apply(v).numpy(), ref), ncomp
        if ncomp == 1:
            assert not T.same_bits(ref, T.transpose_elem_reversed(elem, co, v, len(src)))
    op.free()


# ---------------------------------------------------------------------------------------------- P and row shapes
@pytest.mark.parametrize("name", T.NODE_CASES)
def test_node_cases(ctx, name):
    ids, w, nsrc = T.node_case(name)
    ref = _check_nodes(ctx, ids, w, nsrc, comps=(1, 3) if name == "one_node" else (1, 3, 4), name=name)
    unnamed = np.setdiff1d(np.arange(nsrc), ids.ravel())
    if name in ("one_node", "skewed") or name.startswith("straddle"):
        assert len(unnamed) > 0
    assert not ref[:, unnamed].any() and not np.signbit(ref[:, unnamed]).any()    # (and the device's bits equal these)


@pytest.mark.parametrize("name", T.ELEM_CASES)
def test_elem_cases(ctx, name):
    elem, co, nelem = T.elem_case(name)
    ref = _check_elem(ctx, elem, co, nelem, comps=(1, 3) if name == "one_elem" else (1, 3, 4), name=name)
    unnamed = np.setdiff1d(np.arange(nelem), elem)
    assert len(unnamed) > 0 and not ref[:, unnamed].any() and not np.signbit(ref[:, unnamed]).any()


def test_unnamed_destinations_overwrite_what_was_there(ctx):
    """out= reuse: a buffer full of -0.0 / NaN comes back with +0.0 (sign bit clear) where nobody adds."""
    ids, w, nsrc = T.node_case("skewed")
    v = T.case_values("skewed", len(ids), 3)
    ref = T.transpose_nodes(ids, w, v, nsrc)
    op = ctx.transpose_nodes(ids, w, nsrc)
    out = ctx.to_device(np.full((3, nsrc), np.nan))
    assert op.apply(v, out=out) is out and T.same_bits(out.numpy(), ref)
    check_neg = ctx.to_device(np.full((3, nsrc), -0.0))
    op.apply(v, out=check_neg)
    got = check_neg.numpy()
    unnamed = np.setdiff1d(np.arange(nsrc), ids.ravel())
    assert len(unnamed) > 0 and T.same_bits(got, ref) and not np.signbit(got[:, unnamed]).any()
    with pytest.raises(ValueError):
        op.apply(v, out=ctx.empty((2, nsrc), np.float64))
    op.free()
    elem, co, nelem = T.elem_case("P9")
    ve = T.case_values("P9", len(elem), 2)
    ope = ctx.transpose_elem(elem, co, nelem)
    oute = ctx.to_device(np.full((2, nelem, 9), -0.0))
    ope.apply(ve, out=oute)
    assert T.same_bits(oute.numpy(), T.transpose_elem(elem, co, ve, nelem))
    ope.free()


# ---------------------------------------------------------------------------------------------- empty and invalid
def test_empty_inputs(ctx):
    op = ctx.transpose_nodes(np.zeros((0, 8), np.int64), np.zeros((0, 8)), 37)
    got = op.apply(np.zeros((0, 2))).numpy()
    assert got.shape == (2, 37) and not got.any() and not np.signbit(got).any()
    assert op.apply(np.zeros((0, 0))).numpy().shape == (0, 37)          # ncomp = 0
    op.free()
    ope = ctx.transpose_elem(np.zeros(0, np.int64), np.zeros((0, 27)), 5)
    gote = ope.apply(np.zeros((0, 1))).numpy()
    assert gote.shape == (1, 5, 27) and not gote.any() and not np.signbit(gote).any()
    ope.free()
    ids, w, nsrc = T.node_case("P8")
    op = ctx.transpose_nodes(ids, w, nsrc)
    assert op.apply(np.zeros((len(ids), 0))).numpy().shape == (0, nsrc)
    op.free()
    all_out = ctx.transpose_elem(np.full(100, -1, np.int64), np.ones((100, 8)), 4)      # every target outside
    z = all_out.apply(np.ones(100)).numpy()
    assert not z.any() and not np.signbit(z).any()
    all_out.free()


def test_invalid_ids_are_refused(ctx):
    lib = ctx.lib
    ids, w, nsrc = T.node_case("P8")
    for bad in (nsrc, -1, np.iinfo(np.int64).min):
        b = ids.copy()
        b[1234, 5] = bad
        h = C.c_void_p()
        d_ids, d_w = ctx.to_device(b), ctx.to_device(w)
        assert lib.mm_transpose_create_nodes(ctx.handle, d_ids.ptr, d_w.ptr, len(b), 8, nsrc, C.byref(h)) == MM_ERR_ARG
        assert h.value is None and b"outside" in lib.mm_last_error()
        with pytest.raises(helpers.MultiMeshHipError):
            ctx.transpose_nodes(b, w, nsrc)
    elem, co, nelem = T.elem_case("P9")
    for bad in (nelem, -2):
        e = elem.copy()
        e[77] = bad
        h = C.c_void_p()
        d_e, d_co = ctx.to_device(e), ctx.to_device(co)
        assert lib.mm_transpose_create_elem(ctx.handle, d_e.ptr, d_co.ptr, len(e), 9, nelem, C.byref(h)) == MM_ERR_ARG
        assert h.value is None
    h = C.c_void_p()
    one = ctx.to_device(np.zeros(8, np.int64))
    assert lib.mm_transpose_create_nodes(ctx.handle, one.ptr, one.ptr, 1, 129, 4, C.byref(h)) == MM_ERR_ARG     # P > 128
    assert lib.mm_transpose_create_nodes(ctx.handle, one.ptr, one.ptr, -1, 8, 4, C.byref(h)) == MM_ERR_ARG


def test_oversized_operators_are_refused_from_the_sizes_alone(ctx):
    """npoints * P beyond the sort's reach: MM_ERR_UNSUPPORTED before anything is allocated or read -- the arrays
    handed over are eight bytes long."""
    lib = ctx.lib
    tiny = ctx.to_device(np.zeros(1, np.int64))
    tiny_w = ctx.to_device(np.zeros(1))
    for npoints, P in [(1 << 29, 8), (1 << 32, 1), ((1 << 31) // 128 + 1, 128), (1 << 40, 27)]:
        h = C.c_void_p()
        rc = lib.mm_transpose_create_nodes(ctx.handle, tiny.ptr, tiny_w.ptr, npoints, P, 1000, C.byref(h))
        assert rc == MM_ERR_UNSUPPORTED and h.value is None, (npoints, P, rc)
    h = C.c_void_p()
    assert lib.mm_transpose_create_elem(ctx.handle, tiny.ptr, tiny_w.ptr, 1 << 31, 125, 1000, C.byref(h)) == MM_ERR_UNSUPPORTED
    # the context is still usable
    ids, w, nsrc = T.node_case("P4")
    _check_nodes(ctx, ids, w, nsrc, comps=(1,), name="P4")


# ---------------------------------------------------------------------------------------------- handles
def test_one_handle_many_value_sets(ctx):
    for form in ("nodes", "elem"):
        if form == "nodes":
            ids, w, ndst = T.node_case("skewed")
            op, ref = ctx.transpose_nodes(ids, w, ndst), lambda v: T.transpose_nodes(ids, w, v, ndst)
        else:
            ids, w, ndst = T.elem_case("P25")
            op, ref = ctx.transpose_elem(ids, w, ndst), lambda v: T.transpose_elem(ids, w, v, ndst)
        sets = [T.case_values(f"{form}{i}", len(ids), 2) for i in range(3)]
        first = op.apply(sets[0]).numpy()
        assert T.same_bits(first, ref(sets[0]))
        for v in sets[1:]:
            assert T.same_bits(op.apply(v).numpy(), ref(v))
        assert T.same_bits(op.apply(sets[0]).numpy(), first)
        op.free()
        with pytest.raises(ValueError):
            op.apply(sets[0])


def test_destroy_and_rebuild(ctx):
    ids, w, nsrc = T.node_case("P27")
    v = T.case_values("P27", len(ids), 3)
    ref = T.transpose_nodes(ids, w, v, nsrc)
    for _ in range(3):
        op = ctx.transpose_nodes(ids, w, nsrc)
        assert T.same_bits(op.apply(v).numpy(), ref)
        op.free()
        op.free()     # idempotent
    elem, co, nelem = T.elem_case("P125")
    ve = T.case_values("P125", len(elem), 1)
    for _ in range(2):
        ope = ctx.transpose_elem(elem, co, nelem)
        assert T.same_bits(ope.apply(ve).numpy(), T.transpose_elem(elem, co, ve, nelem))
        ope.free()


# ---------------------------------------------------------------------------------------------- the public API
def _mesh_pair():
    pa, ca = synth.hex_mesh(21, seed=1)
    pb, _ = synth.hex_mesh(26, seed=7)
    names = ("a", "b", "c")
    fields = synth.vector_field(pa)[:3]
    return HexMesh(pa, ca, dict(zip(names, fields))), pb, names


def test_adjoint_identity_through_the_api(ctx):
    """<P f, g> = <f, P^T g>, the issue's bound 8 N 2^-52 sum|w f g|.  Both sides are sums of the same 8 N products
    w f g in different orders: on its way into either sum a product meets one rounding per multiplication (two) and one
    per addition it takes part in -- at most 8 in a row of P plus N in the dot product on the left, at most the longest
    row of P^T plus the number of nodes on the right.  Each side is therefore within k 2^-53 sum|w f g| (1 + O(k 2^-53))
    of the exact sum with k = 10 + N resp. 2 + longest row + nodes, and the two differ by at most the sum of the two;
    the test asserts that this sum of path lengths stays below 8 N, so the issue's bound holds with a factor 2 to spare."""
    mesh, pb, names = _mesh_pair()
    enc, w, nfailed = api.interpolate_operator(mesh, pb, context=ctx)
    assert nfailed == 0
    rng = np.random.default_rng(5)
    g = rng.normal(size=(len(pb), 3))
    Pf = api.apply_operator(mesh, enc, w, names, context=ctx)                    # [N, C]
    PTg = api.apply_operator_transpose(mesh, enc, w, g, context=ctx)             # [C, npoint]
    F = mesh.fields_matrix(names)
    assert PTg.shape == F.shape and T.same_bits(PTg, T.transpose_nodes(enc, w, g, mesh.npoint))
    n = len(pb)
    assert (10 + n) + (2 + np.bincount(enc.ravel()).max() + mesh.npoint) <= 8 * n
    for c in range(3):
        lhs = float(np.dot(Pf[:, c], g[:, c]))
        rhs = float(np.dot(F[c], PTg[c]))
        mass = float(np.abs(w * F[c][enc] * g[:, c, None]).sum())
        print(f"adjoint c={c}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound = {8 * n * 2.0 ** -52 * mass:.3e}")
        assert abs(lhs - rhs) <= 8 * n * 2.0 ** -52 * mass
    one = api.apply_operator_transpose(mesh, enc, w, g[:, 0], context=ctx)       # [N] = one component
    assert T.same_bits(one, PTg[:1])


def test_stored_operator_round_trip(ctx, tmp_path):
    mesh, pb, _ = _mesh_pair()
    enc, w, _ = api.interpolate_operator(mesh, pb, context=ctx)
    g = np.random.default_rng(6).normal(size=(len(pb), 2))
    direct = api.apply_operator_transpose(mesh, enc, w, g, context=ctx)
    api.save_stored_operator(str(tmp_path / "op"), enc, w)
    elements, coeffs = api.load_stored_operator(str(tmp_path / "op"))
    assert T.same_bits(api.apply_operator_transpose(mesh, elements, coeffs, g, context=ctx), direct)
    # the GLL form of the same round trip
    src = synth.gll_mesh(5, 2, seed=1)
    pts = np.concatenate([synth.gll_mesh(7, 1, seed=7).reshape(-1, 3), np.full((3, 3), 1.4)])
    _, elem_d, co_d, missing = ctx.interpolate_gll(2, src, pts, np.zeros((1,) + src.shape[:2]), want_operator=True)
    elem, co = elem_d.numpy(), co_d.numpy()
    assert missing >= 3
    gv = np.random.default_rng(7).normal(size=(len(pts), 2))
    direct = api.apply_gll_operator_transpose(elem, co, gv, len(src), context=ctx)
    assert direct.shape == (2, len(src), 27) and T.same_bits(direct, T.transpose_elem(elem, co, gv, len(src)))
    api.save_stored_operator(str(tmp_path / "gll"), elem, co)
    elements, coeffs = api.load_stored_operator(str(tmp_path / "gll"))
    assert T.same_bits(api.apply_gll_operator_transpose(elements, coeffs, gv, len(src), context=ctx), direct)
