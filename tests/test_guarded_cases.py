"""The inputs of the MM_GUARD_ALLOC tests (tests/guarded_cases.py), checked without a GPU: every unit's arrays span the byte
classes they claim (counted in BYTES: an even number of doubles ends a 16-byte granule, an odd one leaves 8 bytes of slack),
every case holds at least one node of every edge kind its unit names, counted with the statement's own index computation,
and every unit's statement runs on every case.  A later edit of a builder that takes an edge away fails here."""
import numpy as np
import pytest

import diffusion_cases as DC
import frames_cases as FC
import gradient_cases as GC
import grid_adjoint_cases as GA
import guarded_cases as G
import harmonic_adjoint_cases as AC
import harmonic_cases as HC
import layered_cases as LC
import mass_cases as M
import order_cases as OC
import radial_cases as RC
import scattered_cases as SC

ALL = {"pages", "granule", "neither"}


def test_byte_classes_are_counted_in_bytes():
    assert G.byte_class(8 * 2) == "granule" and G.byte_class(8 * 3) == "neither" and G.byte_class(8 * 512) == "pages"
    assert G.byte_class(4 * 4) == "granule" and G.byte_class(4 * 6) == "neither" and G.byte_class(4 * 1024) == "pages"
    assert [c * 24 for c in G.N_POINTS] == [192, 2424, 24576] and [G.byte_class(c * 24) for c in G.N_POINTS] == ["granule", "neither", "pages"]


def test_tile_sizes_are_those_of_the_statements():
    for order in G.ORDERS:
        for dim in (2, 3):
            P = (order + 1) ** dim
            assert G.tile(P) == M.tile_elems(order, dim) == OC.tile_elems(order, order, dim)
            assert G.around_a_tile(P) == [n for n in (G.tile(P) - 1, G.tile(P), G.tile(P) + 1) if n]


@pytest.mark.parametrize("unit,arrays", [
    ("radial", ("points", "mass", "fields", "bins")), ("harmonic", ("points", "values_in")),
    ("harmonic_adjoint", ("points", "values", "weight")), ("layered", ("points",)), ("frames", ("points", "planes", "rows", "positions")),
    ("scattered", ("idx", "dist")), ("order", ("values", "scale_in", "div_out")), ("deviation", ("a", "b")),
    ("gradient", ("points", "u")), ("diffusion", ("points", "u", "kappa_h", "kappa_r")), ("pcg", ("mass", "p", "x")),
    ("grid_operator", ("points", "values")), ("sphere", ("points", "rad"))])
def test_every_per_node_array_spans_the_three_classes(unit, arrays):
    cases = getattr(G, unit + "_cases")()
    for what in arrays:
        assert G.classes(cases, what) == ALL, (unit, what, G.classes(cases, what))


def test_small_tables_span_an_even_and_an_odd_count():
    assert G.classes(G.radial_cases(), "radius") == {"granule", "neither"} == G.classes(G.radial_cases(), "edges")
    assert G.classes(G.harmonic_cases(), "radius") == {"granule", "neither"} == G.classes(G.harmonic_adjoint_cases(), "radius")
    assert G.classes(G.harmonic_cases(), "coef") <= {"granule", "pages"}                  # 16 bytes per (knot, l, k)
    assert {"granule", "neither"} <= G.classes(G.layered_cases(), "lat") | G.classes(G.layered_cases(), "lon")
    assert {"granule", "neither"} <= G.classes(G.layered_cases(), "bounds")
    assert {"granule", "neither"} <= G.classes(G.scattered_cases(), "fields")
    assert all(len(c["radius"]) <= 5 for c in G.radial_cases() + G.harmonic_cases() + G.harmonic_adjoint_cases())
    assert {c["lmax"] for c in G.harmonic_cases()} == set(G.LMAX) == {c["lmax"] for c in G.harmonic_adjoint_cases()}
    assert max(c["points"].size // 3 for c in G.harmonic_adjoint_cases()) < 5000


# ------------------------------------------------------------------------------------------------------- edges are there
def _radial_edges(case):
    counts = G.radial_edge_counts(case["points"], case["radius"])
    kinds = ("top", "bottom", "discontinuity", "above", "below") if case["points"].ndim == 2 else ("top", "above")
    if case["points"].ndim == 3 and len(case["points"]) >= 2:
        kinds += ("bottom", "below")
    assert all(counts[k] >= 1 for k in kinds), (case["name"], counts)


def test_radial_cases():
    for case in G.radial_cases():
        _radial_edges(case)
        ref = RC.model_apply(case["points"], case["radius"], case["values"])
        assert np.isfinite(ref).all()
        for mode in (1, 2, 3, 4):
            RC.model_apply(case["points"], case["radius"], case["values"], mode, case["values_in"])
        if "edges" in case:
            counts = G.bin_edge_counts(case)
            assert all(v >= 1 for v in counts.values()), (case["name"], counts)
            b, nout, _ = RC.bins(case["points"], case["edges"])
            assert nout == counts["below"] + counts["above"] and b[0] == case["nbins"] - 1 and b[1] == 0
            sums = RC.binned_weighted_sum(case["mass"], case["fields"], b, case["nbins"])
            assert np.isfinite(sums).all() and RC.bin_counts(b, case["nbins"]).sum() == len(b) - nout


def test_harmonic_cases():
    for case in G.harmonic_cases():
        _radial_edges(case)
        for extend in (False, True):
            out, nout = HC.model_apply(case["points"], case["radius"], case["coef"], case["lmax"], extend=extend)
            assert np.isfinite(out).all() and (nout > 0) == (not extend and case["points"].ndim == 2), case["name"]
    assert sorted(len(c["coef"]) for c in G.harmonic_cases())[-1] == 5                    # four components and one more launch


def test_harmonic_adjoint_cases():
    cases = G.harmonic_adjoint_cases()
    for case in cases:
        _radial_edges(case)
        grad, nout = AC.model_transpose(case["points"], case["radius"], case["lmax"], case["values"], weight=case["weight"])
        assert np.isfinite(grad).all() and (nout > 0) == (case["points"].ndim == 2), case["name"]
        assert grad[:, -1].any() and grad[:, 0].any()                                       # the first and the last knot's rows
    two = [c for c in cases if len(c["limits"]) == 2]
    assert len(two) == 1 and two[0]["points"].size == min(c["points"].size for c in cases) and two[0]["lmax"] >= 1


def test_layered_cases():
    for case in G.layered_cases():
        counts = G.layered_edge_counts(case)
        assert all(v >= 1 for v in counts.values()), (case["name"], counts)
        flat = case["points"].reshape(-1, 3)
        lld = LC.latlondepth(flat)
        if case["periodic"]:
            lld[:, 1] = LC.wrap(lld[:, 1], case["lon"][0])
        dp = LC.element_depth(case["points"]) if case["points"].ndim == 3 else None
        for lateral in (LC.CELL, LC.BILINEAR):
            for pick in (LC.NODE, LC.ELEMENT) if dp is not None else (LC.NODE,):
                for outside in (LC.FILL, LC.CLAMP):
                    out, layer, span, nout = LC.model_apply(lld, dp, case["lat"], case["lon"], case["bounds"], case["values"],
                                                            lateral, pick, outside, -1.5)
                    assert (layer >= 0).any() and nout == (layer < 0).sum()
    assert {c["periodic"] for c in G.layered_cases()} == {False, True}


def test_frames_cases():
    for case in G.frames_cases():
        if "points" in case:
            assert FC.rotate_points(case["matrix"], case["points"]).shape == case["points"].shape
        else:
            want = FC.rotate_vectors(case["matrix"], case["planes"])
            assert want.shape == case["planes"].shape
            assert np.array_equal(case["rows"][:, case["cols"], :].transpose(1, 0, 2), case["planes"])
            assert np.isfinite(FC.local_components(case["positions"], case["planes"])).all()
    assert any(c["points"].size % 2 for c in G.frames_cases() if "points" in c)            # 3 n doubles with n odd


def test_scattered_cases():
    ks = set()
    for case in G.scattered_cases():
        idx, dist, k = case["idx"], case["dist"], case["k"]
        ks.add(k)
        assert (idx[:, :min(k, G.NSRC)] < G.NSRC).all() and (idx[:, G.NSRC:] == G.NSRC).all() and np.isinf(dist[:, G.NSRC:]).all()
        assert idx[-1, 0] == G.NSRC - 1 and dist[-1, 0] == 0.0                              # the last target is the last source
        assert (idx == G.NSRC - 1).any()
        out, nout, near, used = SC.idw(case["fields"], idx, dist, G.NSRC, max_distance=case["cut"], fill=-5.0)
        assert 0 < nout < len(idx) and (used[near > case["cut"]] == 0).all(), case["name"]
        assert SC.idw(case["fields"], idx, dist, G.NSRC)[1] == 0
    assert ks == {1, 2, G.NSRC, G.NSRC + 3}
    assert any(c["k"] == 2 and len(c["idx"]) % 2 for c in G.scattered_cases())            # a last pair that ends no page


def test_order_and_deviation_cases():
    seen = set()
    for case in G.order_cases():
        oi, oo, dim = case["order_in"], case["order_out"], case["dim"]
        E = case["planes"].shape[1]
        seen.add((oi, oo, dim, E - OC.tile_elems(oi, oo, dim)))
        for layout in (0, 1, 2):
            values = OC.from_planes(case["planes"], layout)
            out = OC.tensor_apply(OC.table(oi, oo), dim, values, layout, case["scale_in"], case["div_out"])
            assert np.isfinite(out).all() and out.size == 3 * E * (oo + 1) ** dim
        OC.tensor_apply(OC.transposed_table(oi, oo), dim, case["planes"])
    for oi, oo in ((1, 2), (4, 1), (2, 4)):
        for dim in (2, 3):
            assert {d for a, b, c, d in seen if (a, b, c) == (oi, oo, dim)} >= {-1, 0, 1}
    for case in G.deviation_cases():
        dev, edge = OC.element_deviation(case["a"], case["b"])
        assert (dev > 0).all() and (edge > 0).all()


def test_gradient_cases():
    from multimesh_amd import api

    seen = set()
    for case in G.gradient_cases():
        order, dim, gp = case["order"], case["dim"], case["points"]
        seen.add((order, dim, len(gp) - M.tile_elems(order, dim)))
        assert gp.shape == (len(gp), (order + 1) ** dim, dim)
        grad = GC.gradient(gp, order, api.gll_quadrature(order)[2], case["u"])[0]
        assert np.isfinite(grad).all()
    for order in G.ORDERS:
        for dim in (2, 3):
            assert {d for a, b, d in seen if (a, b) == (order, dim)} >= {-1, 0, 1}


def test_diffusion_and_pcg_cases():
    from multimesh_amd import api

    seen = set()
    for case in G.diffusion_cases():
        order, dim, gp = case["order"], case["dim"], case["points"]
        seen.add((order, dim, len(gp) - M.tile_elems(order, dim)))
        _, w, D = api.gll_quadrature(order)
        y = DC.apply(gp, order, w, D, case["u"], kh=1.0, kh_array=case["kappa_h"])
        assert np.isfinite(y).all() and y.shape == case["u"].shape and case["kappa_h"].shape == gp.shape[:2]     # element-nodal
        if dim == 3:
            assert np.isfinite(DC.apply(gp, order, w, D, case["u"], kh=1.0, kh_array=case["kappa_h"], kr=1.0, kr_array=case["kappa_r"])).all()
    for order in G.ORDERS:
        for dim in (2, 3):
            assert {d for a, b, d in seen if (a, b) == (order, dim)} >= {-1, 0, 1}
    assert [c["p"].shape for c in G.pcg_cases()] == [(3, n) for n in G.N_POINTS]


def test_grid_operator_cases():
    kinds = set()
    for case in G.grid_operator_cases():
        counts = G.grid_operator_edge_counts(case)
        assert all(v >= 1 for v in counts.values()), (case["name"], counts)
        kinds |= set(counts)
        depth, lat, lon = case["axes"]
        assert all((np.diff(a) > 0).all() for a in case["axes"])
        assert {G.byte_class(a.nbytes) for a in case["axes"]} <= {"granule", "neither"}
        cube = np.arange(np.prod([len(a) for a in case["caller"]]), dtype=np.float64).reshape([len(a) for a in case["caller"]])
        prepared = GA.to_prepared(cube, case["flipped"], case["appended"])
        assert prepared.shape == tuple(len(a) for a in case["axes"])
        back = GA.fold(prepared, case["flipped"], case["appended"])
        assert back.shape == cube.shape and (back[..., 1:] == cube[..., 1:]).all()
    assert {"seam", "flipped axes", "corner of the box", "last depth cell", "last latitude cell"} <= kinds
    plain = [c for c in G.grid_operator_cases() if not c["periodic"]]
    assert all(G.byte_class(a.nbytes) == "granule" for c in plain for a in c["axes"])      # even axis lengths


def test_sphere_cases():
    from test_sphere import map_to_sphere_numpy

    for case in G.sphere_cases():
        conn, n = case["connectivity"], len(case["points"])
        uniq, first = np.unique(conn, return_index=True)
        assert len(uniq) == n and first[-1] == conn.size - 1 == case["rad_nodal"].size - 1       # the last radius is read
        assert not case["points"][2].any()
        for args in ((case["rad"], None), (case["rad_nodal"], conn)):
            out = map_to_sphere_numpy(case["points"], *args)
            assert np.isfinite(out).all() and not out[2].any()
    assert G.classes(G.sphere_cases(), "connectivity") == {"granule", "pages"}                   # 64 bytes per element


def test_regular_grid_cases():
    from multimesh_amd import api

    for case in G.regular_grid_cases():
        lat, lon, depth = case["lat"], case["lon"], case["depth"]
        total = len(lat) * len(lon) * len(depth)
        assert total % G.REGULAR_CHUNK not in (0, total) and total > 2 * G.REGULAR_CHUNK                 # a partial last chunk
        assert G.byte_class(depth.nbytes) == "neither" and G.byte_class(case["fields"].nbytes) in ("granule", "pages")
        D, LA, LO = np.meshgrid(depth, lat, lon, indexing="ij")
        targets = api.latlondepth_to_xyz(np.stack([LA, LO, D], axis=-1).reshape(-1, 3))
        values, found, miss = G.regular_grid_oracle(case, targets)
        assert 0 < miss < total and miss == (~found).sum() and np.isfinite(values[:, found]).all()
        assert found[-len(lat) * len(lon):].any() or found[:total - G.REGULAR_CHUNK * 2].any()
        assert found[2 * G.REGULAR_CHUNK:].any(), "no target of the last chunk lies in the mesh"
