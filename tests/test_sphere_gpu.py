"""make_spherical on the GPU: the map kernels against the reference's own output, the public map_to_sphere /
map_to_ellipse, and the six drivers with make_spherical=True against the same drivers on pre-mapped inputs."""
import numpy as np
import pytest

from multimesh_amd import synth
from test_sphere import (ELLIPSE_ELLIPTICITY_MAX_M, ELLIPSE_HEX8_MAX_M, ELLIPSE_IDENTITY_ULP, ELLIPSE_ORACLE_ULP,
                         ELLIPSE_TOPOGRAPHY_MAX_M, GLL_Z_INTERP_MAX, R_EARTH, WHY_RATIO_MIN, WHY_SPHERICAL_MAX,
                         gll_points_meshes, map_to_ellipse_oracle, map_to_sphere_numpy, why_meshes, why_model)

pytestmark = pytest.mark.gpu

ELL = dict(ellipticity=3.35e-3, topography=3e-4)


@pytest.fixture(scope="module")
def ctx():
    from multimesh_amd.device import Context

    with Context(0) as c:
        yield c


def _hex8(chunk, fields=None):
    """An order-1 Earth chunk as a node-layout hex8 mesh (exodus corner order) with a NODAL z_node_1D."""
    from multimesh_amd.mesh import HexMesh

    gp, z = chunk["points"], chunk["z_node_1D"]
    uniq, first, inv = np.unique(gp.reshape(-1, 3), axis=0, return_index=True, return_inverse=True)
    conn = inv.reshape(gp.shape[:2])[:, [0, 1, 3, 2, 4, 5, 7, 6]]          # tensor order -> exodus order
    nodal = {"z_node_1D": z.reshape(-1)[first]}
    nodal.update({k: v.reshape(-1)[first] for k, v in (fields or {}).items()})
    return HexMesh(uniq, conn, nodal)


def _salvus(chunk, params):
    """A Salvus model in the HDF5 layout, in memory: MODEL/data holds ``params`` and z_node_1D."""
    from multimesh_amd import io as mio

    h = mio.MemoryH5()
    h.create_dataset("MODEL/coordinates", data=chunk["points"])
    names = list(params) + ["z_node_1D"]
    data = np.stack([params[p] for p in params] + [chunk["z_node_1D"]], axis=1)
    mio.set_dimension_labels(h.create_dataset("MODEL/data", data=data), names)
    ed = np.stack([chunk["fluid"], chunk["layer"]], axis=1)
    h.create_dataset("MODEL/element_data", data=ed).attrs["DIMENSION_LABELS"] = np.array([b"element", b"[ fluid | layer ]"])
    return h


def _premapped(chunk):
    out = dict(chunk)
    out["points"] = map_to_sphere_numpy(chunk["points"], chunk["z_node_1D"])
    return out


# ------------------------------------------------------------------------------------------ the kernels
def test_context_map_to_sphere_equals_the_references_output(ctx, golden):
    g = golden("sphere_map")
    got = ctx.map_to_sphere(g["en_points"], g["en_z_node_1D"]).numpy()
    assert np.array_equal(got, g["en_expected"])
    got = ctx.map_to_sphere(g["node_points"], g["node_z_node_1D"], connectivity=g["node_connectivity"]).numpy()
    assert np.array_equal(got, g["node_expected"])
    # in place: on a device array, and on a NumPy array
    d = ctx.to_device(g["en_points"])
    assert ctx.map_to_sphere(d, g["en_z_node_1D"], out=d) is d
    assert np.array_equal(d.numpy(), g["en_expected"])
    host = g["node_points"].copy()
    assert ctx.map_to_sphere(host, g["node_z_node_1D"], connectivity=g["node_connectivity"], out=host) is host
    assert np.array_equal(host, g["node_expected"])
    # the first occurrence is np.unique's return_index
    first = ctx.first_occurrence(g["node_connectivity"], len(g["node_points"])).numpy()
    assert np.array_equal(first, np.unique(g["node_connectivity"], return_index=True)[1])


def test_context_map_to_sphere_on_ten_million_points(ctx):
    # more points than the grid has threads: the grid-stride tail
    rng = np.random.default_rng(11)
    n = 10_000_003
    pts = rng.uniform(-6.4e6, 6.4e6, size=(n, 3))
    pts[::1_000_000] = 0.0
    z = rng.uniform(0.5, 1.0, size=n)
    got = ctx.map_to_sphere(pts, z).numpy()
    assert np.array_equal(got, map_to_sphere_numpy(pts, z))
    ratio = ctx.sphere_ratio(pts, z).numpy()
    assert np.array_equal(ratio, (np.sqrt(np.sum(pts ** 2, axis=1)) / R_EARTH) / z)
    assert np.array_equal(ctx.scale_points(pts, ratio).numpy(), (ratio * pts.T).T)


def test_bad_meshes_raise(ctx):
    from multimesh_amd import api

    g = synth.earth_chunk(order=1, nlat=2, nlon=2, nrad=(1, 1))
    hm = _hex8(g)
    conn = hm.connectivity
    # a node no element references: the reference fails there with an index error
    pts = np.concatenate([hm.points, [[1.0, 2.0, 3.0]]])
    with pytest.raises(ValueError, match="1 nodes are not referenced"):
        ctx.map_to_sphere(pts, np.ones(conn.shape), connectivity=conn)
    node_mesh = type("M", (), {"points": pts, "connectivity": conn, "element_nodal_fields": {"z_node_1D": np.ones(conn.shape)}})()
    with pytest.raises(ValueError, match="not referenced"):
        api.map_to_sphere(node_mesh)
    assert np.array_equal(node_mesh.points, pts)
    with pytest.raises(ValueError, match="outside"):
        ctx.first_occurrence(np.array([[0, 1, 5]]), 3)
    # no z_node_1D
    with pytest.raises(ValueError, match="z_node_1D"):
        api.map_to_sphere(api.GllMesh(g["points"], 1, {"VP": np.ones(g["z_node_1D"].shape)}))
    from multimesh_amd.mesh import HexMesh

    with pytest.raises(ValueError, match="z_node_1D"):
        api.interpolate_to_points(HexMesh(hm.points, conn, {"VP": np.ones(len(hm.points))}), hm.points, ["VP"],
                                  make_spherical=True)
    # a 2-D mesh
    quad = synth.gll_mesh(3, 1, dim=2)
    with pytest.raises(ValueError, match="3-D"):
        api.map_to_sphere(api.GllMesh(quad, 1, {"z_node_1D": np.ones(quad.shape[:2])}))


def test_public_map_to_sphere_on_every_mesh_kind(golden):
    from multimesh_amd import api, io as mio
    from multimesh_amd.mesh import HexMesh

    g = golden("sphere_map")
    # element-nodal: GllMesh (in place: the same array object), and a Salvus model (the file is not written)
    m = api.GllMesh(g["en_points"], 2, {"z_node_1D": g["en_z_node_1D"]})
    arr = m.gll_points
    assert api.map_to_sphere(m) is m and m.gll_points is arr and np.array_equal(arr, g["en_expected"])
    chunk = synth.earth_chunk(order=2, nlat=2, nlon=3, nrad=(1, 2), **ELL)
    h = _salvus(chunk, {"VP": np.ones(chunk["z_node_1D"].shape)})
    sm = mio.SalvusMesh(h, fast_mode=False)
    api.map_to_sphere(sm)
    assert np.array_equal(sm.points, map_to_sphere_numpy(chunk["points"], chunk["z_node_1D"]))
    assert np.array_equal(h["MODEL/coordinates"][()], chunk["points"])
    fast = mio.SalvusMesh(h, fast_mode=True)                          # z_node_1D read from the file on demand
    api.map_to_sphere(fast)
    assert np.array_equal(fast.points, sm.points)
    # node layout: any object with points, connectivity and an element-nodal z_node_1D (first occurrence)
    node_mesh = type("M", (), {"points": g["node_points"].copy(), "connectivity": g["node_connectivity"],
                               "element_nodal_fields": {"z_node_1D": g["node_z_node_1D"]}})()
    api.map_to_sphere(node_mesh)
    assert np.array_equal(node_mesh.points, g["node_expected"])
    # HexMesh with a nodal z_node_1D: one value per node
    hm = HexMesh(g["node_points"], g["node_connectivity"][:, :8], {"z_node_1D": g["en_z_node_1D"].reshape(-1)[:300]})
    api.map_to_sphere(hm)
    assert np.array_equal(hm.points, map_to_sphere_numpy(g["node_points"], g["en_z_node_1D"].reshape(-1)[:300]))


# ------------------------------------------------------------------------------------------ the six drivers
def test_hex8_drivers_with_make_spherical():
    from multimesh_amd import api
    from multimesh_amd.mesh import HexMesh

    a = synth.earth_chunk(order=1, nlat=6, nlon=6, nrad=(3, 3), topo_seed=1, **ELL)
    b = synth.earth_chunk(order=1, nlat=7, nlon=5, nrad=(4, 4), topo_seed=2, **ELL)
    fa = {"VSV": why_model(a["z_node_1D"], a["layer"]), "VSH": a["points"][..., 0] / R_EARTH}
    ma, mb = _hex8(a, fa), _hex8(b)
    pts_a, pts_b = ma.points.copy(), mb.points.copy()
    mapped_a = HexMesh(map_to_sphere_numpy(ma.points, ma.nodal_fields["z_node_1D"]), ma.connectivity, ma.nodal_fields)
    mapped_b_points = map_to_sphere_numpy(mb.points, mb.nodal_fields["z_node_1D"])
    # interpolate_to_points: the mesh is mapped, the points are taken as given
    targets = mb.points
    got = api.interpolate_to_points(ma, targets, ["VSV", "VSH"], make_spherical=True, nelem_to_search=25)
    want = api.interpolate_to_points(mapped_a, targets, ["VSV", "VSH"], nelem_to_search=25)
    assert np.array_equal(got, want) and np.array_equal(ma.points, pts_a)
    # interpolate_to_mesh: both meshes mapped (copies), fields attached to the new mesh
    api.interpolate_to_mesh(ma, mb, ["VSV", "VSH"], make_spherical=True)
    pre_b = HexMesh(mapped_b_points, mb.connectivity)
    api.interpolate_to_mesh(mapped_a, pre_b, ["VSV", "VSH"])
    for p in ("VSV", "VSH"):
        assert np.array_equal(mb.get_nodal_field(p), pre_b.get_nodal_field(p))
    assert np.array_equal(ma.points, pts_a) and np.array_equal(mb.points, pts_b)


def test_gll_to_points_with_make_spherical():
    from multimesh_amd import api

    a, b = gll_points_meshes()
    fields = {"VP": why_model(a["z_node_1D"], a["layer"]), "z_node_1D": a["z_node_1D"]}
    m = api.GllMesh(a["points"], 2, fields)
    before = m.gll_points.copy()
    pts = map_to_sphere_numpy(b["points"], b["z_node_1D"]).reshape(-1, 3)
    got = api.interpolate_gll_to_points(m, pts, ["VP", "z_node_1D"], make_spherical=True)
    pre = api.GllMesh(map_to_sphere_numpy(a["points"], a["z_node_1D"]), 2, fields)
    assert np.array_equal(got, api.interpolate_gll_to_points(pre, pts, ["VP", "z_node_1D"]))
    assert np.array_equal(m.gll_points, before)
    assert np.abs(got[:, 1] - b["z_node_1D"].reshape(-1)).max() < GLL_Z_INTERP_MAX


@pytest.mark.parametrize("driver", ["gll_2_gll_layered_multi_two", "gll_2_gll_layered", "gll_2_gll_layered_multi"])
def test_salvus_file_drivers_with_make_spherical(driver, tmp_path):
    from multimesh_amd import api

    a = synth.earth_chunk(order=2, nlat=4, nlon=4, nrad=(2, 2), fluid_layers=(1,), topo_seed=1, **ELL)
    b = synth.earth_chunk(order=2, nlat=5, nlon=6, nrad=(3, 3), fluid_layers=(1,), topo_seed=2, **ELL)
    rng = np.random.default_rng(5)
    pa = {"VP": why_model(a["z_node_1D"], a["layer"]), "VS": rng.normal(size=a["z_node_1D"].shape)}
    pb = {"VP": np.full(b["z_node_1D"].shape, -1.0), "VS": np.full(b["z_node_1D"].shape, -2.0)}
    fn = getattr(api, driver)
    kw = dict(layers=[2] if driver != "gll_2_gll_layered_multi_two" else "all", parameters=["VP", "VS"],
              nelem_to_search=20)
    src, dst = _salvus(a, pa), _salvus(b, pb)
    src_pre, dst_pre = _salvus(_premapped(a), pa), _salvus(_premapped(b), pb)
    fn(src, dst, make_spherical=True, **kw)
    fn(src_pre, dst_pre, **kw)
    assert np.array_equal(dst["MODEL/data"][()], dst_pre["MODEL/data"][()])
    assert np.array_equal(src["MODEL/coordinates"][()], a["points"])
    assert np.array_equal(dst["MODEL/coordinates"][()], b["points"])
    assert not np.array_equal(dst["MODEL/data"][()][:, 0], pb["VP"])
    if driver == "gll_2_gll_layered_multi_two":
        # the stored operator: written by a mapped run, re-applied by a second one
        store, store_pre = str(tmp_path / "op"), str(tmp_path / "op_pre")
        dst2, dst2_pre = _salvus(b, pb), _salvus(_premapped(b), pb)
        fn(src, dst2, make_spherical=True, **dict(kw, stored_array=store))
        fn(src_pre, dst2_pre, **dict(kw, stored_array=store_pre))
        assert np.array_equal(dst2["MODEL/data"][()], dst_pre["MODEL/data"][()])
        with np.load(f"{store}/interp_info.npz") as f1, np.load(f"{store_pre}/interp_info.npz") as f2:
            assert sorted(f1.files) == sorted(f2.files) and all(np.array_equal(f1[k], f2[k]) for k in f1.files)
        dst3 = _salvus(b, pb)
        fn(src, dst3, make_spherical=True, **dict(kw, stored_array=store))
        assert np.array_equal(dst3["MODEL/data"][()], dst_pre["MODEL/data"][()])


def test_why_make_spherical_reproduces_the_1d_model():
    from multimesh_amd import api

    a, b = why_meshes()
    want = why_model(b["z_node_1D"], b["layer"])
    errs = {}
    for spherical in (True, False):
        src = _salvus(a, {"VP": why_model(a["z_node_1D"], a["layer"])})
        dst = _salvus(b, {"VP": np.zeros(b["z_node_1D"].shape)})
        api.gll_2_gll_layered_multi_two(src, dst, layers="all", parameters=["VP"], make_spherical=spherical)
        errs[spherical] = np.abs(dst["MODEL/data"][()][:, 0] - want).max()
    assert errs[True] < WHY_SPHERICAL_MAX
    assert errs[False] > WHY_RATIO_MIN * errs[True] and errs[False] > WHY_RATIO_MIN * WHY_SPHERICAL_MAX


# ------------------------------------------------------------------------------------------ map_to_ellipse
def test_map_to_ellipse():
    from multimesh_amd import api

    b0 = synth.earth_chunk(order=2, nlat=5, nlon=6, nrad=(3, 3))
    # a spherical chunk stretched onto a spherical base: back where it was
    a0 = synth.earth_chunk(order=2, nlat=4, nlon=4, nrad=(2, 2))
    mesh = api.GllMesh(b0["points"], 2, {"z_node_1D": b0["z_node_1D"]})
    api.map_to_ellipse(api.GllMesh(a0["points"], 2, {"z_node_1D": a0["z_node_1D"]}), mesh)
    assert np.abs(mesh.gll_points - b0["points"]).max() <= ELLIPSE_IDENTITY_ULP * np.spacing(R_EARTH)
    for kw, limit in ((dict(ellipticity=3.35e-3), ELLIPSE_ELLIPTICITY_MAX_M),
                      (dict(ellipticity=3.35e-3, topography=3e-4, topo_seed=1), ELLIPSE_TOPOGRAPHY_MAX_M)):
        a = synth.earth_chunk(order=2, nlat=4, nlon=4, nrad=(2, 2), **kw)
        base = api.GllMesh(a["points"], 2, {"z_node_1D": a["z_node_1D"]})
        mesh = api.GllMesh(b0["points"], 2, {"z_node_1D": b0["z_node_1D"]})
        api.map_to_ellipse(base, mesh)
        want = synth.earth_chunk(order=2, nlat=5, nlon=6, nrad=(3, 3), **kw)["points"]
        assert np.abs(mesh.gll_points - want).max() < limit
        assert np.array_equal(base.gll_points, a["points"])                    # the base is never modified
        oracle, miss = map_to_ellipse_oracle(a["points"], a["z_node_1D"], b0["points"], b0["z_node_1D"], 2)
        assert miss == 0 and np.abs(mesh.gll_points - oracle).max() <= ELLIPSE_ORACLE_ULP * np.spacing(R_EARTH)
    # an elliptic base as a hex8 mesh, a node-layout target
    ah = _hex8(synth.earth_chunk(order=1, nlat=12, nlon=12, nrad=(2, 2), ellipticity=3.35e-3))
    b1 = synth.earth_chunk(order=1, nlat=5, nlon=5, nrad=(3, 3))
    bh = _hex8(b1)
    first = np.unique(b1["points"].reshape(-1, 3), axis=0, return_index=True)[1]          # bh's node order
    want = synth.earth_chunk(order=1, nlat=5, nlon=5, nrad=(3, 3), ellipticity=3.35e-3)["points"].reshape(-1, 3)[first]
    base_before = ah.points.copy()
    api.map_to_ellipse(ah, bh)
    assert np.array_equal(ah.points, base_before) and np.abs(bh.points - want).max() < ELLIPSE_HEX8_MAX_M
    # a target reaching outside the base raises before anything is written
    a = synth.earth_chunk(order=2, nlat=4, nlon=4, nrad=(2, 2), **ELL)
    outside = synth.earth_chunk(order=2, nlat=5, nlon=6, nrad=(3, 3), lat=(-12.0, 8.0))
    mesh = api.GllMesh(outside["points"], 2, {"z_node_1D": outside["z_node_1D"]})
    with pytest.raises(ValueError, match="points could not find an enclosing element"):
        api.map_to_ellipse(api.GllMesh(a["points"], 2, {"z_node_1D": a["z_node_1D"]}), mesh)
    assert np.array_equal(mesh.gll_points, outside["points"])
