"""Grid import, the parts that need no GPU: the NumPy statement of mm_sample_grid against scipy, RegularGrid's netCDF
round trip, the host-side preparation of the axes, and the argument errors, which are raised before a device is asked for."""
import numpy as np
import pytest

import grid_import_cases as G
from multimesh_amd import api, io as mio, synth


def test_statement_agrees_with_scipy():
    """20 000 interior points of the 7 x 9 x 11 grid (non-uniform depths) against RegularGridInterpolator.  Seven nested
    lerps of three roundings each: about 20 ulp of max|g| (4e-15 relative); the bound is 1e-13 max|g|."""
    from scipy.interpolate import RegularGridInterpolator

    g = G.grid_values(1)[0]
    rng = np.random.default_rng(1)
    D = rng.uniform(G.DEPTH[0], G.DEPTH[-1], 20_000)
    LA = rng.uniform(G.LAT[0], G.LAT[-1], 20_000)
    LO = rng.uniform(G.LON[0], G.LON[-1], 20_000)
    got, nmissing, inside = G.sample(g[None], G.DEPTH, G.LAT, G.LON, D, LA, LO)
    want = RegularGridInterpolator((G.DEPTH, G.LAT, G.LON), g)(np.stack([D, LA, LO], axis=1))
    err = np.abs(got[0] - want).max()
    print(f"max |statement - scipy| = {err:.2e} at max|g| = {np.abs(g).max():.2f}")
    assert nmissing == 0 and inside.all()
    assert err <= 1e-13 * np.abs(g).max()


def test_statement_on_the_axis_points():
    lld = G.latlondepth(G.AXIS_POINTS * 6_000_000.0)
    assert np.array_equal(lld[:, :2], G.AXIS_LATLON)
    assert np.array_equal(lld[:6, 2], np.full(6, 371_000.0)) and lld[6, 2] == 6_371_000.0
    x = np.random.default_rng(0).uniform(-4.0, 4.0, 1000)
    assert np.array_equal(np.rad2deg(x), x * G.RAD2DEG)


def test_statement_inverts_latlondepth_to_xyz():
    rng = np.random.default_rng(2)
    lld = np.stack([rng.uniform(-89, 89, 500), rng.uniform(-179, 179, 500), rng.uniform(0, 2.8e6, 500)], axis=1)
    back = G.latlondepth(api.latlondepth_to_xyz(lld))
    assert np.abs(back[:, :2] - lld[:, :2]).max() < 1e-11 and np.abs(back[:, 2] - lld[:, 2]).max() < 1e-8


def _grid(depth=G.DEPTH, lat=G.LAT, lon=G.LON, ncomp=2, seed=5):
    vals = G.grid_values(ncomp, (len(depth), len(lat), len(lon)), seed)
    return api.RegularGrid(depth, lat, lon, {f"P{c}": vals[c] for c in range(ncomp)})


def test_netcdf_round_trip(tmp_path):
    grid = _grid()
    grid.data_vars["P1"][2, 3, 4] = np.nan
    grid.data_vars["P1"][0, 0, 0] = np.nan
    path = str(tmp_path / "cube.nc")
    grid.to_netcdf(path)
    back = api.RegularGrid.from_netcdf(path)
    for d in api.DIMS:
        assert G.same_bits(back.coords[d], grid.coords[d])
    assert list(back.data_vars) == ["P0", "P1"]
    for p in grid.data_vars:
        assert G.same_bits(back[p], grid[p])
    assert np.isnan(back["P1"][2, 3, 4]) and np.isnan(back["P1"][0, 0, 0]) and int(np.isnan(back["P1"]).sum()) == 2
    assert back.attrs["radius_in_meters"] == 6371000.0


def test_netcdf_other_dim_order_and_flags(tmp_path):
    from scipy.io import netcdf_file

    grid = _grid(ncomp=1)
    v = grid["P0"].copy()
    v[1, 2, 3] = -999.0
    v[4, 5, 6] = 1.0e30
    path = str(tmp_path / "other.nc")
    with netcdf_file(path, "w", version=2) as f:
        f.radius_in_meters = 6371000.0
        for d in ("longitude", "latitude", "depth"):
            f.createDimension(d, len(grid.coords[d]))
            f.createVariable(d, "d", (d,))[:] = grid.coords[d]
        f.createDimension("time", 2)
        f.createVariable("time", "d", ("time",))[:] = [0.0, 1.0]
        var = f.createVariable("VS", "d", ("longitude", "depth", "latitude"))
        var._FillValue = np.array([-999.0])        # (a Python float would be stored as a 32-bit attribute)
        var.missing_value = np.array([1.0e30])
        var[:] = np.transpose(v, (2, 0, 1))
        f.createVariable("surface", "d", ("latitude", "longitude"))[:] = 0.0
    back = api.RegularGrid.from_netcdf(path)
    assert list(back.data_vars) == ["VS"] and back["VS"].shape == v.shape
    want = v.copy()
    want[1, 2, 3] = want[4, 5, 6] = np.nan
    assert G.same_bits(back["VS"], want)


def _statement_on(prep, lld, mode="fill"):
    depth, lat, lon, data, _, periodic = prep
    return G.sample(data, depth, lat, lon, lld[:, 2], lld[:, 0], lld[:, 1], mode, np.nan, periodic)


def test_descending_axes_give_the_ascending_values():
    grid = _grid()
    lld = G.latlondepth(G.chunk_points(500))
    want, miss, _ = _statement_on(api.prepare_regular_grid(grid), lld)
    assert 0 < miss < 500
    for flip in ((0,), (1,), (0, 1, 2)):
        coords = [grid.coords[d][::-1] if a in flip else grid.coords[d] for a, d in enumerate(api.DIMS)]
        twin = api.RegularGrid(*coords, {p: np.flip(v, axis=flip) for p, v in grid.data_vars.items()})
        prep = api.prepare_regular_grid(twin)
        assert all((np.diff(a) > 0).all() for a in prep[:3]) and not prep[5]
        got, miss_t, _ = _statement_on(prep, lld)
        assert miss_t == miss and G.same_bits(got, want)


def test_periodic_detection_and_extension():
    lat, depth = np.linspace(-90.0, 90.0, 73), np.array([0.0, 1.0e6])
    lon_a = np.arange(0.0, 360.0, 2.5)
    a = api.RegularGrid(depth, lat, lon_a, {"v": G.periodic_field(lat, lon_a, depth)})
    d, la, lo, data, _, periodic = api.prepare_regular_grid(a)
    assert periodic and len(lo) == 145 and lo[-1] == 360.0 and data.shape == (1, 2, 73, 145)
    assert np.array_equal(data[..., -1], data[..., 0]) and np.array_equal(data[0, :, :, :-1], a["v"])
    lon_b = np.linspace(-180.0, 180.0, 145)
    b = api.RegularGrid(depth, lat, lon_b, {"v": G.periodic_field(lat, lon_b, depth)})
    d, la, lo, data, _, periodic = api.prepare_regular_grid(b)
    assert periodic and np.array_equal(lo, lon_b) and np.array_equal(data[0], b["v"])
    # -180 ... 180 whose ends differ is an ordinary axis; so is a regional one
    c = api.RegularGrid(depth, lat, lon_b, {"v": b["v"] + lon_b[None, None, :]})
    assert not api.prepare_regular_grid(c)[5]
    lon_r = np.linspace(-8.0, 8.0, 9)
    r = api.RegularGrid(depth, lat, lon_r, {"v": G.periodic_field(lat, lon_r, depth)})
    d, la, lo, data, _, periodic = api.prepare_regular_grid(r)
    assert not periodic and np.array_equal(lo, lon_r)
    # a global axis that starts outside [-360, 180] is shifted by whole turns
    lon_s = lon_a + 720.0
    s = api.RegularGrid(depth, lat, lon_s, {"v": a["v"]})
    d, la, lo, data, _, periodic = api.prepare_regular_grid(s)
    assert periodic and lo[0] == 0.0 and lo[-1] == 360.0
    # asked for explicitly, a regional axis is closed too; refused when told not to wrap
    assert api.prepare_regular_grid(r, lon_periodic=True)[2][-1] == 352.0
    assert not api.prepare_regular_grid(a, lon_periodic=False)[5]


def test_validation_errors():
    grid = _grid()
    pts = G.chunk_points(10)
    bad = api.RegularGrid(G.DEPTH, np.array([-6.0, -3.0, -4.0, 0.0, 1.0, 2.0, 3.0, 4.0, 6.0]), G.LON, dict(grid.data_vars))
    with pytest.raises(ValueError, match="monotone"):
        api.sample_regular_grid(bad, pts)
    bad = api.RegularGrid(G.DEPTH, G.LAT, G.LON, dict(grid.data_vars))
    bad.coords["longitude"] = np.where(np.arange(11) == 3, np.nan, G.LON)
    with pytest.raises(ValueError, match="finite"):
        api.sample_regular_grid(bad, pts)
    bad = api.RegularGrid(G.DEPTH, G.LAT, G.LON, dict(grid.data_vars))
    bad.data_vars["P0"] = np.zeros((7, 9, 10))
    with pytest.raises(ValueError, match="shape"):
        api.sample_regular_grid(bad, pts)
    with pytest.raises(ValueError, match="not in the grid"):
        api.sample_regular_grid(grid, pts, parameters=["VS"])
    with pytest.raises(ValueError, match="keep"):
        api.sample_regular_grid(grid, pts, outside="keep")

    chunk = synth.earth_chunk(1, nlat=2, nlon=2)
    mesh = api.GllMesh(chunk["points"], 1, {"P0": np.zeros(chunk["points"].shape[:2])})
    with pytest.raises(ValueError, match="no field"):
        api.import_regular_grid(grid, mesh)                       # keep: P1 is not on the mesh
    assert list(mesh.element_nodal_fields) == ["P0"] and not mesh.element_nodal_fields["P0"].any()
    with pytest.raises(ValueError, match="outside"):
        api.import_regular_grid(grid, mesh, outside="nearest")

    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=chunk["points"])
    model = np.random.default_rng(0).normal(size=(chunk["points"].shape[0], 2, 8))
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=model), ["P0", "RHO"])
    with pytest.raises(ValueError, match="not in MODEL/data"):
        api.import_regular_grid(grid, f, outside="fill")          # P1 is not in the file
    assert G.same_bits(f["MODEL/data"][()], model)
