"""Regular lat/lon/depth grids without a GPU: the device's target arithmetic restated on the host against
latlondepth_to_xyz, extent validation, the netCDF writer, and the layout of the depth slice."""
import numpy as np
import pytest

from multimesh_amd import api, helpers


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def kernel_points(lat, lon, depth, paired):
    """What sample_points_kernel forms, restated: target (d, h) = ((r * sin colat) * cos lon, (r * sin colat) * sin lon,
    r * cos colat) from the host's 1-D tables, column h = i * nlon + j (grid) or h (path) -> f64[D, H, 3]."""
    lat_t, lon_t, r = api.column_tables(lat, lon, depth)
    if paired:
        a = b = np.arange(len(lat))
    else:
        a = np.repeat(np.arange(len(lat)), len(lon))
        b = np.tile(np.arange(len(lon)), len(lat))
    rs = r[:, None] * lat_t[a, 0][None, :]
    return np.stack([rs * lon_t[b, 0][None, :], rs * lon_t[b, 1][None, :], r[:, None] * lat_t[a, 1][None, :]], axis=-1)


def reference_points(lat, lon, depth, paired):
    """latlondepth_to_xyz of the grid's rows in grid order (depth, latitude, longitude) or of the path's."""
    if paired:
        d, h = np.meshgrid(np.arange(len(depth)), np.arange(len(lat)), indexing="ij")
        rows = np.stack([lat[h], lon[h], depth[d]], axis=-1).reshape(-1, 3)
        ncol = len(lat)
    else:
        D, LA, LO = np.meshgrid(depth, lat, lon, indexing="ij")
        rows = np.stack([LA, LO, D], axis=-1).reshape(-1, 3)
        ncol = len(lat) * len(lon)
    return api.latlondepth_to_xyz(rows).reshape(len(depth), ncol, 3)


GRIDS = [
    ((-90.0, 90.0, 37), (-180.0, 180.0, 73), (0.0, 2_000_000.0, 5)),    # poles and both ends of the longitudes
    ((-90.0, 90.0, 181), (-180.0, 179.5, 720), (660_000.0, 660_000.0, 1)),
    ((12.25, 12.25, 1), (-180.0, 180.0, 7), (-4000.0, 6_371_000.0, 3)),  # num = 1, depths up to the centre
    ((-33.3, 41.7, 9), (77.7, 77.7, 1), (35_000.0, 35_000.0, 1)),
    ((-89.99, 89.99, 13), (-179.99, 179.99, 11), (10.0, 2891e3, 17)),
]


@pytest.mark.parametrize("grid", GRIDS)
def test_kernel_arithmetic_is_latlondepth_to_xyz_on_a_grid(grid):
    lat, lon, depth = (np.linspace(*e) for e in grid)
    assert np.array_equal(_bits(kernel_points(lat, lon, depth, False)), _bits(reference_points(lat, lon, depth, False)))


def test_kernel_arithmetic_is_latlondepth_to_xyz_on_a_path():
    rng = np.random.default_rng(3)
    lat = np.concatenate([[-90.0, 90.0, 0.0, 45.0], rng.uniform(-90, 90, 200)])
    lon = np.concatenate([[-180.0, 180.0, 0.0, -45.0], rng.uniform(-180, 180, 200)])
    depth = np.concatenate([[0.0, -3000.0], rng.uniform(0, 6.3e6, 9)])
    assert np.array_equal(_bits(kernel_points(lat, lon, depth, True)), _bits(reference_points(lat, lon, depth, True)))
    one = slice(0, 1)
    assert np.array_equal(_bits(kernel_points(lat[one], lon[one], depth[one], True)),
                          _bits(reference_points(lat[one], lon[one], depth[one], True)))


@pytest.mark.parametrize("bad", [
    dict(lat_extent=(-10, 10, 0)), dict(lon_extent=(-10, 10, -3)), dict(depth_extent=(0, 1e5, 2.5)),
    dict(lat_extent=(np.nan, 10, 4)), dict(lon_extent=(-10, np.inf, 4)), dict(depth_extent=(-np.inf, 0, 4)),
    dict(lat_extent=(-10, 10)),
])
def test_bad_extents_raise_value_error(bad):
    args = dict(lat_extent=(-10, 10, 4), lon_extent=(-10, 10, 4), depth_extent=(0, 1e5, 3))
    args.update(bad)
    with pytest.raises(ValueError):
        api.extract_regular_grid(object(), ["VSV"], **args)   # (rejected before the mesh is looked at)


def test_bad_depth_slice_and_path_raise_value_error():
    with pytest.raises(ValueError):
        api.extract_depth_slice(object(), 100.0, 0)
    with pytest.raises(ValueError):
        api.extract_depth_slice(object(), 100.0, 5, lat_extent=(np.nan, 10))
    with pytest.raises(ValueError):
        api.extract_cross_section(object(), ["VSV"], [0.0, 1.0], [0.0], [0.0])
    with pytest.raises(ValueError):
        api.extract_cross_section(object(), ["VSV"], [0.0, np.nan], [0.0, 1.0], [0.0])


def _grid():
    depth = np.linspace(0.0, 100_000.0, 3)
    lat = np.linspace(-10.0, 10.0, 4)
    lon = np.linspace(20.0, 30.0, 5)
    rng = np.random.default_rng(0)
    a = rng.standard_normal((3, 4, 5))
    a[0, 1, 2] = a[2, 3, 4] = np.nan
    b = rng.standard_normal((3, 4, 5))
    return api.RegularGrid(depth, lat, lon, {"VSV": a, "RHO": b}, nmissing=2)


def test_regular_grid_round_trips_through_netcdf(tmp_path):
    from scipy.io import netcdf_file

    g = _grid()
    assert g.attrs == {"radius_in_meters": 6371000.0}
    assert g["VSV"].shape == (3, 4, 5) and np.array_equal(g["latitude"], np.linspace(-10.0, 10.0, 4))
    path = tmp_path / "grid.nc"
    g.to_netcdf(path)
    with netcdf_file(path, "r", mmap=False) as f:
        assert f.version_byte == 2
        assert f.dimensions == {"depth": 3, "latitude": 4, "longitude": 5}
        assert f.radius_in_meters == 6371000.0
        assert set(f.variables) == {"depth", "latitude", "longitude", "VSV", "RHO"}
        for d, unit in (("depth", b"m"), ("latitude", b"deg"), ("longitude", b"deg")):
            v = f.variables[d]
            assert v.dimensions == (d,) and v.units == unit
            assert np.array_equal(v[:], g.coords[d])
        for name in ("VSV", "RHO"):
            v = f.variables[name]
            assert v.dimensions == ("depth", "latitude", "longitude")
            assert np.array_equal(_bits(v[:]), _bits(g[name]))   # NaN kept as NaN, bit for bit
        assert np.isnan(f.variables["VSV"][0, 1, 2]) and np.isnan(f.variables["VSV"][2, 3, 4])


def test_regular_grid_too_large_for_netcdf_raises_before_writing(tmp_path):
    shape = (1, 32768, 16385)                                     # 4 GiB + 128 kiB as f64 (a view: nothing allocated)
    g = api.RegularGrid(np.zeros(1), np.zeros(shape[1]), np.zeros(shape[2]), {"VSV": np.broadcast_to(0.0, shape)})
    path = tmp_path / "big.nc"
    with pytest.raises(ValueError, match="64-bit-offset"):
        g.to_netcdf(path)
    assert not path.exists()


def test_regular_grid_rejects_wrong_shapes():
    with pytest.raises(ValueError):
        api.RegularGrid(np.zeros(2), np.zeros(3), np.zeros(4), {"VSV": np.zeros((2, 4, 3))})


def create_depthslice(depth_in_m, num, lat_extent, lon_extent):
    """reference components/plotter.py:159-187, restated."""
    lat = np.linspace(lat_extent[0], lat_extent[1], num=num)
    lon = np.linspace(lon_extent[0], lon_extent[1], num=num)
    xx, yy = np.meshgrid(lat, lon)
    return np.array((xx.ravel(), yy.ravel(), np.ones_like(yy).ravel() * depth_in_m)).T


@pytest.mark.parametrize("num", [1, 2, 7])
def test_depth_slice_follows_the_references_point_order(monkeypatch, num):
    lat_extent, lon_extent = (-30.0, 60.0), (-170.0, 10.0)
    seen = {}

    def fake_sample(mesh, parameters, lat, lon, depth, paired, *rest):
        # the value of a target: its column in grid order (latitude i * nlon + longitude j)
        seen.update(lat=lat, lon=lon, depth=depth, paired=paired, parameters=parameters)
        return np.arange(len(lat) * len(lon), dtype=np.float64).reshape(1, 1, -1), 0

    monkeypatch.setattr(api.grids, "_sample", fake_sample)
    vals = api.extract_depth_slice(object(), 35.5, num, lat_extent, lon_extent, parameter="VPV")
    assert vals.shape == (num, num) and not seen["paired"] and seen["parameters"] == ["VPV"]
    assert np.array_equal(seen["depth"], [35_500.0])
    ref = create_depthslice(35.5 * 1000.0, num, lat_extent, lon_extent)
    h = vals.ravel().astype(np.int64)
    nlon = len(seen["lon"])
    assert np.array_equal(seen["lat"][h // nlon], ref[:, 0])
    assert np.array_equal(seen["lon"][h % nlon], ref[:, 1])
    assert np.array_equal(np.full(num * num, seen["depth"][0]), ref[:, 2])


def test_depth_slice_percentages_use_the_points_inside(monkeypatch):
    v = np.array([[1.0, 2.0], [np.nan, 3.0]])   # [lat, lon]; one point outside the mesh

    monkeypatch.setattr(api.grids, "_sample", lambda *a: (v.reshape(1, 1, -1).copy(), 1))
    got = api.extract_depth_slice(object(), 10.0, 2, diff_percentage=True, fill_value=-1.0)
    want = (v.T - 2.0) / 2.0 * 100.0
    want[np.isnan(want)] = -1.0
    assert np.array_equal(got, want)
    flat = np.array([[5.0, 5.0], [5.0, np.nan]])
    monkeypatch.setattr(api.grids, "_sample", lambda *a: (flat.reshape(1, 1, -1).copy(), 1))
    got = api.extract_depth_slice(object(), 10.0, 2, diff_percentage=True)
    assert np.array_equal(np.isnan(got), np.isnan(flat.T)) and np.all(got[~np.isnan(got)] == 0.0)


def test_sample_chunk_budget_constants_match_the_header():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                             "multimesh_hip.h")).read()
    assert re.search(r"#define MM_SAMPLE_CHUNK_BYTES \(\(int64_t\)1 << 34\)", text)
    assert helpers.MM_SAMPLE_CHUNK_BYTES == 1 << 34
    assert re.search(rf"#define MM_SAMPLE_STAGE_BYTES {helpers.MM_SAMPLE_STAGE_BYTES}\b", text)
