"""Sampling on latitude x longitude x depth columns: extract_regular_grid (reference api.py:600-642,
interpolator.py:1600-1646), the depth slice plot_depth_slice samples (plotter.py:89-110, :159-187) and the radius x path
section of plot_cross_section (plotter.py:360-391).  The targets are generated on the device
(Context.sample_columns_gll); the host only computes the 1-D factors below.  Plotting is not part of this."""
import numpy as np

from .. import io as mio
from ..device import _Released, default_context
from ..mesh import HexMesh
from ._common import GllMesh, ImportTarget, _order_from_point_count, is_mesh, named_fields, points_of
from .earth import _sphere_mapped
from .mass import _device_mass, _hex8_mass

DIMS = ("depth", "latitude", "longitude")
UNITS = {"depth": "m", "latitude": "deg", "longitude": "deg"}


def _extent(extent, name):
    """``np.linspace(min, max, num)`` of an extent ``(min, max, num)``, as the reference forms its axes."""
    try:
        lo, hi, num = extent
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be (min, max, num), got {extent!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"{name}: the bounds must be finite, got {extent!r}")
    if isinstance(num, (bool, np.bool_)) or not float(num).is_integer() or int(num) < 1:
        raise ValueError(f"{name}: num must be an integer >= 1, got {num!r}")
    return np.linspace(lo, hi, int(num))


def column_tables(lat, lon, depth):
    """``(lat_table f64[nlat, 2], lon_table f64[nlon, 2], radius f64[D])`` as :meth:`Context.sample_columns_gll`
    reads them: (sin colat, cos colat), (cos lon, sin lon) and 6371000 - depth, computed with the expressions of
    :func:`latlondepth_to_xyz` on columns of [n, 3] arrays like its own (so that NumPy runs the same loops).  The
    device forms ``((r * sin colat) * cos lon, (r * sin colat) * sin lon, r * cos colat)`` from them: that
    function's rows bit for bit."""
    def rows(values, col):
        a = np.zeros((len(values), 3))
        a[:, col] = np.asarray(values, dtype=np.float64)
        return a

    la, lo, de = rows(lat, 0), rows(lon, 1), rows(depth, 2)
    colat = np.deg2rad(90.0 - la[:, 0])
    lonr = np.deg2rad(lo[:, 1])
    lat_table = np.ascontiguousarray(np.stack([np.sin(colat), np.cos(colat)], axis=1))
    lon_table = np.ascontiguousarray(np.stack([np.cos(lonr), np.sin(lonr)], axis=1))
    return lat_table, lon_table, np.ascontiguousarray(6371000.0 - de[:, 2])


def _as_gll_mesh(mesh, parameters, make_spherical):
    """A :class:`GllMesh` as it is; a Salvus model (file or h5py-like object) read into one: its coordinates, the named
    parameters and, for ``make_spherical``, its ``z_node_1D``."""
    if isinstance(mesh, GllMesh):
        return mesh
    points, data, names = mio.load_hdf5_params_to_memory(mesh)
    missing = [p for p in parameters if p not in names]
    if missing:
        raise ValueError(f"parameters {missing} are not in the model (it holds {names})")
    P = points.shape[1]
    order = _order_from_point_count(P, 3)
    if points.ndim != 3 or points.shape[2] != 3 or (order + 1) ** 3 != P:
        raise ValueError(f"MODEL/coordinates must be [nelem, (order+1)^3, 3], got {points.shape}")
    wanted = set(parameters) | ({"z_node_1D"} if make_spherical and "z_node_1D" in names else set())
    return GllMesh(points, order, {p: data[:, names.index(p), :] for p in wanted})


def _gll_model(mesh, parameters, make_spherical, ctx):
    """(gll_points f64[E, P, 3] (host or device), shape_order, fields f64[C, E, P]) of a :class:`GllMesh` or of a Salvus
    model (a file, or an h5py-like object read through :func:`multimesh_amd.io.load_hdf5_params_to_memory`, whose
    parameters are picked by name from ``DIMENSION_LABELS``).  ``make_spherical`` maps a copy onto the mesh's 1-D sphere."""
    parameters = mio.pick_parameters(parameters)
    mesh = _as_gll_mesh(mesh, parameters, make_spherical)
    fields = np.stack([np.asarray(mesh.element_nodal_fields[p], dtype=np.float64) for p in parameters])
    gll_points = _sphere_mapped(mesh, ctx) if make_spherical else mesh.gll_points
    return gll_points, mesh.shape_order, fields


def _sample(mesh, parameters, lat, lon, depth, paired, make_spherical, nelem_to_search, tolerance, fill_value,
            chunk_points, context):
    """values f64[C, D, H] (host) and the number of targets without an element."""
    ctx = context or default_context()
    gll_points, order, fields = _gll_model(mesh, parameters, make_spherical, ctx)
    lat_t, lon_t, radius = column_tables(lat, lon, depth)
    values, nmissing = ctx.sample_columns_gll(order, gll_points, fields, lat_t, lon_t, radius, paired=paired,
                                              nelem_to_search=nelem_to_search, tolerance=tolerance,
                                              fill_value=fill_value, chunk_points=chunk_points)
    return values.numpy(), nmissing


class RegularGrid:
    """What reference ``extract_regular_grid`` returns as an xarray Dataset (``utils.create_xarray_dataset``,
    utils.py:619-646), without xarray: ``coords`` depth (m), latitude and longitude (deg); ``data_vars`` one f64
    array per parameter with dims (depth, latitude, longitude); ``attrs`` {"radius_in_meters": 6371000.0};
    ``nmissing`` targets outside the mesh, which hold ``fill_value``.  ``grid[name]`` returns a variable or a
    coordinate."""

    dims = DIMS

    def __init__(self, depth, latitude, longitude, data_vars, nmissing=0, fill_value=np.nan):
        self.coords = {"depth": np.asarray(depth, dtype=np.float64), "latitude": np.asarray(latitude, dtype=np.float64),
                       "longitude": np.asarray(longitude, dtype=np.float64)}
        shape = tuple(len(self.coords[d]) for d in DIMS)
        self.data_vars = {}
        for name, v in data_vars.items():
            v = np.asarray(v, dtype=np.float64)
            if v.shape != shape:
                raise ValueError(f"{name}: shape {v.shape}, the grid is {shape}")
            self.data_vars[name] = v
        self.attrs = {"radius_in_meters": 6371000.0}
        self.nmissing = int(nmissing)
        self.fill_value = float(fill_value)

    def __getitem__(self, name):
        return self.data_vars[name] if name in self.data_vars else self.coords[name]

    def to_netcdf(self, path):
        """Classic netCDF with 64-bit offsets (``scipy.io.netcdf_file(version=2)``): dimensions and coordinate
        variables depth / latitude / longitude with their ``units``, the global ``radius_in_meters``, one f64 variable
        per parameter over (depth, latitude, longitude) with ``_FillValue`` = the fill value (NaN stays NaN).  A
        variable the format cannot hold (4 GiB - 4 bytes at most) raises ``ValueError`` before anything is written."""
        from scipy.io import netcdf_file

        limit = 2 ** 32 - 4
        for name, v in list(self.coords.items()) + list(self.data_vars.items()):
            if v.nbytes > limit:
                raise ValueError(f"variable {name!r} needs {v.nbytes} bytes; the 64-bit-offset netCDF format holds "
                                 f"at most {limit} per variable: write a smaller grid (or fewer depths) per file")
        clash = set(self.data_vars) & set(DIMS)
        if clash:
            raise ValueError(f"parameter names {sorted(clash)} clash with the coordinates")
        with netcdf_file(path, "w", version=2) as f:
            f.radius_in_meters = self.attrs["radius_in_meters"]
            for d in DIMS:
                f.createDimension(d, len(self.coords[d]))
                c = f.createVariable(d, "d", (d,))
                c[:] = self.coords[d]
                c.units = UNITS[d]
            for name, v in self.data_vars.items():
                var = f.createVariable(name, "d", DIMS)
                var._FillValue = self.fill_value
                var[:] = v

    @classmethod
    def from_netcdf(cls, path):
        """The inverse of :meth:`to_netcdf`, for any classic netCDF cube (``scipy.io.netcdf_file``): the coordinate
        variables ``depth``, ``latitude`` and ``longitude``, and every other variable over exactly those three
        dimensions, in any order -- transposed to (depth, latitude, longitude).  Values equal to a variable's
        ``_FillValue`` or ``missing_value`` become NaN (``fill_value`` of the result is NaN); the global
        ``radius_in_meters`` is kept when the file has one.  Other variables are ignored."""
        from scipy.io import netcdf_file

        with netcdf_file(path, "r", mmap=False) as f:
            missing = [d for d in DIMS if d not in f.variables]
            if missing:
                raise ValueError(f"{path}: no coordinate variable(s) {missing}")
            coords = {d: np.array(f.variables[d][:], dtype=np.float64).reshape(-1) for d in DIMS}
            data_vars = {}
            for name, var in f.variables.items():
                if name in DIMS or sorted(var.dimensions) != sorted(DIMS):
                    continue
                v = np.array(var[:], dtype=np.float64)
                for attr in ("_FillValue", "missing_value"):
                    flag = getattr(var, attr, None)
                    if flag is not None:
                        flag = np.asarray(flag, dtype=np.float64).reshape(-1)
                        v[np.isin(v, flag[~np.isnan(flag)])] = np.nan
                data_vars[name] = np.ascontiguousarray(np.transpose(v, [var.dimensions.index(d) for d in DIMS]))
            radius = getattr(f, "radius_in_meters", None)
        grid = cls(coords["depth"], coords["latitude"], coords["longitude"], data_vars)
        if radius is not None:
            grid.attrs["radius_in_meters"] = float(np.asarray(radius).reshape(-1)[0])
        return grid

    def __repr__(self):
        shape = ", ".join(f"{d}: {len(self.coords[d])}" for d in DIMS)
        return f"<RegularGrid ({shape}) {list(self.data_vars)} nmissing={self.nmissing}>"


def extract_regular_grid(mesh, parameters, lat_extent, lon_extent, depth_extent, save_to_netcdf=False, netcdf_path=None,
                         *, make_spherical=False, nelem_to_search=25, tolerance=1.05, fill_value=np.nan,
                         chunk_points=None, context=None):
    """A GLL model on a regular latitude x longitude x depth grid (reference api.py:600-642, interpolator.py:1600-1646).

    ``mesh``: a :class:`GllMesh`, a Salvus model file, or an h5py-like object (parameters picked by name from
    ``MODEL/data``'s ``DIMENSION_LABELS``).  Extents are ``(min, max, num)`` through ``np.linspace``; latitudes are
    geocentric degrees and depths metres below 6371 km (:func:`latlondepth_to_xyz`).  Every grid point is
    interpolated as :meth:`Context.interpolate_gll` interpolates it (centroid kNN over ``nelem_to_search``,
    acceptance at ``tolerance``); points outside the mesh hold ``fill_value``.  The points are generated on the
    device in chunks (``chunk_points``; None: a fixed scratch budget).  ``make_spherical`` samples a copy of the mesh
    mapped onto its 1-D sphere (:func:`map_to_sphere`); the caller's arrays are not changed.

    Returns a :class:`RegularGrid` (the reference returns an xarray Dataset; xarray is not used here), or, with
    ``save_to_netcdf``, writes it to ``netcdf_path`` (:meth:`RegularGrid.to_netcdf`) and returns None."""
    lat = _extent(lat_extent, "lat_extent")
    lon = _extent(lon_extent, "lon_extent")
    depth = _extent(depth_extent, "depth_extent")
    if save_to_netcdf and netcdf_path is None:
        raise ValueError("save_to_netcdf needs a netcdf_path")
    parameters = mio.pick_parameters(parameters)
    values, nmissing = _sample(mesh, parameters, lat, lon, depth, False, make_spherical, nelem_to_search, tolerance,
                               fill_value, chunk_points, context)
    shape = (len(depth), len(lat), len(lon))
    grid = RegularGrid(depth, lat, lon, {p: values[c].reshape(shape) for c, p in enumerate(parameters)}, nmissing,
                       fill_value)
    if save_to_netcdf:
        grid.to_netcdf(netcdf_path)
        return None
    return grid


def extract_depth_slice(mesh, depth_in_km, num, lat_extent=(-90.0, 90.0), lon_extent=(-180.0, 180.0), parameter="VSV",
                        diff_percentage=False, *, make_spherical=False, nelem_to_search=25, tolerance=1.05,
                        fill_value=np.nan, chunk_points=None, context=None):
    """The ``num x num`` array reference ``plot_depth_slice`` plots (plotter.py:89-110): ``parameter`` at
    ``depth_in_km`` on ``np.linspace`` latitudes and longitudes, in the reference's layout -- the points of
    ``_create_depthslice`` (``np.meshgrid(lat, lon)``, raveled) reshaped to (num, num), i.e. ``[longitude, latitude]``.
    ``diff_percentage``: ``(v - mean) / mean * 100`` with the mean over the points inside the mesh, and all zeros
    when the largest deviation is below 0.1 % (a 1-D model), as the reference does.  Points outside the mesh hold
    ``fill_value``."""
    lat = _extent((lat_extent[0], lat_extent[1], num), "lat_extent")
    lon = _extent((lon_extent[0], lon_extent[1], num), "lon_extent")
    depth = np.array([depth_in_km * 1000.0])
    values, _ = _sample(mesh, [parameter], lat, lon, depth, False, make_spherical, nelem_to_search, tolerance, np.nan,
                        chunk_points, context)
    vals = np.ascontiguousarray(values[0, 0].reshape(len(lat), len(lon)).T)   # [lat, lon] -> the reference's [lon, lat]
    found = ~np.isnan(vals)
    if diff_percentage and found.any():
        mean = np.mean(vals[found])
        vals = (vals - mean) / mean * 100.0
        if np.max(np.abs(vals[found])) < 0.1:   # (reference plotter.py:108-109)
            vals[found] = 0.0
    vals[~found] = fill_value
    return vals


def extract_cross_section(mesh, parameters, lats, lons, depths, make_spherical=True, *, nelem_to_search=25,
                          tolerance=1.05, fill_value=np.nan, chunk_points=None, context=None):
    """A radius x path section, what reference ``plot_cross_section`` samples (plotter.py:360-391):
    values f64[C, ndepth, npath] at the points (``lats[h]``, ``lons[h]``, ``depths[d]``) -> :func:`latlondepth_to_xyz`.

    The reference builds its path as a WGS84 geodesic between two points (``greatcircle_points`` through
    geographiclib) and converts it to geocentric latitudes; that library is not used here, so the caller passes the
    path itself: ``lats`` (geocentric degrees) and ``lons`` of equal length, and ``depths`` in metres.
    ``make_spherical`` (default True, as plotter.py:385-390) samples a copy of the mesh mapped onto its 1-D sphere.
    Points outside the mesh hold ``fill_value``; the reference's per-radius percentage is plotting and not done."""
    lats = np.atleast_1d(np.asarray(lats, dtype=np.float64))
    lons = np.atleast_1d(np.asarray(lons, dtype=np.float64))
    depths = np.atleast_1d(np.asarray(depths, dtype=np.float64))
    if lats.ndim != 1 or lons.ndim != 1 or depths.ndim != 1 or len(lats) != len(lons):
        raise ValueError("lats and lons must be 1-D of the same length, depths 1-D")
    if not (np.isfinite(lats).all() and np.isfinite(lons).all() and np.isfinite(depths).all()):
        raise ValueError("the path and the depths must be finite")
    values, _ = _sample(mesh, parameters, lats, lons, depths, True, make_spherical, nelem_to_search, tolerance,
                        fill_value, chunk_points, context)
    return values


# --------------------------------------------------------------------------------------------------------------------
# The other direction: a regular latitude x longitude x depth grid onto the points of a mesh (Context.sample_grid).  The
# host only prepares the grid-sized arrays below; the mesh-sized work -- xyz -> lat/lon/depth, the cell search and the
# trilinear values -- runs on the device.
def _ascending_axis(name, values):
    """(axis ascending, flipped?) of a coordinate; ``ValueError`` unless it is 1-D, finite and strictly monotone."""
    a = np.array(values, dtype=np.float64)
    if a.ndim != 1 or a.size < 1 or not np.isfinite(a).all():
        raise ValueError(f"the {name} axis must be 1-D, finite and not empty")
    d = np.diff(a)
    if (d > 0).all():
        return a, False
    if (d < 0).all():
        return np.ascontiguousarray(a[::-1]), True
    raise ValueError(f"the {name} axis is not strictly monotone")


def _is_global_longitude(lon, data):
    """A longitude axis that goes once round: its span plus one mean spacing is 360 (within 1e-6 of a spacing), or its
    span is 360 and the first and the last column hold the same data."""
    if len(lon) < 2:
        return False
    span = lon[-1] - lon[0]
    spacing = span / (len(lon) - 1)
    if abs(span + spacing - 360.0) <= 1e-6 * spacing:
        return True
    return abs(span - 360.0) <= 1e-6 * spacing and np.array_equal(data[..., 0], data[..., -1], equal_nan=True)


def prepare_regular_grid(grid, parameters=None, lon_periodic=None):
    """``(depth, lat, lon, data f64[C, D, LA, LO], parameters, periodic)`` as :meth:`Context.sample_grid` takes them, from
    a :class:`RegularGrid`: descending axes are flipped to ascending with their data, an axis that is not strictly
    monotone or not finite raises ``ValueError``.  ``lon_periodic=None`` detects a global longitude axis
    (:func:`_is_global_longitude`).  A periodic axis is shifted by a multiple of 360 to start in [-180, 180) when it
    starts outside [-360, 180], and closed: when it ends before ``lon[0] + 360``, the column ``lon[0] + 360`` with the
    data of column 0 is appended; an end within rounding of it becomes exactly that."""
    parameters = list(grid.data_vars) if parameters is None else mio.pick_parameters(parameters)
    unknown = [p for p in parameters if p not in grid.data_vars]
    if unknown:
        raise ValueError(f"parameters {unknown} are not in the grid (it holds {list(grid.data_vars)})")
    axes, flipped = {}, {}
    for d in DIMS:
        axes[d], flipped[d] = _ascending_axis(d, grid.coords[d])
    shape = tuple(len(axes[d]) for d in DIMS)
    fields = []
    for p in parameters:
        v = np.asarray(grid.data_vars[p], dtype=np.float64)
        if v.shape != shape:
            raise ValueError(f"{p}: shape {v.shape}, the grid is {shape}")
        fields.append(v)
    data = np.stack(fields) if fields else np.zeros((0,) + shape)
    for ax, d in enumerate(DIMS):
        if flipped[d]:
            data = np.flip(data, axis=ax + 1)
    lon = axes["longitude"]
    periodic = _is_global_longitude(lon, data) if lon_periodic is None else bool(lon_periodic)
    if periodic:
        if not -360.0 <= lon[0] <= 180.0:
            lon = lon - 360.0 * np.floor((lon[0] + 180.0) / 360.0)
        end = lon[0] + 360.0
        spacing = (lon[-1] - lon[0]) / max(len(lon) - 1, 1)
        if lon[-1] > end + 1e-6 * spacing:
            raise ValueError("a periodic longitude axis must not span more than 360 degrees")
        if len(lon) > 1 and abs(lon[-1] - end) <= 1e-6 * spacing:
            lon = np.concatenate([lon[:-1], [end]])
        else:
            lon = np.concatenate([lon, [end]])
            data = np.concatenate([data, data[..., :1]], axis=-1)
        if not (np.diff(lon) > 0).all():
            raise ValueError("the longitude axis cannot be closed at lon[0] + 360")
    return axes["depth"], axes["latitude"], lon, np.ascontiguousarray(data), parameters, periodic


def sample_regular_grid(grid, points, parameters=None, outside="fill", fill_value=np.nan, lon_periodic=None, context=None):
    """A :class:`RegularGrid` sampled at ``points`` f64[N, 3] (metres, Earth-centred): trilinear in (depth, geocentric
    latitude, longitude), with ``depth = 6371000 - |p|`` -- the inverse of :func:`latlondepth_to_xyz`, evaluated on the
    device (:meth:`Context.sample_grid`, where the arithmetic is stated).  ``parameters``: names of ``grid.data_vars``
    (None: all).  ``outside``: "fill" (points outside the grid get ``fill_value``) or "clamp" (the edge value extends).
    ``lon_periodic``: None detects a global longitude axis (``0 ... 357.5``, or ``-180 ... 180`` with the first column
    repeated), which then wraps; see :func:`prepare_regular_grid` for what is done to the axes.  A NaN node makes the
    values of its eight cells NaN.  Returns (values f64[C, N], number of points outside the grid)."""
    depth, lat, lon, data, _, periodic = prepare_regular_grid(grid, parameters, lon_periodic)
    if outside == "keep":
        raise ValueError('outside="keep" needs values to keep: use import_regular_grid, or Context.sample_grid with out')
    ctx = context or default_context()
    values, nmissing = ctx.sample_grid(points, data, depth, lat, lon, outside=outside, fill_value=fill_value,
                                       lon_periodic=periodic)
    return values.numpy(), nmissing


def _need_3d(points, who):
    if np.shape(points)[-1] != 3:
        raise ValueError(f"{who} needs a 3-D mesh (points of shape {np.shape(points)})")


def import_regular_grid(grid, mesh, parameters=None, outside="keep", fill_value=np.nan, lon_periodic=None,
                        make_spherical=False, context=None):
    """A gridded model onto a mesh: every node of ``mesh`` gets the value of ``grid`` at its (geocentric latitude,
    longitude, depth = 6371000 - |p|), as :func:`sample_regular_grid` gives it.

    ``grid``: a :class:`RegularGrid` or the path of a netCDF file (:meth:`RegularGrid.from_netcdf`).  ``mesh``:

    * a :class:`GllMesh`: ``element_nodal_fields[p]`` becomes a new f64[E, P] array;
    * a :class:`HexMesh`: nodal fields through ``attach_field``;
    * a writable Salvus model -- an h5py-like object (:class:`multimesh_amd.io.MemoryH5`) or, with h5py, a path: the
      columns of ``MODEL/data`` that ``DIMENSION_LABELS`` names are overwritten in place, every other column stays as it
      is.  A parameter the labels do not hold raises ``ValueError`` before anything is written.

    ``parameters``: None = every variable of the grid.  ``outside``: "keep" (default: nodes outside the grid keep the
    mesh's value; the field must exist, else ``ValueError``), "fill" or "clamp".  ``make_spherical`` evaluates the
    coordinates on a copy of the mesh mapped onto its 1-D sphere (:func:`map_to_sphere`), as the extract drivers do; the
    mesh's own coordinates never change.  Returns the number of nodes outside the grid."""
    if outside not in ("keep", "fill", "clamp"):
        raise ValueError(f'outside must be "keep", "fill" or "clamp", got {outside!r}')
    if not isinstance(grid, RegularGrid):
        grid = RegularGrid.from_netcdf(grid)
    depth, lat, lon, data, parameters, periodic = prepare_regular_grid(grid, parameters, lon_periodic)

    def ctx():   # (asked for when the first kernel runs: what is wrong with the arguments is said without a device)
        return context or default_context()

    with ImportTarget(mesh) as target:
        _need_3d(target.points, "import_regular_grid")
        target.require(parameters, values=outside == "keep")
        out = target.existing(parameters) if outside == "keep" else None
        points = _sphere_mapped(target.sphere_mesh(), ctx()) if make_spherical else target.points
        values, nmissing = ctx().sample_grid(points, data, depth, lat, lon, outside=outside, fill_value=fill_value,
                                             lon_periodic=periodic, out=out)
        target.write(parameters, values.numpy().reshape((len(parameters),) + target.lead))
    return nmissing


# --------------------------------------------------------------------------------------------------------------------
# The grid import as an operator G (Context.grid_operator: ids int64[N, 8], w f64[N, 8] into the prepared cube), and its
# transpose.  The two functions below are the host's part of it, pure NumPy of grid size: between the caller's layout and
# the prepared one (axes ascending, a periodic axis closed by one more column).
TRANSPOSE_MAX_ENTRIES = 2 ** 31      # mm_transpose_create_nodes: npoints * 8 must stay below this


def to_prepared_layout(values, flipped, appended):
    """A cube f64[..., D, LA, LO] in the caller's layout as :func:`prepare_regular_grid` lays it out: the axes named in
    ``flipped`` (three booleans: depth, latitude, longitude) reversed and, with ``appended``, column 0 repeated behind
    the last longitude."""
    v = np.asarray(values, dtype=np.float64)
    for ax, f in zip((-3, -2, -1), flipped):
        if f:
            v = np.flip(v, axis=ax)
    if appended:
        v = np.concatenate([v, v[..., :1]], axis=-1)
    return np.ascontiguousarray(v)


def fold_to_caller_layout(values, flipped, appended):
    """The transpose of :func:`to_prepared_layout`: what was scattered onto the prepared cube f64[..., D, LA, LO'] brought
    back to the caller's layout.  An appended closing longitude column holds what belongs to column 0: it is added onto
    column 0 (``col0 + closing``, one rounding) and dropped; flipped axes are flipped back."""
    v = np.asarray(values, dtype=np.float64)
    if appended:
        closing = v[..., -1]
        v = v[..., :-1].copy()
        v[..., 0] = v[..., 0] + closing
    for ax, f in zip((-3, -2, -1), flipped):
        if f:
            v = np.flip(v, axis=ax)
    return np.ascontiguousarray(v)


class GridOperator(_Released):
    """The import of a regular grid onto fixed points, kept: ``ids`` int64[N, 8] and ``w`` f64[N, 8] on the device
    (``mm_grid_operator``, where the arithmetic is stated), built on first use.  The ids index the PREPARED cube of
    ``prepared_shape`` (:func:`prepare_regular_grid`); ``flipped`` (depth, latitude, longitude) and ``appended`` (a closing
    longitude column) record what was done to the caller's axes, and every method takes and returns the caller's layout
    ``grid_shape``.  ``noutside``: the points outside the grid (``outside="fill"``; their rows are all zero), known once
    the operator or a chunked transpose has run.  ``lead``: the leading shape of the points ([E, P] of a GLL mesh)."""

    def __init__(self, ctx, points, coords, prepared_axes, periodic, flipped, appended, clamp):
        # the points are BORROWED: a view that keeps the array alive and never frees it (it may be the caller's own
        # DeviceArray), as Source keeps its mesh
        self.ctx, self.points = ctx, points.reshape(*points.shape)
        self.lead = tuple(points.shape[:-1])
        self.npoints = points.size // 3
        self.coords = coords
        self.depth, self.lat, self.lon = prepared_axes
        self.periodic, self.flipped, self.appended, self.clamp = bool(periodic), tuple(flipped), bool(appended), bool(clamp)
        self.grid_shape = tuple(len(coords[d]) for d in DIMS)
        self.prepared_shape = (len(self.depth), len(self.lat), len(self.lon))
        self.nsrc = int(np.prod(self.prepared_shape, dtype=np.int64))
        self.ids = self.w = self.noutside = None
        self._transposed = self._outside_rows = None

    # ---- the operator itself ----------------------------------------------------------------
    def _rows(self, start, stop):
        """(ids, w, noutside) of the points [start, stop)"""
        pts = self.points.reshape(self.npoints, 3).rows(start, stop)
        return self.ctx.grid_operator(pts, self.depth, self.lat, self.lon, clamp=self.clamp, lon_periodic=self.periodic)

    def build(self):
        """Make the whole operator resident (128 B per point); the methods that need it call this."""
        if self.points is None:
            raise ValueError("the operator has been freed")
        if self.ids is None:
            self.ids, self.w, self.noutside = self._rows(0, self.npoints)
        return self

    def _cube(self, values, what):
        """f64[C, *grid_shape] of an array f64[C, D, LA, LO] or [D, LA, LO] in the caller's layout"""
        v = np.asarray(values, dtype=np.float64)
        v = v[None] if v.ndim == 3 else v
        if v.ndim != 4 or v.shape[1:] != self.grid_shape:
            raise ValueError(f"{what} must be [C, {', '.join(map(str, self.grid_shape))}] (or one component), got {v.shape}")
        return v

    def apply(self, grid_or_values, parameters=None, fill_value=np.nan):
        """Import a cube through the kept operator, without a new search: ``mm_gather`` of the prepared cube through
        ``(ids, w)`` -> f64[C, *lead] (NumPy).  ``grid_or_values``: a :class:`RegularGrid` over the operator's axes
        (``parameters``: names, None = all) or an array f64[C, D, LA, LO] / [D, LA, LO] in the caller's layout.  Points
        outside the grid get ``fill_value`` (``outside="clamp"``: there are none).

        The result is the sum ``sum_c w_c * g[id_c]`` in NumPy's order for eight terms.  It is NOT bit-equal to
        :func:`import_regular_grid`, which nests seven lerps: for finite corners the two differ by at most
        ``32 * eps * max|corner|`` (ten roundings through the three lerp levels, seven through the weights, the products
        and the 8-term sum)."""
        if isinstance(grid_or_values, RegularGrid):
            for d in DIMS:
                if not np.array_equal(grid_or_values.coords[d], self.coords[d]):
                    raise ValueError(f"the grid's {d} axis is not the one this operator was built on")
            names = list(grid_or_values.data_vars) if parameters is None else mio.pick_parameters(parameters)
            unknown = [p for p in names if p not in grid_or_values.data_vars]
            if unknown:
                raise ValueError(f"parameters {unknown} are not in the grid (it holds {list(grid_or_values.data_vars)})")
            grid_or_values = np.stack([grid_or_values.data_vars[p] for p in names]) if names else np.zeros((0,) + self.grid_shape)
        cube = to_prepared_layout(self._cube(grid_or_values, "values"), self.flipped, self.appended)
        self.build()
        ncomp = cube.shape[0]
        out = self.ctx.gather(cube.reshape(ncomp, self.nsrc), self.ids, self.w, point_major=False).numpy()
        if not self.clamp and self.noutside:
            if self._outside_rows is None:     # a row inside the grid sums to 1 within rounding, one outside is all zero
                ones = np.ones((1, self.nsrc))
                self._outside_rows = self.ctx.gather(ones, self.ids, self.w, point_major=False).numpy()[0] == 0.0
            out[:, self._outside_rows] = fill_value
        return out.reshape((ncomp,) + self.lead)

    # ---- its transpose ------------------------------------------------------------------------
    def _values(self, values):
        """f64[C, N] of f64[C, N], [C, *lead], [N] or [*lead], on the host or on the device"""
        if not hasattr(values, "data_ptr"):
            values = np.asarray(values, dtype=np.float64)
        shape = tuple(values.shape)
        if shape in ((self.npoints,), self.lead):
            shape = (1,) + shape
        if shape[1:] not in ((self.npoints,), self.lead):
            raise ValueError(f"values must be [C, {self.npoints}] or [C, {', '.join(map(str, self.lead))}], got {tuple(values.shape)}")
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):
            return np.ascontiguousarray(values, dtype=np.float64).reshape(shape[0], self.npoints)
        return self.ctx.asdevice(values, np.float64).reshape(shape[0], self.npoints)

    def transpose(self, values, chunk_points=None, prepared=False):
        """``G^T values``: values f64[C, N] or f64[C, *lead] (one component without its leading axis) at the points ->
        f64[C, D, LA, LO] (NumPy) on the grid, deterministically.  On the prepared cube the result is bit for bit
        ``np.add.at(zeros, ids, w * v[:, None])`` per component (``mm_transpose_create_nodes`` once per operator, kept;
        then ``mm_transpose_apply``); ``prepared=True`` returns that, of ``prepared_shape``.  Otherwise it is brought back
        to the caller's layout by :func:`fold_to_caller_layout`: an appended closing longitude column is added onto
        column 0 and dropped, flipped axes are flipped back.  A grid that itself holds both ends of a global axis
        (``-180 ... 180``) keeps each column's own sum -- the exact transpose of what the import reads, which takes a point
        at the seam from the two columns by its weights; add the two columns for the sum over the meridian.

        The grouping needs ``8 N < 2^31``.  Beyond that, or when ``chunk_points`` is given, consecutive chunks of that many
        points are transposed on their own -- ids and weights of the chunk built, grouped, applied, freed, so that the
        operator is never resident whole -- and added on the host in ascending chunk order, ``((c0 + c1) + c2) + ...``:
        that sum of per-chunk ``np.add.at`` results is then the stated result."""
        v = self._values(values)
        ncomp = v.shape[0]
        if self.points is None:
            raise ValueError("the operator has been freed")
        if chunk_points is None and 8 * self.npoints >= TRANSPOSE_MAX_ENTRIES:
            chunk_points = TRANSPOSE_MAX_ENTRIES // 8 - 1
        if self.npoints == 0:
            total, self.noutside = np.zeros((ncomp, self.nsrc)), 0
        elif chunk_points is None:
            if self._transposed is None:
                self.build()
                self._transposed = self.ctx.transpose_nodes(self.ids, self.w, self.nsrc)
            total = self._transposed.apply(v, point_major=False).numpy()
        else:
            chunk_points = int(chunk_points)
            if not 1 <= chunk_points <= TRANSPOSE_MAX_ENTRIES // 8 - 1:
                raise ValueError(f"chunk_points must be in 1 .. {TRANSPOSE_MAX_ENTRIES // 8 - 1}")
            total, noutside = np.zeros((ncomp, self.nsrc)), 0
            for k, start in enumerate(range(0, self.npoints, chunk_points)):
                stop = min(start + chunk_points, self.npoints)
                ids, w, miss = self._rows(start, stop)
                noutside += miss
                part = np.empty((ncomp, self.nsrc))
                with self.ctx.transpose_nodes(ids, w, self.nsrc) as op:
                    for c in range(ncomp):                   # (a row's columns start .. stop are contiguous)
                        vc = v[c, start:stop] if isinstance(v, np.ndarray) else v.rows(c, c + 1).reshape(self.npoints).rows(start, stop)
                        part[c] = op.apply(vc, point_major=False).numpy()[0]
                ids.free()
                w.free()
                total = part if k == 0 else total + part
            self.noutside = noutside
        total = total.reshape((ncomp,) + self.prepared_shape)
        return total if prepared else fold_to_caller_layout(total, self.flipped, self.appended)

    def coverage(self, chunk_points=None):
        """``G^T 1`` f64[D, LA, LO]: how much of the mesh's points every grid node carries (0: the node is not read by the
        import)."""
        return self.transpose(np.ones((1, self.npoints)), chunk_points=chunk_points)[0]

    def free(self):
        """Frees what the operator built (ids, weights, the grouped transpose) and lets go of the points, which it only
        borrowed."""
        for name in ("_transposed", "ids", "w"):
            x = getattr(self, name, None)
            if x is not None:
                x.free()
            setattr(self, name, None)
        self.points = None


def _operator_grid(grid, outside, lon_periodic):
    """(grid, prepared axes, periodic, flipped, appended, clamp) of the grid argument of the operator drivers"""
    if outside == "keep":
        raise ValueError('outside="keep" keeps values of the mesh, which an operator does not have: use "fill" (rows of '
                         'points outside are zero) or "clamp"')
    if outside not in ("fill", "clamp"):
        raise ValueError(f'outside must be "fill" or "clamp", got {outside!r}')
    if not isinstance(grid, RegularGrid):
        grid = RegularGrid.from_netcdf(grid)
    if lon_periodic is None and grid.data_vars:
        # the detection import_regular_grid makes for this grid, from the two end columns of its variables alone
        ends = np.stack([np.stack([np.asarray(v, dtype=np.float64)[..., 0], np.asarray(v, dtype=np.float64)[..., -1]], axis=-1)
                         for v in grid.data_vars.values()])
        lon_periodic = _is_global_longitude(_ascending_axis("longitude", grid.coords["longitude"])[0], ends)
    depth, lat, lon, _, _, periodic = prepare_regular_grid(grid, [], lon_periodic)
    flipped = tuple(_ascending_axis(d, grid.coords[d])[1] for d in DIMS)
    appended = len(lon) == len(grid.coords["longitude"]) + 1
    return grid, (depth, lat, lon), periodic, flipped, appended, outside == "clamp"


def grid_import_operator(grid, mesh_or_points, outside="fill", lon_periodic=None, make_spherical=False, context=None):
    """The import of ``grid`` onto a mesh as a :class:`GridOperator`, to be applied to any number of cubes
    (``.apply``) and turned round (``.transpose``, ``.coverage``).

    ``grid``: a :class:`RegularGrid` or the path of a netCDF file; only its axes matter, prepared as
    :func:`prepare_regular_grid` prepares them.  ``lon_periodic=None`` detects a global longitude axis as
    :func:`import_regular_grid` detects it for the same grid with all its variables, so that this ``G`` is that import's:
    an axis that spans exactly 360 degrees wraps when the first and the last column of every variable agree; a grid
    without variables has no columns to differ, and such an axis then wraps.  ``mesh_or_points``: a
    :class:`GllMesh`, a :class:`HexMesh`, or points f64[..., 3] on the host or on the device (a device array is
    borrowed: it must stay alive and unchanged while the operator is used, and freeing the operator leaves it alone).
    ``outside``: "fill" (a
    point outside the grid gets an all-zero row: it imports nothing and sends nothing back) or "clamp" (the edge
    extends); "keep" is refused, an operator has no values to keep.  ``make_spherical`` evaluates the coordinates on a
    copy of the mesh mapped onto its 1-D sphere, as :func:`import_regular_grid` does."""
    grid, axes, periodic, flipped, appended, clamp = _operator_grid(grid, outside, lon_periodic)
    ctx = context or default_context()
    if is_mesh(mesh_or_points):
        pts = points_of(mesh_or_points)
        _need_3d(pts, "grid_import_operator")
        points = _sphere_mapped(mesh_or_points, ctx) if make_spherical else ctx.to_device(pts, np.float64)
        points = points.reshape(*pts.shape)
    else:
        if make_spherical:
            raise ValueError("make_spherical needs a mesh with z_node_1D, not bare points")
        points, _ = ctx._points3(mesh_or_points)
    return GridOperator(ctx, points, dict(grid.coords), axes, periodic, flipped, appended, clamp)


def regular_grid_adjoint(grid, mesh, parameters, mass=True, normalise=False, outside="fill", lon_periodic=None,
                         make_spherical=False, context=None):
    """Sensitivities on a mesh brought back to the grid the model was imported from: with ``G`` the import operator of
    ``grid`` onto ``mesh`` (:func:`grid_import_operator`) and ``K`` the mesh's fields ``parameters``, the returned
    :class:`RegularGrid` holds ``G^T (M * K)`` per parameter -- the chain rule of a misfit through
    :func:`import_regular_grid`, ``M`` being the diagonal mass (:func:`gll_mass_matrix` of a :class:`GllMesh` or a
    readable Salvus model, :func:`hex8_mass_matrix` of a :class:`HexMesh`, of the mesh's own geometry) and the product
    formed on the device.  ``mass=False``: ``G^T K``.  ``normalise=True`` divides every grid node by the ``"volume"``
    below (``mm_divide_rows``): the volume-weighted mean of ``K`` over the node's hat function, 0 where that volume is 0.

    The grid also carries ``"volume"`` = ``G^T (M * 1)`` (with ``mass=False``: ``G^T 1``, the coverage) and ``nmissing``,
    the nodes of the mesh outside the grid, which send nothing back.  ``grid``, ``outside``, ``lon_periodic`` and
    ``make_spherical`` as :func:`grid_import_operator` -- a global longitude axis is detected from the grid's own
    variables as :func:`import_regular_grid` detects it, so pass the grid the model was imported from (a grid without
    variables: an axis spanning exactly 360 degrees wraps).  The mesh must be 3-D; the sum over the grid of a parameter equals ``sum(M * K)`` over
    the nodes inside it."""
    grid, axes, periodic, flipped, appended, clamp = _operator_grid(grid, outside, lon_periodic)
    parameters = mio.pick_parameters(parameters)
    if "volume" in parameters:
        raise ValueError('a parameter called "volume" clashes with the volume variable of the result')
    if not is_mesh(mesh):
        mesh = _as_gll_mesh(mesh, parameters, make_spherical)              # (a file is read once, here)
    own = points_of(mesh)
    _need_3d(own, "regular_grid_adjoint")
    fields = named_fields(mesh, parameters)[1]
    ctx = context or default_context()
    points = ctx.asdevice(_sphere_mapped(mesh, ctx) if make_spherical else own, np.float64)
    if mass:
        weight = _hex8_mass(mesh, ctx) if isinstance(mesh, HexMesh) else _device_mass(own, int(mesh.shape_order), ctx)
    ncomp = len(parameters)
    n = points.size // 3
    # rows: K per parameter, then 1 -- each multiplied by the mass on the device (mm_pcg_combine with tau = 0 is the plain
    # product mass[i] * row[i], one rounding; M * 1.0 is M)
    values = ctx.to_device(np.concatenate([np.asarray(fields, dtype=np.float64).reshape(ncomp, n), np.ones((1, n))]))
    if mass and n:
        values = ctx.multiply_rows(weight, values)
    with GridOperator(ctx, points.reshape(n, 3), dict(grid.coords), axes, periodic, flipped, appended, clamp) as op:
        back = op.transpose(values)
        nmissing = op.noutside
    volume = back[ncomp]
    data = back[:ncomp]
    if normalise and ncomp:
        data = ctx.divide_rows(data, volume).numpy()
        data[:, volume == 0.0] = 0.0
    out = RegularGrid(grid.coords["depth"], grid.coords["latitude"], grid.coords["longitude"],
                      dict({p: data[c] for c, p in enumerate(parameters)}, volume=volume), nmissing)
    out.attrs = dict(grid.attrs)
    return out
