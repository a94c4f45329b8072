"""Earth meshes onto their 1-D sphere (make_spherical) without a GPU: the NumPy restatement of the reference's
map_to_sphere against the fixture the reference itself produced, the argument checks of the new C entry points,
the synthetic Earth chunks, and -- with the CPU oracle's GLL path -- the thresholds the GPU tests
(tests/test_sphere_gpu.py) hold the drivers to."""
import ctypes as C

import numpy as np
import pytest

from multimesh_amd import helpers, synth
from oracle import oracle as O

R_EARTH = 6371000.0

# ---- thresholds fixed here with the oracle (order-2 chunks below) and asserted on the GPU ------------------------
#: |value - own 1-D value| after gll_2_gll_layered_multi_two(make_spherical=True) (oracle: 1.8e-7)
WHY_SPHERICAL_MAX = 1e-6
#: the same without the mapping is at least this many times larger (oracle: 7.4e3)
WHY_RATIO_MIN = 100.0
#: map_to_ellipse of a spherical chunk onto an elliptic one (ellipticity only / with topography), metres
#: (oracle: 0.036 m / 142.6 m -- the coarse base resolves the topography pattern only roughly)
ELLIPSE_ELLIPTICITY_MAX_M = 0.05
ELLIPSE_TOPOGRAPHY_MAX_M = 150.0
#: the same from an order-1 (hex8) base of 12 x 12 elements (oracle: 1.8 m; a coarser one's chords miss the sphere)
ELLIPSE_HEX8_MAX_M = 2.5
#: a spherical chunk stretched onto a spherical base comes back within this many ulp of R (oracle: 7)
ELLIPSE_IDENTITY_ULP = 8
#: the device's map_to_ellipse against the oracle's, in ulp of R: the chunks' centroid grids are symmetric, many
#: targets have equidistant candidates, and their order alone moves a result by up to 3 ulp (oracle)
ELLIPSE_ORACLE_ULP = 8
#: z_node_1D interpolated at the sphere-mapped nodes of another chunk (interpolate_gll_to_points; oracle: 6.1e-8)
GLL_Z_INTERP_MAX = 1e-7


def map_to_sphere_numpy(points, z_node_1d, connectivity=None, r_ref=R_EARTH):
    """Restatement of reference components/interpolator.py:1125-1144 on a copy: node layout (``connectivity``
    given) reads z_node_1D at the first occurrence of every node, else one value per point."""
    pts = np.array(points, dtype=np.float64, copy=True)
    z = np.asarray(z_node_1d, dtype=np.float64)
    if connectivity is not None:
        _, first = np.unique(connectivity, return_index=True)
        rad = z.reshape(-1)[first]
    else:
        rad = z
    x, y, zz = pts[..., 0], pts[..., 1], pts[..., 2]
    r = np.sqrt((x * x + y * y) + zz * zz)
    m = r > 0
    for c in range(3):
        v = pts[..., c]
        v[m] = ((v[m] * r_ref) * rad[m]) / r[m]
    return pts


def why_model(z, layer):
    """A model that is a function of z_node_1D with a jump at the boundary of layers 1 and 2."""
    return np.where(np.asarray(layer)[:, None] == 2, 9.0 - 3.0 * z, 4.0 + 2.0 * z)


def why_meshes():
    """Source and target: elliptic Earth chunks of different resolution and topography."""
    a = synth.earth_chunk(order=2, nlat=4, nlon=4, nrad=(2, 2), ellipticity=3.35e-3, topography=3e-4, topo_seed=1)
    b = synth.earth_chunk(order=2, nlat=5, nlon=6, nrad=(3, 3), ellipticity=3.35e-3, topography=3e-4, topo_seed=2)
    return a, b


def gll_points_meshes():
    """Source and target of the interpolate_gll_to_points checks."""
    a = synth.earth_chunk(order=2, nlat=4, nlon=4, nrad=(2, 2), ellipticity=3.35e-3, topography=3e-4, topo_seed=1)
    b = synth.earth_chunk(order=2, nlat=5, nlon=3, nrad=(3, 3), ellipticity=3.35e-3, topography=3e-4, topo_seed=2)
    return a, b


def layered_oracle(src, layer_a, fields, tgt, layer_b, order, k=30, tol=1.05):
    """The per-layer loop of gll_2_gll_layered_multi_two (reference interpolator.py:1047-1082) with the oracle."""
    out = np.zeros((fields.shape[0],) + tgt.shape[:2])
    for layer in np.unique(layer_b):
        sm, tm = layer_a == layer, layer_b == layer
        nodes = tgt[tm]
        uniq, inv = np.unique(nodes.reshape(-1, 3), return_inverse=True, axis=0)
        nn, _ = O.knn_ckdtree(src[sm].mean(axis=1), uniq, k)
        elem, co, _ = O.locate_gll(order, nn, np.ascontiguousarray(src[sm]), uniq, tolerance=tol, snap_to_nearest=True)
        vals = O.gather_elem(np.ascontiguousarray(fields[:, sm]), elem, co)
        out[:, tm] = vals[inv.reshape(-1)].reshape(nodes.shape[0], nodes.shape[1], -1).transpose(2, 0, 1)
    return out


def map_to_ellipse_oracle(base, z_base, points, z_points, order, k=25, tol=1.05, knn=O.knn_brute):
    """map_to_ellipse's intent (reference interpolator.py:1085-1122) with the oracle's GLL path, element-nodal
    base: (stretched points, number of points without an element)."""
    ratio = (np.sqrt(np.sum(base ** 2, axis=-1)) / R_EARTH) / z_base
    bs = map_to_sphere_numpy(base, z_base)
    ts = map_to_sphere_numpy(points, z_points).reshape(-1, 3)
    nn = knn(bs.mean(axis=1), ts, k)
    nn = nn[0] if isinstance(nn, tuple) else nn
    elem, co, miss = O.locate_gll(order, nn, bs, ts, tolerance=tol)
    vals = O.gather_elem(ratio[None], elem, co)[:, 0]
    return (vals[:, None] * ts).reshape(np.shape(points)), miss


# ------------------------------------------------------------------------------------------ the restatement
def test_restatement_reproduces_the_references_map_to_sphere(golden):
    g = golden("sphere_map")
    got = map_to_sphere_numpy(g["en_points"], g["en_z_node_1D"])
    assert np.array_equal(got, g["en_expected"])
    got = map_to_sphere_numpy(g["node_points"], g["node_z_node_1D"], connectivity=g["node_connectivity"])
    assert np.array_equal(got, g["node_expected"])
    # the fixture exercises what it is meant to: centre points, and copies of a node that disagree
    assert (np.linalg.norm(g["en_points"], axis=-1) == 0).sum() >= 3
    assert np.array_equal(g["en_expected"][3, 5], [0.0, 0.0, 0.0])
    conn, z = g["node_connectivity"].reshape(-1), g["node_z_node_1D"].reshape(-1)
    assert (conn == 7).sum() > 50 and len(np.unique(z[conn == 7])) > 50
    last = np.zeros(conn.max() + 1, dtype=np.int64)
    last[conn] = np.arange(conn.size)                     # (fancy assignment: the LAST occurrence wins)
    wrong = g["node_points"].copy()
    x, y, zz = wrong.T
    r = np.sqrt((x * x + y * y) + zz * zz)
    m = r > 0
    for c in range(3):
        wrong[m, c] = ((wrong[m, c] * R_EARTH) * z[last][m]) / r[m]
    assert not np.array_equal(wrong, g["node_expected"])  # the first occurrence matters


# ------------------------------------------------------------------------------------------ C ABI
def test_sphere_entry_points_reject_bad_arguments_without_a_gpu():
    lib = helpers.load_lib()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below fails its argument checks first
    buf = C.c_void_p(0x2000)
    assert lib.mm_map_to_sphere(None, buf, 4, buf, 4, None, R_EARTH, buf) == -1
    assert b"null" in lib.mm_last_error()
    assert lib.mm_map_to_sphere(fake, buf, -1, buf, 4, None, R_EARTH, buf) == -1
    assert lib.mm_map_to_sphere(fake, buf, 4, buf, -4, buf, R_EARTH, buf) == -1
    assert lib.mm_map_to_sphere(fake, buf, 4, buf, 3, None, R_EARTH, buf) == -1        # one radius per point
    assert lib.mm_map_to_sphere(fake, None, 4, buf, 4, None, R_EARTH, buf) == -1
    assert lib.mm_map_to_sphere(fake, buf, 4, None, 4, None, R_EARTH, buf) == -1
    assert lib.mm_map_to_sphere(fake, buf, 4, buf, 4, None, R_EARTH, None) == -1
    assert lib.mm_map_to_sphere(fake, C.c_void_p(0x2000), 4, buf, 4, None, R_EARTH, C.c_void_p(0x2008)) == -1
    assert b"overlaps" in lib.mm_last_error()
    assert lib.mm_first_occurrence(None, buf, 8, 4, buf) == -1
    assert lib.mm_first_occurrence(fake, buf, -8, 4, buf) == -1
    assert lib.mm_first_occurrence(fake, buf, 8, -4, buf) == -1
    assert lib.mm_first_occurrence(fake, None, 8, 4, buf) == -1
    assert lib.mm_first_occurrence(fake, buf, 8, 4, None) == -1
    assert lib.mm_sphere_ratio(None, buf, 4, buf, 4, None, R_EARTH, buf) == -1
    assert lib.mm_sphere_ratio(fake, buf, -4, buf, 4, None, R_EARTH, buf) == -1
    assert lib.mm_sphere_ratio(fake, buf, 4, buf, 4, None, R_EARTH, None) == -1
    assert lib.mm_scale_points(None, buf, 4, buf, buf) == -1
    assert lib.mm_scale_points(fake, buf, -4, buf, buf) == -1
    assert lib.mm_scale_points(fake, buf, 4, None, buf) == -1
    assert lib.mm_scale_points(fake, C.c_void_p(0x2000), 4, buf, C.c_void_p(0x2010)) == -1
    # nothing to do is not an error
    assert lib.mm_map_to_sphere(fake, None, 0, None, 0, None, R_EARTH, None) == 0
    assert lib.mm_scale_points(fake, None, 0, None, None) == 0


# ------------------------------------------------------------------------------------------ synthetic Earth chunks
def test_earth_chunk_layout_fields_and_deformation():
    sph = synth.earth_chunk(order=2, nlat=3, nlon=4, nrad=(2, 3), fluid_layers=(1,))
    E = 3 * 4 * 5
    assert sph["points"].shape == (E, 27, 3) and sph["z_node_1D"].shape == (E, 27)
    assert np.array_equal(np.unique(sph["layer"]), [1.0, 2.0]) and (sph["layer"] == 1).sum() == 3 * 4 * 2
    assert np.array_equal(sph["fluid"], (sph["layer"] == 1) * 1.0)
    r = np.linalg.norm(sph["points"], axis=-1)
    assert np.abs(r / R_EARTH - sph["z_node_1D"]).max() < 4e-16          # z_node_1D = r / R at every node
    # copies of a node are bit-identical (one unique row per grid node)
    assert len(np.unique(sph["points"].reshape(-1, 3), axis=0)) == (2 * 3 + 1) * (2 * 4 + 1) * (2 * 5 + 1)
    ell = synth.earth_chunk(order=2, nlat=3, nlon=4, nrad=(2, 3), ellipticity=3.35e-3, topography=3e-4, topo_seed=4)
    assert np.array_equal(ell["z_node_1D"], sph["z_node_1D"])             # the deformation leaves z_node_1D alone
    assert len(np.unique(ell["points"].reshape(-1, 3), axis=0)) == len(np.unique(sph["points"].reshape(-1, 3), axis=0))
    stretch = np.linalg.norm(ell["points"], axis=-1) / r
    assert np.abs(stretch - 1).max() > 1e-3                                # ellipticity + topography at the top
    deep = sph["z_node_1D"] < 6_000_000 / R_EARTH
    other = synth.earth_chunk(order=2, nlat=3, nlon=4, nrad=(2, 3), ellipticity=3.35e-3, topography=3e-4, topo_seed=5)
    # topography tapers to zero at depth: below the taper two topographies agree, at the surface they do not
    assert np.array_equal(other["points"][deep], ell["points"][deep])
    assert np.abs(other["points"] - ell["points"]).max() > 100.0
    # mapping the deformed chunk to the sphere gives the spherical one back (to rounding)
    back = map_to_sphere_numpy(ell["points"], ell["z_node_1D"])
    assert np.abs(back - sph["points"]).max() <= 4 * np.spacing(R_EARTH)


# ------------------------------------------------------------------------------------------ thresholds (oracle)
def test_why_spherical_mapping_matters_on_the_oracle():
    a, b = why_meshes()
    fa = why_model(a["z_node_1D"], a["layer"])[None]
    want = why_model(b["z_node_1D"], b["layer"])
    sa, sb = map_to_sphere_numpy(a["points"], a["z_node_1D"]), map_to_sphere_numpy(b["points"], b["z_node_1D"])
    err_sph = np.abs(layered_oracle(sa, a["layer"], fa, sb, b["layer"], 2)[0] - want).max()
    err_ell = np.abs(layered_oracle(a["points"], a["layer"], fa, b["points"], b["layer"], 2)[0] - want).max()
    assert err_sph < WHY_SPHERICAL_MAX
    assert err_ell > WHY_RATIO_MIN * err_sph and err_ell > WHY_RATIO_MIN * WHY_SPHERICAL_MAX


def test_map_to_ellipse_thresholds_on_the_oracle():
    b0 = synth.earth_chunk(order=2, nlat=5, nlon=6, nrad=(3, 3))
    for kw, limit in ((dict(ellipticity=3.35e-3), ELLIPSE_ELLIPTICITY_MAX_M),
                      (dict(ellipticity=3.35e-3, topography=3e-4, topo_seed=1), ELLIPSE_TOPOGRAPHY_MAX_M)):
        a = synth.earth_chunk(order=2, nlat=4, nlon=4, nrad=(2, 2), **kw)
        want = synth.earth_chunk(order=2, nlat=5, nlon=6, nrad=(3, 3), **kw)["points"]
        got, miss = map_to_ellipse_oracle(a["points"], a["z_node_1D"], b0["points"], b0["z_node_1D"], 2)
        assert miss == 0 and np.abs(got - want).max() < limit
        other, _ = map_to_ellipse_oracle(a["points"], a["z_node_1D"], b0["points"], b0["z_node_1D"], 2,
                                         knn=O.knn_ckdtree)                  # equidistant candidates in another order
        assert np.abs(other - got).max() <= ELLIPSE_ORACLE_ULP * np.spacing(R_EARTH)
    a1 = synth.earth_chunk(order=1, nlat=12, nlon=12, nrad=(2, 2), ellipticity=3.35e-3)
    b1 = synth.earth_chunk(order=1, nlat=5, nlon=5, nrad=(3, 3))
    want = synth.earth_chunk(order=1, nlat=5, nlon=5, nrad=(3, 3), ellipticity=3.35e-3)["points"]
    got, miss = map_to_ellipse_oracle(a1["points"], a1["z_node_1D"], b1["points"], b1["z_node_1D"], 1)
    assert miss == 0 and np.abs(got - want).max() < ELLIPSE_HEX8_MAX_M
    a0 = synth.earth_chunk(order=2, nlat=4, nlon=4, nrad=(2, 2))
    got, miss = map_to_ellipse_oracle(a0["points"], a0["z_node_1D"], b0["points"], b0["z_node_1D"], 2)
    assert miss == 0 and np.abs(got - b0["points"]).max() <= ELLIPSE_IDENTITY_ULP * np.spacing(R_EARTH)
    outside = synth.earth_chunk(order=2, nlat=5, nlon=6, nrad=(3, 3), lat=(-12.0, 8.0))
    _, miss = map_to_ellipse_oracle(a0["points"], a0["z_node_1D"], outside["points"], outside["z_node_1D"], 2)
    assert miss > 0


def test_gll_z_interpolation_threshold_on_the_oracle():
    a, b = gll_points_meshes()
    sa = map_to_sphere_numpy(a["points"], a["z_node_1D"])
    pts = map_to_sphere_numpy(b["points"], b["z_node_1D"]).reshape(-1, 3)
    nn = O.knn_brute(sa.mean(axis=1), pts, 25)
    elem, co, miss = O.locate_gll(2, nn, sa, pts, tolerance=1.05)
    z = O.gather_elem(a["z_node_1D"][None], elem, co)[:, 0]
    assert miss == 0 and np.abs(z - b["z_node_1D"].reshape(-1)).max() < GLL_Z_INTERP_MAX
