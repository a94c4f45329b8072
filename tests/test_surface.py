"""The surface distance without a GPU: the extension header against the module's signature table, the argument checks of the
Python layer and of the two entry points, and the NumPy statement (tests/surface_cases.py) against an independent
formulation, in exact cases and against the node distance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import boundary_cases as BC
import surface_cases as SC
from multimesh_amd import helpers, surface, synth
from multimesh_amd.api import GllMesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multimesh_surface.h")
SYMBOLS = ("mm_boundary_triangles", "mm_surface_distance")

# The statement and the independent formulation round differently.  Over the seeded cases below -- 400 triangles of size
# about 1 and aspect <= 10 at the origin, 50 points each within three triangle sizes -- the largest difference measured on
# the CPU is 8.882e-16 (one unit in the last place of a distance between 4 and 8; printed by the test); times 4:
SLACK = 4 * 8.882e-16


# ------------------------------------------------------------------------------------------- the header and the table
_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}


def _declared_prototypes():
    """name -> (restype, [argtypes]) of the header's declarations, a pointer of any kind being c_void_p"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    code = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    protos = {}
    for ret, name, params in re.findall(r"(\w[\w\s\*]*?)\b(mm_\w+)\s*\(([^()]*)\)\s*;", code):
        def kind(decl, has_name):
            if "*" in decl:
                return C.c_void_p
            words = [w for w in decl.split() if w != "const"]
            return _SCALARS[" ".join(words[:-1] if has_name else words)]
        protos[name] = (kind(ret, False), [kind(p, True) for p in params.split(",")])
    return protos


def test_the_extension_header_and_the_table_agree():
    protos = _declared_prototypes()
    assert list(protos) == list(surface.SIGNATURES) == list(SYMBOLS)
    lib = surface.bind()
    assert lib is helpers.load_lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = surface.SIGNATURES[name]
        assert (restype, list(argtypes)) == (ret, params), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert name not in helpers.SIGNATURES and name not in helpers.EXPORTED_SYMBOLS


# --------------------------------------------------------------------------------------------------- argument checks
def test_the_python_layer_checks_its_arguments():
    assert surface._cutoff(None) == np.inf and surface._cutoff(np.inf) == np.inf and surface._cutoff(2) == 2.0
    for cutoff in (0.0, -1.0, np.nan, -np.inf):
        with pytest.raises(ValueError, match="cutoff must be positive"):
            surface._cutoff(cutoff)
    gp = synth.gll_mesh(2, 1)
    mesh = GllMesh(gp, 1, {"K": np.ascontiguousarray(gp[..., 0])})
    for call in (lambda: surface.boundary_triangles(None), lambda: surface.distance_to_surface(gp, "boundary"),
                 lambda: surface.taper_to_surface(mesh, "K", 0.1, 0.2, boundary=3)):
        with pytest.raises(ValueError, match="boundary must come from mesh_boundary"):
            call()
    with pytest.raises(ValueError, match="radii"):
        surface.taper_to_surface(mesh, "K", 0.3, 0.2)
    with pytest.raises(ValueError, match="sides are named"):
        surface.taper_to_surface(mesh, "K", 0.1, 0.2, sides=("left",))
    assert sorted(surface.__all__) == sorted(["boundary_triangles", "distance_to_triangles", "distance_to_surface",
                                              "depth_below_surface", "taper_to_surface", "blend_models"])


def test_the_entry_points_refuse_on_the_host_before_the_device_is_touched():
    lib = surface.bind()
    ctx, buf = C.c_void_p(0x1000), C.c_void_p(0x100000)        # dummies: a refused call looks at neither
    tri, dist = lib.mm_boundary_triangles, lib.mm_surface_distance
    assert tri(None, buf, 1, 1, buf, buf, 1, 7, buf) == -1 and b"ctx" in lib.mm_last_error()
    for order in (0, 3, 5):
        assert tri(ctx, buf, 1, order, buf, buf, 1, 7, buf) == -1 and b"order" in lib.mm_last_error()
    assert tri(ctx, buf, 1, 1, buf, buf, 1, 8, buf) == -1 and b"side_mask" in lib.mm_last_error()
    assert tri(ctx, buf, 1, 1, buf, buf, 7, 7, buf) == -1 and b"nb" in lib.mm_last_error()
    assert tri(ctx, buf, -1, 1, buf, buf, 0, 7, buf) == -1 and b"nelem" in lib.mm_last_error()
    assert tri(ctx, buf, 1, 1, buf, buf, 1, 7, None) == -1 and b"null" in lib.mm_last_error()
    assert dist(None, buf, 1, buf, 1, 1.0, buf) == -1 and b"ctx" in lib.mm_last_error()
    for cutoff in (0.0, -1.0, float("nan"), -float("inf"), 1e-200):
        assert dist(ctx, buf, 1, buf, 1, cutoff, buf) == -1 and b"cutoff" in lib.mm_last_error()
    assert dist(ctx, buf, -1, buf, 1, 1.0, buf) == -1
    assert dist(ctx, buf, 1, buf, -1, 1.0, buf) == -1
    assert dist(ctx, buf, 1, buf, 1 << 30, 1.0, buf) == -1 and b"T must lie" in lib.mm_last_error()
    assert dist(ctx, buf, 1, None, 1, 1.0, buf) == -1 and b"null triangles" in lib.mm_last_error()
    assert dist(ctx, None, 1, buf, 1, 1.0, buf) == -1 and dist(ctx, buf, 1, buf, 1, 1.0, None) == -1


# ------------------------------------------------------------------------------- the statement against another formulation
def _independent(p, a, b, c):
    """The least of: the distance to the plane where the projection falls inside the triangle, the three segment distances,
    the three vertex distances -- no regions, float64 throughout"""
    def norm(u):
        return np.sqrt((u * u).sum(axis=-1))

    def segment(p, s, t):
        st = t - s
        u = np.clip(((p - s) * st).sum(axis=-1) / (st * st).sum(axis=-1), 0.0, 1.0)
        return norm(p - (s + u[..., None] * st))

    nrm = np.cross(b - a, c - a)
    height = ((p - a) * nrm).sum(axis=-1) / norm(nrm)
    foot = p - (height / norm(nrm))[..., None] * nrm
    inside = np.ones(height.shape, bool)
    for s, t in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(t - s, foot - s) * nrm).sum(axis=-1) >= 0.0
    best = np.where(inside, np.abs(height), np.inf)
    for s, t in ((a, b), (b, c), (c, a)):
        best = np.minimum(best, segment(p, s, t))
    for s in (a, b, c):
        best = np.minimum(best, norm(p - s))
    return best


def _seeded_cases():
    rng = np.random.default_rng(2024)
    ntri, npts = 400, 50
    a = rng.uniform(-0.5, 0.5, (ntri, 3))
    u = rng.normal(size=(ntri, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(ntri, 3)))
    w /= np.linalg.norm(w, axis=1)[:, None]
    base = rng.uniform(0.5, 1.5, ntri)
    height = base / rng.uniform(1.0, 10.0, ntri)              # aspect <= 10
    b = a + base[:, None] * u
    c = a + (rng.uniform(0.0, 1.0, ntri) * base)[:, None] * u + height[:, None] * w
    p = a[:, None, :] + rng.uniform(-3.0, 3.0, (ntri, npts, 3)) * base[:, None, None]
    return p, a[:, None, :], b[:, None, :], c[:, None, :]


def test_the_statement_agrees_with_an_independent_formulation():
    p, a, b, c = _seeded_cases()
    r = SC.triangle_distance(p, a, b, c)
    other = _independent(p, *np.broadcast_arrays(a, b, c, p)[:3])
    worst = float(np.abs(r - other).max())
    print(f"largest |statement - independent| over {r.size} cases: {worst:.3e} (SLACK {SLACK:.3e})")
    assert np.isfinite(r).all() and 0.0 < worst <= SLACK and r.max() > 3.0 and r.min() < 0.05


# ------------------------------------------------------------------------------------------------------- exact cases
def test_exact_cases():
    a, b, c = np.array([1.0, 2.0, 0.5]), np.array([3.0, 2.0, 0.5]), np.array([1.0, 6.0, 0.5])   # flat, z = 0.5
    for vertex in (a, b, c):
        r = SC.triangle_distance(vertex, a, b, c)
        assert r == 0.0 and not np.signbit(r)                                        # exactly +0.0
        assert SC.same_bits(SC.closest(vertex, a, b, c), vertex)
    for x, y, h in ((1.5, 2.5, 0.25), (1.25, 3.0, -2.0), (2.0, 2.5, 1024.0)):        # above and below the interior
        assert SC.triangle_distance(np.array([x, y, 0.5 + h]), a, b, c) == abs(h)
    assert SC.triangle_distance(np.array([2.0, 0.0, 0.5]), a, b, c) == 2.0           # off the edge ab
    assert SC.triangle_distance(np.array([-2.0, -2.0, 0.5]), a, b, c) == 5.0         # off the vertex a: 3, 4, 5
    assert SC.triangle_distance(np.array([2.0, 2.0, 0.5]), a, b, c) == 0.0           # on the edge ab
    # a degenerate triangle gives a NaN off its doubled vertex's region, which the minimum skips; a NaN point keeps the cutoff
    tri = np.array([[a, a, c], [a, b, c]])
    with np.errstate(all="ignore"):
        assert np.isnan(SC.triangle_distance(np.array([1.0, 4.0, 1.5]), a, a, c))
    d, count = SC.surface_distance(np.array([[1.0, 4.0, 1.5], [np.nan, 0.0, 0.0], [1.5, 2.5, 100.0]]), tri, 8.0)
    assert d.tolist() == [1.0, 8.0, 8.0] and count == 1
    d, count = SC.surface_distance(np.zeros((3, 3)), np.zeros((0, 3, 3)), np.inf)
    assert (d == np.inf).all() and count == 0
    # the set of triangles defines the result: any order, any repetition
    rng = np.random.default_rng(3)
    tris, pts = rng.normal(size=(40, 3, 3)), rng.normal(size=(100, 3))
    ref = SC.surface_distance(pts, tris, 0.7)[0]
    assert SC.same_bits(SC.surface_distance(pts, np.concatenate([tris[::-1], tris[:7]]), 0.7)[0], ref)


def test_boundary_triangles_of_the_statement():
    gp = synth.gll_mesh(3, 2)
    corners = gp[:, BC.corner_nodes(2)]
    faces, _ = BC.boundary_faces(BC.corner_ids(corners)[0])
    side = BC.classify(corners, faces, up=(0.0, 0.0, 1.0))
    tri = SC.boundary_triangles(gp, 2, faces, side, 0b101)
    assert tri.shape == (8 * int((side != 1).sum()), 3, 3) and SC.boundary_triangles(gp, 2, faces, side, 0).shape == (0, 3, 3)
    nodes = BC.boundary_nodes(gp, 2, faces, side, 0b101)
    assert {tuple(v) for v in tri.reshape(-1, 3)} == {tuple(v) for v in nodes}       # every node is a vertex, and no other
    # the two triangles of a sub-quad share its diagonal q[j][i] -- q[j+1][i+1], and the facets tile the unit cube's faces
    assert SC.same_bits(tri[0::2, 0], tri[1::2, 0]) and SC.same_bits(tri[0::2, 2], tri[1::2, 1])
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert abs(area.sum() - 5.0) < 1e-12
    assert SC.same_bits(SC.boundary_triangles(gp, 2, faces, None, 0), SC.boundary_triangles(gp, 2, faces, side, 7))


# ------------------------------------------------------------------------------------- against the distance to the nodes
@pytest.mark.parametrize("kind", ["cube", "chunk"])
def test_the_surface_is_never_farther_than_its_nodes(kind):
    if kind == "cube":
        gp, order, up = synth.gll_mesh(4, 2, seed=2), 2, (0.0, 0.0, 1.0)
    else:
        gp, order, up = synth.earth_chunk(order=2, nlat=2, nlon=2, nrad=(1, 1), topography=3e-4,
                                          ellipticity=3.35e-3)["points"], 2, None
    corners = gp[:, BC.corner_nodes(order)]
    faces, _ = BC.boundary_faces(BC.corner_ids(corners)[0])
    side = BC.classify(corners, faces, up=up)
    tri = SC.boundary_triangles(gp, order, faces, side, 0b101)
    nodes = BC.boundary_nodes(gp, order, faces, side, 0b101)
    flat = gp.reshape(-1, 3)
    pairs = np.random.default_rng(6).integers(0, len(flat), (500, 2))
    targets = np.concatenate([flat, 0.5 * (flat[pairs[:, 0]] + flat[pairs[:, 1]])])   # the nodes, and points between them
    d_surface, _ = SC.surface_distance(targets, tri, np.inf)
    d_node, _ = BC.cutoff_distance(targets, nodes, 1e300)
    scale = np.abs(gp).max()                                   # the slack was measured at coordinates and distances of about 1
    assert (d_surface <= d_node + SLACK * scale).all() and (d_surface < 0.9 * d_node).any()
    on_boundary = d_node == 0.0
    assert on_boundary.any() and (d_surface[on_boundary] == 0.0).all()
