"""Regions without a GPU: the extension header against the module's signature table, the argument errors that are decided
before the device is touched, what :class:`multimesh_amd.regions.Region` refuses and builds, the anchor it picks, and the NumPy
statement (tests/regions_cases.py) against independent methods: the inside flag against winding numbers by summed atan2
angles, the distance against the nearest of 2 000 samples per arc.  The bounding balls of the culls are built on the device, so
they have no host test here: tests/test_regions_gpu.py holds the device to the statement on nodes at the rims."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guarded_cases as G
import regions_cases as RC
from multimesh_amd import helpers
from multimesh_amd import regions as RG
from test_parametrisation import _c_class, _ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multimesh_regions.h")


# ----------------------------------------------------------------------------------------------- the header and the table
def _declared_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    code = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    protos = {}
    for statement in code.split(";"):
        m = re.fullmatch(r"\s*([^()]*?)\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^()]*)\)\s*", re.split(r"[{}]", statement)[-1])
        if m:
            ret, name, params = m.groups()
            protos[name] = (_c_class(ret, is_return=True), [_c_class(p) for p in params.split(",")])
    return protos


def test_the_extension_header_and_the_table_agree():
    protos = _declared_prototypes()
    assert list(protos) == list(RG.SIGNATURES) == ["mm_region_distance"]
    lib = RG.bind()
    assert lib is helpers.load_lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = RG.SIGNATURES[name]
        assert len(params) == len(argtypes) == 13
        assert (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes]) == (ret, params), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert name not in helpers.SIGNATURES and name not in helpers.EXPORTED_SYMBOLS
    text = open(HEADER).read()
    assert int(re.search(r"#define MM_REGION_MAX_EDGES (\d+)", text).group(1)) == RG.MAX_EDGES == 1 << 20
    assert int(re.search(r"#define MM_REGION_EDGE_CHUNK (\d+)", text).group(1)) == RG.EDGE_CHUNK == RC.CHUNK


# --------------------------------------------------------------------------------------------------- argument checks
CTX = C.c_void_p(0x1000)            # a dummy: a refused call never looks at the context
PTS, EDG, ANC, OUT, FLG = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000, 0x500000))


def _call(lib, ctx=CTX, pts=PTS, ngroups=10, P=8, edges=EDG, E=12, anchor=ANC, flag=1, cutoff=0.1, scale=6371000.0, out=OUT, flags=FLG):
    return lib.mm_region_distance(ctx, pts, ngroups, P, edges, E, anchor, flag, cutoff, scale, out, flags, None)


#: every MM_ERR_ARG case of the header that is decided before the device is touched
REFUSED = {
    "null ctx": dict(ctx=None),
    "null points": dict(pts=None),
    "null edges": dict(edges=None),
    "null anchor": dict(anchor=None),
    "both outputs null": dict(out=None, flags=None),
    "negative ngroups": dict(ngroups=-1),
    "ngroups at 2^48": dict(ngroups=1 << 48),
    "P zero": dict(P=0),
    "P above 256": dict(P=257),
    "negative E": dict(E=-1),
    "E above 2^20": dict(E=(1 << 20) + 1),
    "cutoff zero": dict(cutoff=0.0),
    "cutoff negative": dict(cutoff=-0.1),
    "cutoff above 2": dict(cutoff=2.0000001),
    "cutoff nan": dict(cutoff=float("nan")),
    "scale zero": dict(scale=0.0),
    "scale negative": dict(scale=-1.0),
    "scale inf": dict(scale=float("inf")),
    "scale nan": dict(scale=float("nan")),
    "flag two": dict(flag=2),
    "flag negative": dict(flag=-1),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refuses_without_a_gpu(what):
    lib = RG.bind()
    assert _call(lib, **REFUSED[what]) == -1, what
    message = lib.mm_last_error()
    assert b"mm_region_distance" in message and len(message) > len(b"mm_region_distance: "), message
    assert lib.mm_last_status() == -1


# ------------------------------------------------------------------------------------------------------------------ Region
def test_what_a_region_refuses():
    ring = RC.wiggly_ring(8)
    for bad, match in ((ring[:2], "3 distinct"), (np.array([ring[0], ring[1], ring[0], ring[1]]), "3 distinct"),
                       (np.where(np.arange(16).reshape(8, 2) == 5, np.nan, ring), "finite"), (ring + [80.0, 0.0], "finite"),
                       (np.array([[0.0, 0.0], [0.0, 180.0], [10.0, 90.0]]), "antipodal"),
                       (np.array([[0.0, 0.0], [0.0, 10.0], [0.0, 10.0], [10.0, 5.0]]), "equal or antipodal"),
                       (np.zeros((4, 3)), "f64\\[n, 2\\]")):
        with pytest.raises(ValueError, match=match):
            RG.Region(bad)
    with pytest.raises(ValueError, match="interior must be"):
        RG.Region(ring, interior="right")
    with pytest.raises(ValueError, match="at least one ring"):
        RG.Region([])
    closed = RG.Region(np.concatenate([ring, ring[:1]]))
    assert np.array_equal(closed.edges, RG.Region(ring).edges)


def test_too_many_edges_are_refused():
    n = RG.MAX_EDGES + 1
    lon = np.arange(n) * (360.0 / n)
    with pytest.raises(ValueError, match="at most 2\\^20 edges"):
        RG.Region(np.stack([np.full(n, 40.0), lon], axis=1))


def test_the_edge_table_is_what_the_header_states():
    reg = RG.Region(RC.ring_with_hole())
    U, V, N = reg.edges[:, 0:3], reg.edges[:, 3:6], reg.edges[:, 6:9]
    assert reg.edges.shape == (33, 9) and reg.edges.flags.c_contiguous
    assert np.abs(RC.dot(U, U) - 1.0).max() <= 2.0 ** -48 and np.abs(RC.dot(reg.anchor, reg.anchor) - 1.0) <= 2.0 ** -48
    c = RC.cross(U, V)
    assert np.array_equal(N, c / np.sqrt(RC.dot(c, c))[:, None])
    # both rows that share a vertex hold the same doubles, ring by ring
    assert np.array_equal(V[:23], U[1:24]) and np.array_equal(V[23], U[0]) and np.array_equal(V[24:32], U[25:33]) and np.array_equal(V[32], U[24])


def _inside(region, latlon):
    pts = RG.unit_vectors(np.atleast_2d(np.asarray(latlon, dtype=np.float64)))
    return RC.region_distance(pts, region.edges, region.anchor, region.anchor_inside, 2.0, 1.0)[1].tolist()


def test_a_polar_cap_given_both_ways():
    """A 10 degree cap about the north pole: "smaller" gives the cap both times, "left" the cap and its complement."""
    probes = [[89.0, 12.0], [85.0, -140.0], [75.0, 50.0], [0.0, 0.0], [-89.0, 3.0]]
    cap, rest = [1, 1, 0, 0, 0], [0, 0, 1, 1, 1]
    for clockwise in (False, True):
        assert _inside(RG.Region(RC.polar_cap(clockwise=clockwise), interior="smaller"), probes) == cap
        assert _inside(RG.Region(RC.polar_cap(clockwise=clockwise), interior="left"), probes) == (rest if clockwise else cap)
        assert _inside(RG.Region(RC.polar_cap(clockwise=clockwise), interior=(88.0, 100.0)), probes) == cap
        assert _inside(RG.Region(RC.polar_cap(clockwise=clockwise), interior=(-20.0, 100.0)), probes) == rest


def test_complement_flips_the_flag_and_keeps_the_edges():
    reg = RG.Region(RC.concave_12gon())
    other = reg.complement()
    assert other.edges is reg.edges and np.array_equal(other.anchor, reg.anchor) and other.anchor_inside == 1 - reg.anchor_inside
    pts = RC.sphere_points(2000, 3)
    a = RC.region_distance(pts, reg.edges, reg.anchor, reg.anchor_inside, 0.3, 1.0)
    b = RC.region_distance(pts, other.edges, other.anchor, other.anchor_inside, 0.3, 1.0)
    assert np.array_equal(a[0], -b[0]) and np.array_equal(a[1], 1 - b[1]) and a[3] == b[3]
    assert other.complement().anchor_inside == reg.anchor_inside


def test_a_box_across_the_antimeridian():
    box = RG.Region.from_box(-10.0, 10.0, 170.0, -170.0, step=1.0)
    assert len(box.edges) == 2 * 20 + 2 * 20
    assert _inside(box, [[0.0, 180.0], [0.0, -175.0], [9.5, 171.0], [0.0, 160.0], [11.0, 180.0], [0.0, 0.0]]) == [1, 1, 1, 0, 0, 0]
    # densified: the box follows its parallels -- a point just inside the northern side, midway, is inside (the great circle
    # through the corners would bulge north of it by 0.15 degrees and make 10.1 inside as well)
    assert _inside(box, [[9.99, 180.0], [10.01, 180.0]]) == [1, 0]
    coarse = RG.Region(np.array([[40.0, 0.0], [40.0, 60.0], [60.0, 60.0], [60.0, 0.0]]))
    assert _inside(coarse, [[42.0, 30.0]]) == [0] and _inside(coarse.densify(0.5), [[42.0, 30.0]]) == [1]
    with pytest.raises(ValueError, match="lat0 < lat1"):
        RG.Region.from_box(10.0, -10.0, 0.0, 5.0)


def test_a_circle():
    c = RG.Region.circle(40.0, 10.0, 1.0e6, n=360)
    assert len(c.edges) == 360 and c.anchor_inside == 0
    s, inside = RC.region_distance(RG.unit_vectors(np.array([[40.0, 10.0], [40.0, 30.0]])), c.edges, c.anchor, c.anchor_inside, 2.0,
                                   RC.R_EARTH)[:2]
    assert inside.tolist() == [1, 0] and abs(s[0] - RG.arc_to_chord(1.0e6)) < 50.0       # (the polygon lies inside the circle)


def test_geodetic_latitude_moves_a_vertex_at_45_degrees_by_the_known_amount():
    assert abs((45.0 - float(RG.geocentric_latitude(45.0))) - 0.1924) < 1e-4
    assert float(RG.geocentric_latitude(90.0)) == 90.0 and float(RG.geocentric_latitude(0.0)) == 0.0
    ring = np.array([[45.0, 0.0], [45.0, 20.0], [60.0, 10.0]])
    plain, geo = RG.Region(ring), RG.Region(ring, geodetic=True)
    moved = np.rad2deg(np.arcsin(geo.edges[0, 2])) - np.rad2deg(np.arcsin(plain.edges[0, 2]))
    assert abs(moved + 0.1924) < 1e-4


def test_the_anchor_keeps_its_distance_for_every_region_of_the_gpu_tests():
    regions = [RC.region_with(max(E, 3)) for E in RC.EDGE_COUNTS] + list(RC.named_regions().values())
    regions += [RG.Region.from_box(-8.0, 8.0, -8.0, 8.0), RG.Region.circle(0.0, 0.0, 5.0e5)]
    generic = RG.unit_vectors(np.array(RG.ANCHOR_CANDIDATES))
    assert (np.abs(generic) > 0.05).all()                       # no pole, no coordinate plane
    for reg in regions:
        d = -RC.region_distance(reg.anchor[None], reg.edges, reg.anchor, 0, 2.0, 1.0)[0][0]
        assert d == reg.anchor_distance >= RG.MIN_ANCHOR_CHORD
        assert any(np.array_equal(reg.anchor, g) for g in generic)
    for case in RC.guarded_cases():
        d = -RC.region_distance(case["anchor"][None], case["edges"], case["anchor"], 0, 2.0, 1.0)[0][0]
        assert d >= RG.MIN_ANCHOR_CHORD


def test_the_statement_in_blocks_and_the_modules_statement_are_the_headers_loop():
    """tests/regions_cases.py edge by edge in ascending order (block=1), the same in blocks of edges, and the module's own
    copy, which picks the anchor and decides anchor_inside: one result, bit for bit, on every region of these tests, on the
    degenerate nodes and on a table of 1 000 edges."""
    regions = list(RC.named_regions().values()) + [RC.region_with(1000)]
    for k, reg in enumerate(regions):
        pts = RC.node_groups(200, 1, reg.edges, reg.anchor, seed=k)
        for cutoff, scale in ((0.1, 6371000.0), (2.0, 1.0)):
            a = RC.region_distance(pts, reg.edges, reg.anchor, reg.anchor_inside, cutoff, scale)
            assert a[4] == 5                                            # the centre, a NaN, two infs, a node below 2^-500
            for b in (RC.region_distance(pts, reg.edges, reg.anchor, reg.anchor_inside, cutoff, scale, block=7),
                      RC.region_distance(pts, reg.edges, reg.anchor, reg.anchor_inside, cutoff, scale, block=4096),
                      RG.statement(pts, reg.edges, reg.anchor, reg.anchor_inside, cutoff, scale),
                      RG.statement(pts, reg.edges, reg.anchor, reg.anchor_inside, cutoff, scale, block=1)):
                assert RC.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert RC.MIN_RADIUS == RG.MIN_RADIUS == 2.0 ** -500


def test_a_region_of_16_391_edges_is_built_in_seconds():
    """The constructor evaluates the statement a handful of times over all edges (24 anchor candidates in one pass): it must stay
    far below the minutes an edge-by-edge loop takes.  Measured here: about a second; allowed: 20 s on any machine."""
    import time

    t = time.perf_counter()
    reg = RC.big_region()
    assert len(reg.edges) == 2 * 256 * RC.CHUNK + 7 and time.perf_counter() - t < 20.0
    assert reg.anchor_distance >= RG.MIN_ANCHOR_CHORD


def test_a_box_whose_corners_are_antipodal():
    box = RG.Region.from_box(0.0, 10.0, 0.0, 180.0, step=1.0)
    assert len(box.edges) == 2 * 180 + 2 * 10 and _inside(box, [[5.0, 90.0], [5.0, -90.0], [11.0, 90.0]]) == [1, 0, 0]


# ----------------------------------------------------------------------------------- the statement against other methods
@pytest.mark.parametrize("name", list(RC.named_regions()))
def test_the_inside_flag_against_winding_numbers(name):
    reg = RC.named_regions()[name]
    pts = RC.sphere_points(20000, seed=len(name))
    inside = RC.region_distance(pts, reg.edges, reg.anchor, reg.anchor_inside, 2.0, 1.0)[1].astype(bool)
    want, near = RC.winding_inside(pts, reg)
    print(f"{name}: {int(inside.sum())} inside, {int(near.sum())} left out")
    assert near.sum() <= 20 and near.sum() <= 0.01 * len(pts)          # the independent method alone leaves out far fewer than 1 %
    assert 100 < inside.sum() < len(pts) - 100 and np.array_equal(inside[~near], want[~near])


@pytest.mark.parametrize("name", list(RC.named_regions()))
def test_the_distance_against_samples_of_the_arcs(name):
    reg = RC.named_regions()[name]
    pts = RC.sphere_points(500, seed=7 + len(name))
    d = np.abs(RC.region_distance(pts, reg.edges, reg.anchor, reg.anchor_inside, 2.0, 1.0)[0])
    sampled, spacing = RC.sampled_distance(pts, reg, per_arc=2000)
    # distance <= sampled holds between exact values; both sides are computed: a sample's coordinates carry about four roundings
    # of 2^-53 and its chord three more, the statement's d about six, on values up to 2: together below 16 * 2^-53 * 2 = 2^-48,
    # which is all that is allowed (measured excess on these inputs: 1 to 2 ulp, 4.4e-16 at the most)
    print(f"{name}: largest d - sampled = {(d - sampled).max():.3g}")
    assert (d <= sampled + 2.0 ** -48).all() and (d >= sampled - spacing).all()


def test_a_vertex_on_the_arc_to_the_anchor_is_counted_once():
    """Nodes beyond a vertex as seen from the anchor, built from the vertex's own bits: inside iff a neighbour just off the
    great circle on the generic side is."""
    reg = RC.region_with(12)
    a = reg.anchor
    for U in reg.edges[:, 0:3]:
        beyond = (2.0 * (a @ U)) * U - a
        side = np.cross(a, U)
        flags = RC.region_distance(np.array([beyond + 1e-7 * side, beyond, beyond - 1e-7 * side]), reg.edges, a, reg.anchor_inside, 2.0, 1.0)[1]
        assert flags[1] in (flags[0], flags[2])


# --------------------------------------------------------------------------------------- the cases of the guarded test
def test_the_guarded_cases_span_the_byte_classes_and_end_on_a_deciding_edge():
    cases = RC.guarded_cases()
    for what in ("points", "edges", "signed", "inside"):
        assert G.classes(cases, what) == {"pages", "granule", "neither"}, what
    for case in cases:
        assert len(case["edges"]) % RC.CHUNK != 0 or len(case["edges"]) == 512
        ndist, ncross = RC.guarded_last_edge(case)
        assert ndist > 0 and ncross > 0, (case["name"], ndist, ncross)
