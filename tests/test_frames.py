"""Frames without a GPU: the extension header against the module's signature table, :class:`Rotation` on the host (the
reference's matrices bit for bit, the rotation to the north pole, what ``check`` refuses, inverse and composition), the NumPy
statement of tests/frames_cases.py against the reference's ``rotate`` and its own rules for the local basis, and the
argument errors that are decided before the device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frames_cases as FC
from multimesh_amd import frames as F
from multimesh_amd import helpers
from multimesh_amd.api import GllMesh
from multimesh_amd.mesh import HexMesh
from test_parametrisation import _c_class, _ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multimesh_frames.h")
SYMBOLS = ["mm_rotate_points", "mm_rotate_vectors", "mm_local_components"]
EPS = FC.EPS


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "rotation.npz")) as g:
        return {k: g[k] for k in g.files}


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
    assert list(protos) == list(F.SIGNATURES) == SYMBOLS
    lib = F.bind()
    assert lib is helpers.load_lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = F.SIGNATURES[name]
        assert (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes]) == (ret, params), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert name not in helpers.SIGNATURES and name not in helpers.EXPORTED_SYMBOLS
    text = open(HEADER).read()
    params = open(os.path.join(ROOT, "include", "multimesh_params.h")).read()
    assert int(re.search(r"#define MM_PARAM_MAX_P (\d+)", params).group(1)) == F.MAX_P
    for name, number in F.BASIS.items():
        assert int(re.search(rf"#define MM_FRAMES_BASIS_{name.upper()} (\d+)", text).group(1)) == number
    assert int(re.search(r"#define MM_FRAMES_TO_LOCAL (\d+)", text).group(1)) == FC.TO_LOCAL == 0
    assert int(re.search(r"#define MM_FRAMES_TO_CARTESIAN (\d+)", text).group(1)) == FC.TO_CARTESIAN == 1
    assert (FC.RTP, FC.ZNE) == (F.BASIS["rtp"], F.BASIS["zne"])


def test_the_library_exports_the_symbols():
    lib = helpers.load_lib()
    assert all(hasattr(lib, s) for s in SYMBOLS)


# ------------------------------------------------------------------------------------------------------------ Rotation
def test_from_axis_angle_is_the_references_matrix_bit_for_bit(golden):
    angles, axes, matrices = golden["angles"], golden["axes"], golden["matrices"]
    assert len(angles) >= 20 and 0.0 in angles and 180.0 in angles
    assert (np.abs(np.linalg.norm(axes, axis=1) - 1.0) > 1e-3).sum() >= 5           # axes that are not normalised
    for angle, axis, want in zip(angles, axes, matrices):
        got = F.Rotation.from_axis_angle(axis, angle).matrix
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (angle, axis)
        assert np.array_equal(F.Rotation.from_axis_angle_rad(axis, np.deg2rad(angle)).matrix, want)
    with pytest.raises(ValueError, match="axis"):
        F.Rotation.from_axis_angle([0.0, 0.0, 0.0], 10.0)
    with pytest.raises(ValueError, match="angle"):
        F.Rotation.from_axis_angle([0.0, 0.0, 1.0], np.inf)


def _direction(lat, lon):
    phi, lam = np.deg2rad(lat), np.deg2rad(lon)
    return np.array([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)])


def test_to_north_pole():
    rng = np.random.default_rng(7)
    lats = np.concatenate([rng.uniform(-90.0, 90.0, 200), [0.0, 45.0, -45.0, 89.999999, -89.999999, 1e-9, 37.0]])
    lons = np.concatenate([rng.uniform(-360.0, 360.0, 200), [0.0, 180.0, -90.0, 10.0, 20.0, 30.0, 360.0]])
    for lat, lon in zip(lats, lons):
        R = F.Rotation.to_north_pole(lat, lon)
        e = _direction(lat, lon)
        assert np.abs(R.matrix @ e - [0.0, 0.0, 1.0]).max() <= 4 * EPS, (lat, lon)
        lam = np.deg2rad(lon)
        axis = np.array([np.sin(lam), -np.cos(lam), 0.0])                           # e x n, normalised
        assert np.abs(R.matrix @ axis - axis).max() <= 4 * EPS, (lat, lon)
        F.Rotation(R.matrix, check=True)                                            # it passes the check
        assert np.abs(R.inverse().matrix @ [0.0, 0.0, 1.0] - e).max() <= 4 * EPS
    assert np.array_equal(F.Rotation.to_north_pole(90.0, 123.0).matrix, np.eye(3))
    assert np.array_equal(F.Rotation.to_north_pole(-90.0, -5.0).matrix, np.diag([-1.0, 1.0, -1.0]))    # a half turn about y
    # the sense: a point on the equator at lon 0 goes to the pole, the pole goes to lon 180
    R = F.Rotation.to_north_pole(0.0, 0.0).matrix
    assert np.abs(R @ [1.0, 0.0, 0.0] - [0.0, 0.0, 1.0]).max() <= 4 * EPS and np.abs(R @ [0.0, 0.0, 1.0] - [-1.0, 0.0, 0.0]).max() <= 4 * EPS
    for bad in ((91.0, 0.0), (np.nan, 0.0), (0.0, np.inf)):
        with pytest.raises(ValueError, match="lat"):
            F.Rotation.to_north_pole(*bad)


def test_check_refuses_what_is_not_a_rotation():
    R = FC.matrix(1)
    F.Rotation(R)
    with pytest.raises(ValueError, match="not a rotation"):
        F.Rotation(R * (1.0 + 1e-11))                                               # scaled: |R^T R - I| ~ 2e-11
    F.Rotation(R * (1.0 + 1e-14))                                                   # within the tolerance
    with pytest.raises(ValueError, match="reflection"):
        F.Rotation(R @ np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError, match="finite"):
        F.Rotation(np.where(np.eye(3) > 0, np.nan, 0.0), check=False)
    with pytest.raises(ValueError, match=r"\[3, 3\]"):
        F.Rotation(np.eye(4))
    skew = F.Rotation(2.0 * R, check=False)                                         # check=False: the caller's business
    assert np.array_equal(skew.matrix, 2.0 * R)
    given = R.copy()
    rot = F.Rotation(given)
    given[0, 0] = 5.0
    assert rot.matrix[0, 0] == R[0, 0]                                              # it holds a copy


def test_inverse_and_composition():
    a, b = F.Rotation(FC.matrix(2)), F.Rotation(FC.matrix(3))
    assert np.array_equal(a.inverse().matrix, a.matrix.T)
    assert np.array_equal((a @ b).matrix, a.matrix @ b.matrix)
    assert np.abs((a @ a.inverse()).matrix - np.eye(3)).max() <= 8 * EPS
    p = FC.cloud(10, seed=1)
    assert np.allclose(FC.rotate_points((a @ b).matrix, p), FC.rotate_points(a.matrix, FC.rotate_points(b.matrix, p)), rtol=0, atol=1e-8)
    with pytest.raises(TypeError):
        a @ np.eye(3)


# ------------------------------------------------------------------------------------------------------- the statement
def test_the_statement_agrees_with_the_references_rotate(golden):
    """The reference's ``matrix.dot`` may sum in any order or fuse; two evaluations of a 3-term dot product each err by at
    most 3 eps sum_j |R_ij| |p_j| to first order: the bound is 6 eps (|R| |p|), elementwise."""
    assert golden["points"].shape[0] * golden["points"].shape[1] >= 1000
    for R, p, want in zip(golden["matrices"], golden["points"], golden["rotated"]):
        got = FC.rotate_points(R, p)
        bound = 6 * EPS * (np.abs(p) @ np.abs(R).T)
        assert (np.abs(got - want) <= bound).all()
        back = FC.rotate_points(R, got, transpose=True)
        assert np.abs(back - p).max() <= 1e-8                                      # the transpose is the way back


def test_the_statement_on_special_values():
    R = FC.matrix(4)
    assert (R != 0.0).all()
    out = FC.rotate_points(R, FC.special_rows())
    assert np.isnan(out[0]).all() and np.isnan(out[1]).all()                        # a NaN coordinate reaches every output
    assert np.array_equal(out[2], np.where(R[:, 0] > 0, np.inf, -np.inf))           # +inf in x: the sign of the first column
    assert np.array_equal(FC.rotate_points(np.eye(3), FC.cloud(50, seed=2)), FC.cloud(50, seed=2))    # 1*x + 0*y + 0*z is x
    assert np.array_equal(FC.rotate_points(R, FC.cloud(50, seed=2), transpose=True), FC.rotate_points(R.T.copy(), FC.cloud(50, seed=2)))


def test_the_local_basis_is_orthonormal_and_direction_1_undoes_direction_0():
    pts = FC.cloud(500, seed=3)
    v = FC.vectors((500,), seed=3)
    st, ct, sp, cp = FC.local_basis(pts)
    basis = np.stack([np.stack([st * cp, st * sp, ct]), np.stack([ct * cp, ct * sp, -st]), np.stack([-sp, cp, np.zeros(500)])])
    gram = np.einsum("aip,bip->abp", basis, basis)
    assert np.abs(gram - np.eye(3)[:, :, None]).max() <= 8 * EPS
    assert np.abs(basis[0] - (pts / np.linalg.norm(pts, axis=1, keepdims=True)).T).max() <= 4 * EPS      # radial is p / |p|
    norm = np.sqrt((v * v).sum(axis=0))
    for basis_id in (FC.RTP, FC.ZNE):
        local = FC.local_components(pts, v, FC.TO_LOCAL, basis_id)
        back = FC.local_components(pts, local, FC.TO_CARTESIAN, basis_id)
        assert (np.abs(back - v) <= 32 * EPS * norm).all()
        assert np.abs(np.sqrt((local * local).sum(axis=0)) - norm).max() <= 8 * EPS * norm.max()


def test_the_pole_takes_longitude_zero_and_the_centre_gives_nan():
    pos = FC.special_positions()
    v = FC.vectors((len(pos),), seed=5)
    local = FC.local_components(pos, v)
    # north pole: radial = vz, south = vx, east = vy; south pole: radial = -vz, south = -vx, east = vy
    assert np.array_equal(local[:, 0], [v[2, 0], v[0, 0], v[1, 0]])
    assert np.array_equal(local[:, 1], [-v[2, 1], -v[0, 1], v[1, 1]])
    assert np.array_equal(local[:, 2], [v[2, 2], v[0, 2], v[1, 2]])                 # (-0.0, 0, r): s is +0 too
    assert np.isnan(local[:2, 3]).all() and local[2, 3] == v[1, 3]                  # the centre: st and ct are 0 / 0
    assert np.isnan(local[:2, 4]).all() and local[2, 4] == v[1, 4]                  # a NaN s: longitude 0, like the pole
    assert np.isnan(local[:2, 5]).all() and np.isfinite(local[2, 5])                # a NaN z: the east component has no z in it
    assert np.array_equal(local[:, 6], [v[0, 6], -v[2, 6], v[1, 6]])                # (r, 0, 0): radial x, south -z, east y


def test_basis_1_is_the_exact_negation_of_the_south_component():
    pos = np.concatenate([FC.cloud(200, seed=6), FC.special_positions()])
    v = FC.vectors((len(pos),), seed=6)
    rtp, zne = FC.local_components(pos, v, FC.TO_LOCAL, FC.RTP), FC.local_components(pos, v, FC.TO_LOCAL, FC.ZNE)
    sign = np.uint64(1) << np.uint64(63)
    assert np.array_equal(zne[1].view(np.uint64), rtp[1].view(np.uint64) ^ sign)    # the sign bit, of a NaN too
    assert np.array_equal(zne[[0, 2]].view(np.uint64), rtp[[0, 2]].view(np.uint64))
    flipped = np.stack([v[0], -v[1], v[2]])
    assert FC.same_bits_nan(FC.local_components(pos, v, FC.TO_CARTESIAN, FC.ZNE), FC.local_components(pos, flipped, FC.TO_CARTESIAN, FC.RTP))


# --------------------------------------------------------------------------------------------------- argument checks
CTX = C.c_void_p(0x1000)            # a dummy: a refused call never looks at the context
A, B, PTS = 0x100000, 0x900000, 0x4000000          # never read
IDENTITY = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
COLS = (C.c_int * 3)(0, 1, 2)


def _matrix(**changed):
    m = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for k, v in changed.items():
        m[int(k[1:])] = v
    return (C.c_double * 9)(*m)


def _points(lib, ctx=CTX, n=10, a=A, b=B, R=IDENTITY, transpose=0):
    return lib.mm_rotate_points(ctx, n, a, b, R, transpose)


def _field_args(ngroups=10, P_=8, a=A, gs=8, cs=80, cols=COLS, b=B, ogs=8, ocs=80, ocols=COLS):
    return (ngroups, P_, a, gs, cs, cols, b, ogs, ocs, ocols)


def _vectors(lib, ctx=CTX, R=IDENTITY, transpose=0, **kw):
    return lib.mm_rotate_vectors(ctx, *_field_args(**kw), R, transpose)


def _local(lib, ctx=CTX, pts=PTS, direction=0, basis=0, **kw):
    ngroups, P_, *rest = _field_args(**kw)
    return lib.mm_local_components(ctx, ngroups, P_, pts, *rest, direction, basis)


POINTS_REFUSED = {
    "null ctx": dict(ctx=None),
    "negative n": dict(n=-1),
    "3 n at 2^48": dict(n=-(-(1 << 48) // 3)),
    "null R": dict(R=None),
    "NaN in R": dict(R=_matrix(m4=np.nan)),
    "inf in R": dict(R=_matrix(m8=np.inf)),
    "-inf in R": dict(R=_matrix(m0=-np.inf)),
    "null in": dict(a=None),
    "null out": dict(b=None),
    "out starts inside in": dict(b=A + 8),
    "out one point into in": dict(b=A + 24),
    "out ends inside in": dict(b=A - 24 * 9),
}
FIELD_REFUSED = {
    "null ctx": dict(ctx=None),
    "negative ngroups": dict(ngroups=-1),
    "ngroups at 2^48": dict(ngroups=1 << 48, P_=1, gs=0, ogs=0),
    "P zero": dict(P_=0),
    "P above the limit": dict(P_=4097),
    "null in": dict(a=None),
    "null out": dict(b=None),
    "null in cols": dict(cols=None),
    "null out cols": dict(ocols=None),
    "negative stride": dict(gs=-8),
    "negative column": dict(cols=(C.c_int * 3)(0, -1, 2)),
    "equal output columns": dict(ocols=(C.c_int * 3)(0, 1, 1)),
    "output nodes share an element": dict(ogs=4),
    "extent at 2^48": dict(ngroups=1 << 36, P_=4096, gs=4096, cs=1 << 48, ogs=4096, ocs=1 << 48),
    "partial overlap": dict(b=A + 8 * 40),
    "the same base with other strides": dict(b=A, ogs=24, ocs=8, gs=8, cs=80),
}


@pytest.mark.parametrize("what", list(POINTS_REFUSED))
def test_rotate_points_refuses_without_a_gpu(what):
    lib = F.bind()
    assert _points(lib, **POINTS_REFUSED[what]) == -1, what
    message = lib.mm_last_error()
    assert b"mm_rotate_points" in message and len(message) > len(b"mm_rotate_points: "), message
    assert lib.mm_last_status() == -1


@pytest.mark.parametrize("entry", ("mm_rotate_vectors", "mm_local_components"))
@pytest.mark.parametrize("what", list(FIELD_REFUSED))
def test_the_field_entry_points_refuse_without_a_gpu(entry, what):
    lib = F.bind()
    call = _vectors if entry == "mm_rotate_vectors" else _local
    assert call(lib, **FIELD_REFUSED[what]) == -1, what
    message = lib.mm_last_error()
    assert entry.encode() in message and len(message) > len(entry) + 2, message


def test_what_only_one_field_entry_point_refuses_without_a_gpu():
    lib = F.bind()
    for R in (None, _matrix(m2=np.nan), _matrix(m6=-np.inf)):
        assert _vectors(lib, R=R) == -1 and b"mm_rotate_vectors: R" in lib.mm_last_error()
    for kw in (dict(direction=2), dict(direction=-1), dict(basis=2), dict(basis=-1), dict(pts=None),
               dict(pts=B + 8), dict(pts=B - 8)):
        assert _local(lib, **kw) == -1 and b"mm_local_components" in lib.mm_last_error(), kw


def test_nothing_to_do_is_valid_without_a_gpu():
    """n == 0 and ngroups == 0: MM_OK before the device is touched, null arrays allowed."""
    lib = F.bind()
    assert _points(lib, n=0, a=None, b=None) == 0
    assert _vectors(lib, ngroups=0, a=None, b=None) == 0
    assert _local(lib, ngroups=0, a=None, b=None, pts=None) == 0


def test_python_refuses_before_the_library_is_asked():
    flat = GllMesh(np.zeros((2, 9, 2)), 2, {})
    with pytest.raises(ValueError, match="3-D meshes only"):
        F.rotate_mesh(flat, F.Rotation.identity())
    with pytest.raises(ValueError, match="3-D meshes only"):
        F.in_frame(HexMesh(np.zeros((4, 2)), np.zeros((1, 4), dtype=np.int64)), F.Rotation.identity())
    with pytest.raises(ValueError, match="GllMesh or a HexMesh"):
        F.in_frame(np.zeros((4, 3)), F.Rotation.identity())
    with pytest.raises(ValueError, match="basis must be one of"):
        F.local_components(np.zeros((4, 3)), np.zeros((3, 4)), basis="enu")
