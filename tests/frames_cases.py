"""The NumPy statement of include/multimesh_frames.h, operation by operation -- every product, quotient, sum and square
root a separate IEEE binary64 operation, sums left to right --, and the case builders of tests/test_frames.py and
tests/test_frames_gpu.py."""
import numpy as np

R_EARTH = 6371000.0
EPS = np.finfo(np.float64).eps
RTP, ZNE = 0, 1                    # MM_FRAMES_BASIS_*
TO_LOCAL, TO_CARTESIAN = 0, 1      # MM_FRAMES_TO_*


# ------------------------------------------------------------------------------------------------------- the statement
def rotate(R, x, y, z, transpose=False):
    """(x', y', z') of the header's ROTATION for arrays x, y, z."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    if transpose:
        R = R.T
    with np.errstate(all="ignore"):
        return ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z,
                (R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z,
                (R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z)


def rotate_points(R, points, transpose=False):
    """mm_rotate_points: f64[..., 3] -> f64[..., 3]."""
    p = np.asarray(points, dtype=np.float64)
    return np.stack(rotate(R, p[..., 0], p[..., 1], p[..., 2], transpose), axis=-1)


def rotate_vectors(R, planes, transpose=False):
    """mm_rotate_vectors on planes f64[3, ...]."""
    v = np.asarray(planes, dtype=np.float64)
    return np.stack(rotate(R, v[0], v[1], v[2], transpose))


def local_basis(points):
    """(st, ct, sp, cp) of the header's LOCAL BASIS at positions f64[..., 3]."""
    p = np.asarray(points, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) + z * z)
        s = np.sqrt(x * x + y * y)
        off_axis = s > 0.0
        safe = np.where(off_axis, s, 1.0)
        cp = np.where(off_axis, x / safe, 1.0)
        sp = np.where(off_axis, y / safe, 0.0)
        return s / r, z / r, sp, cp


def local_components(points, planes, direction=TO_LOCAL, basis=RTP):
    """mm_local_components on planes f64[3, ...] over positions f64[..., 3]."""
    st, ct, sp, cp = local_basis(points)
    u, v, w = (np.asarray(a, dtype=np.float64) for a in planes)
    with np.errstate(all="ignore"):
        if direction == TO_LOCAL:
            a_r = ((st * cp) * u + (st * sp) * v) + ct * w
            a_t = ((ct * cp) * u + (ct * sp) * v) - st * w
            a_p = cp * v - sp * u
            return np.stack([a_r, -a_t if basis == ZNE else a_t, a_p])
        if basis == ZNE:
            v = -v
        vx = ((st * cp) * u + (ct * cp) * v) - sp * w
        vy = ((st * sp) * u + (ct * sp) * v) + cp * w
        vz = ct * u - st * v
        return np.stack([vx, vy, vz])


def same_bits_nan(a, b):
    """Equal bit for bit where neither is a NaN, and NaN in the same places (a NaN's payload and sign are the processor's)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


# ------------------------------------------------------------------------------------------------------------ the cases
def matrix(seed=0):
    """A rotation by a generic angle about a generic axis: nine entries none of which is 0 or 1 (host arithmetic; how it
    was made does not matter to the device, which applies what it is given)."""
    rng = np.random.default_rng(1000 + seed)
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1].copy()


def cloud(n, seed=0):
    """n points at Earth scale, f64[n, 3]."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    return d * rng.uniform(3.4e6, R_EARTH, (n, 1))


def special_rows():
    """Rows that hold NaN, +-inf, -0.0 and denormals."""
    return np.array([[np.nan, 1.0, 2.0], [1.0, np.nan, -2.0], [np.inf, 1.0, 1.0], [1.0, -np.inf, 1.0], [np.inf, -np.inf, 0.0],
                     [-0.0, -0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, 3.0, -0.0], [5e-324, -5e-324, 1e-310], [1e308, 1e308, -1e308]])


def special_positions():
    """Positions for the local basis: both poles (s = 0), the centre (r = 0), NaN coordinates, the axes of the equator,
    a negative zero and an infinity."""
    r = R_EARTH
    return np.array([[0.0, 0.0, r], [0.0, 0.0, -r], [-0.0, 0.0, r], [0.0, 0.0, 0.0], [np.nan, 1.0, r], [1.0, 2.0, np.nan],
                     [r, 0.0, 0.0], [-r, 0.0, 0.0], [0.0, r, 0.0], [0.0, -r, -0.0], [np.inf, 1.0, 1.0], [1e-200, 0.0, 1.0]])


def vectors(shape, seed=0):
    """Three components over ``shape``: f64[3, *shape]."""
    return np.random.default_rng(500 + seed).normal(size=(3,) + tuple(shape)) * 1e-3


def rows_of(planes, ncol, cols, seed=0):
    """Planes f64[3, E, P] laid into MODEL/data rows f64[E, ncol, P] at the columns ``cols``; the other columns hold noise."""
    _, E, P = planes.shape
    rows = np.random.default_rng(900 + seed).normal(size=(E, ncol, P))
    for c, col in enumerate(cols):
        rows[:, col, :] = planes[c]
    return rows
