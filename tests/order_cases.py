"""The NumPy statement of the order change of element-nodal GLL values (mm_gll_tensor_apply in include/multimesh_hip.h), its
own construction of the 1-D table, and the bounds the tests assert.  Nothing here imports the code under test.

Per element, with m = order + 1, node p = i + m j + m^2 k (i fastest) and R f64[m_out][m_in]:

  v[a,b,c]      = in[a,b,c]                        or   in[a,b,c] * scale_in[e, p_in]
  t1[qi,b,c]    = sum_a R[qi][a] * v[a,b,c]
  t2[qi,qj,c]   = sum_b R[qj][b] * t1[qi,b,c]
  out[qi,qj,qk] = sum_c R[qk][c] * t2[qi,qj,c]     then   / div_out[e, p_out] if given          (2-D: out = t2)

Every product is rounded on its own (NumPy forms each as an array), every sum starts from its first term and runs in
ascending index: the loop over the summed index below is sequential, everything else is vectorised.  Nothing is
special-cased (0 * NaN is NaN).

Layouts of ``values`` (the same for the result, with P_out): 0 = [C, E, P], 1 = [E, P, C], 2 = [E, C, P].
"""
import numpy as np

EPS = 2.0 ** -52
ORDERS = (1, 2, 4)
PAIRS = [(a, b) for a in ORDERS for b in ORDERS if a != b]        # the 6 (order_in, order_out) of a dimension
UP = [(1, 2), (1, 4), (2, 4)]
SHAPES = [(a, b, dim) for dim in (2, 3) for a, b in PAIRS]        # the 12 kernels

# Bounds OBSERVED on this statement on the CPU (tests assert ten times each, the convention of
# gradient_cases.LINEAR_OBSERVED).  How each was obtained is said beside it; tests/test_order.py prints what it finds.
#
# |<I u, v> - <u, I^T v>|, both dot products by np.sum, for unit-normal u [1, 7, P_in] and v [1, 7, P_out] (rng seed
# 10 * order_in + order_out + dim, u drawn first), I = order_in -> order_out, I^T = the kernel from order_out to order_in
# with transposed_table; the larger of the 2-D and the 3-D case of a pair.  (Dot products of 28 .. 875 terms of size one.)
ADJOINT_OBSERVED = {(1, 2): 7.2e-15, (1, 4): 5.4e-15, (2, 4): 1.8e-15}
# max |upsampled gll_mesh(4, o_in, seed=3) - gll_mesh(4, o_out, seed=3)| in 3-D, layout 1 (coordinates in [0, 1], both
# built from the same trilinear map, so the difference is rounding alone).
COORDS_OBSERVED = {(1, 2): 1.2e-16, (1, 4): 3.4e-16, (2, 4): 4.5e-16}
# max |I f - f(nodes_out)| for f = the tensor polynomial prod_d sum_n c[d][n] x_d^n of degree order_in per axis with
# unit-normal coefficients (seed 100 + 10 * order_in + order_out + dim) on the reference element [-1, 1]^dim, relative to
# prod_d sum_n |c[d][n]|, the size of what is summed; the larger of 2-D and 3-D.
POLY_OBSERVED = {(1, 2): 5.9e-17, (1, 4): 1.3e-16, (2, 4): 1.3e-16}
# |int K_c - int K_f| / int |K_f| of the restriction statement (scale_in = M_f, transposed table, div_out = M_c, masses of
# mass_cases.mass, M_c on the subsampled coordinates) with unit-normal K_f [1, E, P] (seed 7) on earth_chunk(order_f,
# nlat=3, nlon=3, ellipticity=3.3e-3, topography=3e-4); every integral by mass_cases.weighted_sum, the statement of what
# api.integrate computes, so the device repeats these figures.  The pairs are (order_f, order_c).
RESTRICT_OBSERVED = {(4, 2): 3.2e-18, (4, 1): 4.2e-18, (2, 1): 3.7e-17}


def nodes(order):
    """The GLL nodes on [-1, 1], written out."""
    return {1: np.array([-1.0, 1.0]), 2: np.array([-1.0, 0.0, 1.0]),
            4: np.array([-1.0, -np.sqrt(3.0 / 7.0), 0.0, np.sqrt(3.0 / 7.0), 1.0])}[order]


def table(order_in, order_out):
    """R[q][a] = l_a^in(g_q^out): an exact unit row where g_q^out is an input node, else the product of
    (x - g_b) / (g_a - g_b) over b != a in ascending b."""
    gi, go = nodes(order_in), nodes(order_out)
    R = np.zeros((len(go), len(gi)))
    for q, x in enumerate(go):
        same = [a for a in range(len(gi)) if gi[a] == x]
        if same:
            R[q, same[0]] = 1.0
            continue
        for a in range(len(gi)):
            prod = None
            for b in range(len(gi)):
                if b == a:
                    continue
                f = (x - gi[b]) / (gi[a] - gi[b])
                prod = f if prod is None else prod * f
            R[q, a] = prod
    return R


def transposed_table(order_in, order_out):
    """The table that makes the kernel, run from order_in to order_out, the TRANSPOSE of the interpolation
    order_out -> order_in: table(order_out, order_in).T, f64[m_out][m_in], contiguous."""
    return np.ascontiguousarray(table(order_out, order_in).T)


def tile_elems(order_in, order_out, dim):
    """Elements that share one step of a 256-thread block of mm_gll_tensor_apply: 256 // max(P_in, P_out)."""
    return 256 // max((order_in + 1) ** dim, (order_out + 1) ** dim)


def _sweep(R, x, axis):
    """sum over the index of ``axis`` of R[q][a] * x[.., a, ..], ascending a, from the first term; the axis becomes q."""
    shape = [1] * x.ndim
    shape[axis] = R.shape[0]
    acc = None
    for a in range(R.shape[1]):
        t = R[:, a].reshape(shape) * np.take(x, [a], axis=axis)
        acc = t if acc is None else acc + t
    return acc


def to_planes(values, layout):
    """values in ``layout`` -> [C, E, P] (a view)."""
    v = np.asarray(values, dtype=np.float64)
    return v if layout == 0 else v.transpose(2, 0, 1) if layout == 1 else v.transpose(1, 0, 2)


def from_planes(planes, layout):
    """[C, E, P] -> a contiguous array in ``layout``."""
    p = planes if layout == 0 else planes.transpose(1, 2, 0) if layout == 1 else planes.transpose(1, 0, 2)
    return np.ascontiguousarray(p)


def tensor_apply(R, dim, values, layout=0, scale_in=None, div_out=None):
    """The statement: values in ``layout`` over (E, P_in) -> the same layout over (E, P_out)."""
    R = np.asarray(R, dtype=np.float64)
    mo, mi = R.shape
    v = to_planes(values, layout)
    C, E, P = v.shape
    assert P == mi ** dim and dim in (2, 3)
    if scale_in is not None:
        v = v * np.asarray(scale_in, dtype=np.float64)[None]
    x = v.reshape((C, E) + (mi,) * dim)                      # [C, E, (k,) j, i]
    for d in range(dim):                                     # i, then j, then k
        x = _sweep(R, x, x.ndim - 1 - d)
    out = x.reshape(C, E, mo ** dim)
    if div_out is not None:
        out = out / np.asarray(div_out, dtype=np.float64)[None]
    return from_planes(out, layout)


def element_deviation(a, b):
    """The statement of mm_element_deviation for a, b f64[E, P, dim]: (max |a - b| per element, NaN where a difference is;
    the largest bounding-box edge of b per element, fmax / fmin passing over a NaN)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    deviation = np.abs(a - b).reshape(len(a), -1).max(axis=1, initial=0.0)
    edge = np.fmax.reduce(np.fmax.reduce(b, axis=1) - np.fmin.reduce(b, axis=1), axis=1)
    return deviation, edge
