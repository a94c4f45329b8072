"""The NumPy statement of the operator transpose (mm_transpose_* in include/multimesh_hip.h) and the operators the tests
apply it to.  Nothing here imports the code under test.

The definition is ``np.add.at`` on zeros, which is the sequential loop in ascending flat index (tests/test_transpose.py
checks that on the CPU, bit for bit):

  node form     out[c][j]    = (((+0.0 + t1) + t2) + ...), t = w[n][p] * v[n][c], over ids[n][p] == j, ascending n * P + p
  element form  out[c][e][p] = the same sum of coeffs[n][p] * v[n][c] over elem[n] == e, ascending n; elem -1 is skipped

Every product is rounded on its own before it is added (NumPy forms ``w * v`` as an array first).

The ordering cases carry values with a wide dynamic range, so that the order of a row's terms shows in the bits of its
sum: ``*_reversed`` sums every row from its far end, and tests/test_transpose.py asserts that this changes at least one
destination of every case -- a comparison with the reference is then a test of the order, not only of the set of terms.
"""
import functools

import numpy as np

LONG_ROW = 32       # mm_transpose.hip kLongRow: node-form rows of more contributions are summed by a wave each ...
WAVE = 64           # ... 64 products per step, so row lengths around multiples of 64 end a step
ELEM_GROUPS = (4, 8, 16, 32, 64)   # element form: lanes per element, and targets per step of a group
NODE_PS = (1, 4, 8, 27, 128)
ELEM_PS = (4, 9, 25, 8, 27, 125)
# row lengths around every bin edge of the node form (empty, the lane bin up to LONG_ROW, whole and broken steps of a wave)
STRADDLE_LENGTHS = (0, 1, 2, 3, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, LONG_ROW + 2, 63, 64, 65, 127, 128, 129, 191, 192, 193,
                    255, 256, 257, 1000, 4097)


# ------------------------------------------------------------------------------------------------ the reference
def transpose_nodes(ids, w, values, nsrc):
    """values f64[N, C] -> f64[C, nsrc]: np.add.at on zeros."""
    ids, w, values = np.asarray(ids), np.asarray(w), np.asarray(values).reshape(len(ids), -1)
    out = np.zeros((values.shape[1], nsrc))
    for c in range(values.shape[1]):
        np.add.at(out[c], ids, w * values[:, c, None])
    return out


def transpose_elem(elem, coeffs, values, nelem):
    """values f64[N, C] -> f64[C, nelem, P]: np.add.at on zeros over the rows with an element."""
    elem, coeffs, values = np.asarray(elem), np.asarray(coeffs), np.asarray(values).reshape(len(elem), -1)
    out = np.zeros((values.shape[1], nelem, coeffs.shape[1]))
    found = elem >= 0
    for c in range(values.shape[1]):
        np.add.at(out[c], elem[found], coeffs[found] * values[found, c, None])
    return out


def transpose_nodes_loop(ids, w, values, nsrc):
    """The explicit loop of the definition (small cases)."""
    ids, w, values = np.asarray(ids), np.asarray(w), np.asarray(values).reshape(len(ids), -1)
    out = np.zeros((values.shape[1], nsrc))
    n, P = ids.shape
    for c in range(values.shape[1]):
        for flat in range(n * P):
            i, p = divmod(flat, P)
            t = np.float64(w[i, p]) * np.float64(values[i, c])
            out[c, ids[i, p]] = out[c, ids[i, p]] + t
    return out


def transpose_elem_loop(elem, coeffs, values, nelem):
    elem, coeffs, values = np.asarray(elem), np.asarray(coeffs), np.asarray(values).reshape(len(elem), -1)
    P = coeffs.shape[1]
    out = np.zeros((values.shape[1], nelem, P))
    for c in range(values.shape[1]):
        for i in range(len(elem)):
            if elem[i] < 0:
                continue
            for p in range(P):
                t = np.float64(coeffs[i, p]) * np.float64(values[i, c])
                out[c, elem[i], p] = out[c, elem[i], p] + t
    return out


def transpose_nodes_reversed(ids, w, values, nsrc):
    """Every row summed from its far end (descending flat index): what a broken in-row order would give."""
    ids, w, values = np.asarray(ids), np.asarray(w), np.asarray(values).reshape(len(ids), -1)
    out = np.zeros((values.shape[1], nsrc))
    for c in range(values.shape[1]):
        np.add.at(out[c], ids.ravel()[::-1], (w * values[:, c, None]).ravel()[::-1])
    return out


def transpose_elem_reversed(elem, coeffs, values, nelem):
    return transpose_elem(np.asarray(elem)[::-1], np.asarray(coeffs)[::-1],
                          np.asarray(values).reshape(len(elem), -1)[::-1], nelem)


def same_bits(a, b):
    """Bit equality of two f64 arrays (distinguishes -0.0 from +0.0; NaNs compare by pattern)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def wide(rng, shape):
    """Values over sixteen decades with both signs: sums of them depend on the order of the terms."""
    return rng.normal(size=shape) * 10.0 ** rng.uniform(-8.0, 8.0, size=shape)


# ------------------------------------------------------------------------------------------------ the operators
@functools.lru_cache(maxsize=None)
def node_case(name):
    """(ids int64[N, P], w f64[N, P], nsrc) of one node-form ordering case."""
    if name.startswith("P"):                      # random destinations, P = 1 .. 128; rows of ~4 P contributions
        P = int(name[1:])
        rng = np.random.default_rng(1000 + P)
        n, nsrc = 3000, 750
        return rng.integers(0, nsrc, size=(n, P)), wide(rng, (n, P)), nsrc
    if name == "one_node":                        # every target on one node: one row of 1.6 M terms, ten nodes unnamed
        rng = np.random.default_rng(7)
        n = 200_000
        return np.full((n, 8), 5, dtype=np.int64), wide(rng, (n, 8)), 11
    if name.startswith("straddle"):               # one row of every length in STRADDLE_LENGTHS (P = 1), three orders
        rng = np.random.default_rng(11)
        lengths = np.array(STRADDLE_LENGTHS)
        dest = rng.permutation(len(lengths))      # (the row lengths do not follow the node numbers)
        ids = np.repeat(dest, lengths)
        order = {"straddle_unsorted": rng.permutation(len(ids)), "straddle_sorted": np.argsort(ids, kind="stable"),
                 "straddle_reverse_sorted": np.argsort(-ids, kind="stable")}[name]
        w = wide(rng, len(ids))
        return ids[order].reshape(-1, 1).astype(np.int64), w[order].reshape(-1, 1), len(lengths)
    if name == "skewed":                          # a fine cloud in a coarse source: a few long rows among short ones
        rng = np.random.default_rng(13)
        n, nsrc = 40_000, 5000
        ids = rng.integers(0, nsrc - 50, size=(n, 8))     # (the last fifty nodes stay unnamed)
        heavy = rng.random((n, 8)) < 0.3
        ids[heavy] = rng.integers(0, 6, size=int(heavy.sum())) * 7
        return ids, wide(rng, (n, 8)), nsrc
    raise KeyError(name)


NODE_CASES = tuple(f"P{p}" for p in NODE_PS) + ("one_node", "straddle_unsorted", "straddle_sorted",
                                                "straddle_reverse_sorted", "skewed")


@functools.lru_cache(maxsize=None)
def elem_case(name):
    """(elem int64[N], coeffs f64[N, P], nelem) of one element-form ordering case."""
    if name.startswith("P"):                      # random elements, some targets outside (-1), some elements empty
        P = int(name[1:])
        rng = np.random.default_rng(2000 + P)
        n, nelem = 3000, 200
        elem = rng.integers(0, nelem - 20, size=n)
        elem[rng.random(n) < 0.1] = -1
        return elem, wide(rng, (n, P)), nelem
    if name == "one_elem":                        # every target in one element: 200 k rows through one group of lanes
        rng = np.random.default_rng(17)
        n = 200_000
        return np.full(n, 3, dtype=np.int64), wide(rng, (n, 27)), 9
    if name == "elem_straddle":                   # elements with 0, 1, G - 1, G, G + 1 ... targets for every group size
        rng = np.random.default_rng(19)
        lengths = np.array(sorted({0, 1, 2} | {g + d for g in ELEM_GROUPS for d in (-1, 0, 1)} | {127, 128, 129, 1000}))
        dest = rng.permutation(len(lengths))
        elem = np.repeat(dest, lengths)
        elem = np.concatenate([elem, np.full(37, -1)])[rng.permutation(len(elem) + 37)]
        return elem.astype(np.int64), wide(rng, (len(elem), 9)), len(lengths)
    raise KeyError(name)


ELEM_CASES = tuple(f"P{p}" for p in ELEM_PS) + ("one_elem", "elem_straddle")


def case_values(name, n, ncomp):
    """values f64[N, C] of a case (wide dynamic range), the same on every call."""
    rng = np.random.default_rng(abs(hash_name(name)) % (2 ** 31) + ncomp)
    return wide(rng, (n, ncomp))


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (2 ** 61 - 1)
    return h


def golden_operator(golden, name):
    """(enc, w, nsrc) of a hex8 fixture (tests/golden/<name>.npz): rows of failed targets are all zero."""
    d = golden(name)
    return np.ascontiguousarray(d["enc"]), np.ascontiguousarray(d["w"]), int(d["points_a"].shape[0])
