"""The kernels' hex8 Newton solve (multimesh_amd/csrc/mm_newton_hex8.h) compiled for the HOST and compared, iterate
for iterate, with the CPU oracle and the compiled reference (trilinearinterpolator.c:260-305; its iterates are stored as
digests in tests/golden/newton_reference.npz by tests/golden/make_golden.py).

The header restates the reference's expressions with fewer fp64 instructions (Jacobian carried at 8x, first trip
specialised at xi = 0, exact-product fused multiply-adds); the claim is bit equality of every final iterate and every
verdict, also when a solve is stopped at a cap and continued, the way locate_pass_kernel's tiers do it.  The same
header is what the GPU kernels compile, so this runs without a GPU; the -m gpu parity tests then check the kernels."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "newton_host.cpp")
HDR = os.path.join(HERE, "..", "multimesh_amd", "csrc", "mm_newton_hex8.h")
OUT = os.path.join(HERE, "host", "_build", "libnewton_host.so")

# corner (R, S, T) signs of trilinearinterpolator.c:8-10
RST = np.array([[-1, -1, -1], [-1, 1, -1], [1, 1, -1], [1, -1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], float)


@pytest.fixture(scope="module")
def host():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-fPIC", "-shared",
                        "-o", OUT, SRC], check=True)
    L = C.CDLL(OUT)
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags=["C_CONTIGUOUS"])
    L.nh_compare.restype = C.c_int64
    L.nh_compare.argtypes = [C.c_int64, f64p, f64p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                             C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.nh_newton.restype = C.c_int
    L.nh_newton.argtypes = [f64p, f64p, f64p, C.c_int, C.c_int]
    L.nh_solve.restype = None
    L.nh_solve.argtypes = [C.c_int64, f64p, f64p, C.c_int, C.c_int, C.c_int, f64p,
                           np.ctypeslib.ndpointer(dtype=np.int8, flags=["C_CONTIGUOUS"])]
    return L


def elements(rng, n, jitter, scale, offset, spread):
    """n hexahedra: the reference cube's corners, jittered, stretched per axis, moved to `offset`; one point each at
    `spread` reference units (normal) around the centre."""
    stretch = np.exp(rng.uniform(-1.0, 1.0, size=(n, 1, 3)))
    vtx = (RST[None] + rng.uniform(-jitter, jitter, size=(n, 8, 3))) * stretch * (0.5 * scale)
    pnt = vtx.mean(1) + rng.normal(scale=spread, size=(n, 3)) * stretch[:, 0] * (0.5 * scale)
    off = np.asarray(offset, float)
    return np.ascontiguousarray(pnt + off), np.ascontiguousarray(vtx + off)


DIGEST_BLOCK = 1000


def iterate_digests(xi, ok):
    """SHA-256 of every block of DIGEST_BLOCK solves: verdicts (0 / 1) and final iterates, NaNs made one bit pattern (NaN
    payloads are not part of the contract, as in nh_compare)."""
    xi = np.where(np.isnan(xi), np.nan, xi)
    ok = (np.asarray(ok) != 0).astype(np.int8)
    return [hashlib.sha256(ok[a:a + DIGEST_BLOCK].tobytes() + xi[a:a + DIGEST_BLOCK].tobytes()).digest()
            for a in range(0, len(ok), DIGEST_BLOCK)]


def input_digest(pnt, vtx):
    return hashlib.sha256(pnt.tobytes() + vtx.tobytes()).digest()


def compare(L, fn, no_iters, pnt, vtx, staged, c1=6, c2=9):
    first, conv = C.c_int64(), C.c_int64()
    bad = L.nh_compare(len(pnt), pnt, vtx, C.cast(fn, C.c_void_p), no_iters, staged, c1, c2, C.byref(first), C.byref(conv))
    return bad, first.value, conv.value


CASES = [
    # jitter, scale, offset, spread of the points (reference units)
    (0.25, 1.0, (0, 0, 0), 0.6),          # mildly distorted, points in and around the element
    (0.45, 1.0, (0.3, -0.2, 0.1), 1.5),   # strongly distorted, many rejections and slow solves
    (0.2, 29.5e3, (3.1e6, -2.2e6, 5.0e6), 0.8),   # Earth-scale coordinates in metres
    (0.0, 1.0, (0, 0, 0), 0.7),           # affine elements: one update and the closing residual
    (0.9, 1e-3, (1.0, 1.0, 1.0), 2.0),    # tangled elements far from the origin: divergence, caps, NaN
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_final_iterates_equal_the_oracle(host, case):
    jitter, scale, offset, spread = CASES[case]
    rng = np.random.default_rng(9000 + case)
    pnt, vtx = elements(rng, 200_000, jitter, scale, offset, spread)
    fn = O.lib().mmo_hex8_newton
    for staged in (0, 1):
        bad, first, conv = compare(host, fn, 0, pnt, vtx, staged)
        assert bad == 0, (case, staged, first)
    assert 0 < conv <= len(pnt)


def test_every_cap_pair_continues_to_the_same_iterate(host):
    rng = np.random.default_rng(77)
    pnt, vtx = elements(rng, 20_000, 0.45, 1.0, (0, 0, 0), 1.2)
    fn = O.lib().mmo_hex8_newton
    for c1, c2 in [(1, 2), (2, 3), (3, 7), (5, 6), (6, 9), (1, 49)]:
        bad, first, _ = compare(host, fn, 0, pnt, vtx, 1, c1, c2)
        assert bad == 0, (c1, c2, first)


REFERENCE_CASES = (0, 1, 2)
REFERENCE_SOLVES = 100_000


def reference_inputs():
    """The solves the compiled reference's iterates are stored for (tests/golden/newton_reference.npz)."""
    rng = np.random.default_rng(5)
    for case in REFERENCE_CASES:
        jitter, scale, offset, spread = CASES[case]
        yield case, elements(rng, REFERENCE_SOLVES, jitter, scale, offset, spread)


def test_final_iterates_equal_the_compiled_reference(host, golden):
    # the reference's 300,000 verdicts and final iterates are stored as SHA-256 digests of blocks of 1000 solves (the
    # iterates themselves are 7 MB): equal digests = every verdict and iterate bit-equal, NaN payloads aside
    d = golden("newton_reference")
    for i, (case, (pnt, vtx)) in enumerate(reference_inputs()):
        assert input_digest(pnt, vtx) == d["inputs"][i].tobytes(), f"case {case}: not the inputs the fixture was made from"
        xi, ok = np.zeros((len(pnt), 3)), np.zeros(len(pnt), np.int8)
        host.nh_solve(len(pnt), pnt, vtx, 1, 6, 9, xi, ok)
        bad = [b for b, dg in enumerate(iterate_digests(xi, ok)) if dg != d["iterates"][i, b].tobytes()]
        assert not bad, (case, [b * DIGEST_BLOCK for b in bad[:5]])


def test_the_gll_paths_corner_solve_equals_the_oracles(host):
    # mm_locate_gll.hip starts a 3-D inverse transform from newton_hex8_start (the corners' trilinear map in its polynomial
    # form, at most 8 trips); the oracle from mmo_hex8_start: the same iterate, bit for bit
    L = O.lib()
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags=["C_CONTIGUOUS"])
    host.nh_compare_start.restype = C.c_int64
    host.nh_compare_start.argtypes = [C.c_int64, f64p, f64p, C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    fn = C.cast(L.mmo_hex8_start, C.c_void_p)
    for case, (jitter, scale, offset, spread) in enumerate(CASES):
        rng = np.random.default_rng(700 + case)
        pnt, vtx = elements(rng, 100_000, jitter, scale, offset, spread)
        for cap in (8, 3, 1):
            first = C.c_int64()
            bad = host.nh_compare_start(len(pnt), pnt, vtx, fn, cap, C.byref(first))
            assert bad == 0, (case, cap, first.value)
    # and the polish does what it is for: on a straight-sided element the start is the solution to rounding
    rng = np.random.default_rng(1)
    pnt, vtx = elements(rng, 2000, 0.3, 1.0, (0, 0, 0), 0.5)
    host.nh_start.restype = C.c_int
    host.nh_start.argtypes = [f64p, f64p, f64p, C.c_int]
    worst = 0.0
    for p, v in zip(pnt, vtx):
        xi = np.zeros(3)
        host.nh_start(p, np.ascontiguousarray(v), xi, 8)
        if np.isfinite(xi).all() and np.abs(xi).max() < 1.2:
            r = 0.125 * ((1 + RST[:, 0] * xi[0]) * (1 + RST[:, 1] * xi[1]) * (1 + RST[:, 2] * xi[2])) @ v - p
            worst = max(worst, np.abs(r).max())
    assert worst < 1e-13


def test_degenerate_inputs_give_the_same_verdicts(host):
    # flat element (zero determinant), a point exactly at the centre, a point exactly on a corner, zero-size element
    L = O.lib()
    flat = RST.copy()
    flat[:, 2] = 0.0
    cube = RST.copy()
    for vtx, pnt in [(flat, [0.1, 0.2, 0.0]), (cube, [0.0, 0.0, 0.0]), (cube, [1.0, 1.0, 1.0]), (cube * 0.0, [0.0, 0.0, 0.0]),
                     (cube, [np.nan, 0.0, 0.0]), (cube * 1e-200, [1e-201, 0, 0])]:
        vtx = np.ascontiguousarray(vtx, float)
        pnt = np.ascontiguousarray(pnt, float)
        a, b = np.zeros(3), np.zeros(3)
        ok_o = L.mmo_hex8_newton(pnt, vtx, a, None)
        ok_m = host.nh_newton(pnt, vtx, b, 50, 0)
        assert bool(ok_o) == bool(ok_m)
        assert np.array_equal(a, b, equal_nan=True)
        assert np.array_equal(np.signbit(a), np.signbit(b)) or np.isnan(a).any()


# ----------------------------------------------------------------------------------------------------------------------
# MM_FP_TOL: newton_hex8_fast must reach the reference's verdict or say "unsure" (csrc/mm_newton_hex8.h)
# ----------------------------------------------------------------------------------------------------------------------
def fast_stats(host, pnt, vtx, cap=6):
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags=["C_CONTIGUOUS"])
    host.nh_fast_stats.restype = None
    host.nh_fast_stats.argtypes = [C.c_int64, f64p, f64p, C.c_void_p, C.c_int, np.ctypeslib.ndpointer(dtype=np.int64), f64p]
    out, dout = np.zeros(6, np.int64), np.zeros(4)
    host.nh_fast_stats(len(pnt), pnt, vtx, C.cast(O.lib().mmo_hex8_newton, C.c_void_p), cap, out, dout)
    return dict(accept=int(out[0]), reject=int(out[1]), unsure=int(out[2]), wrong=int(out[3]), tripdiff=int(out[4]),
                unsure_but_acceptable=int(out[5]), worst_over_delta=dout[0], worst=dout[1], max_delta=dout[2], max_ratio=dout[3])


@pytest.mark.parametrize("case", range(len(CASES)))
def test_fast_solve_never_certifies_a_wrong_verdict(host, case):
    # every certified accept / reject equals the reference's decision (converged within 50 trips AND max|xi| < 1.025),
    # the certified solves stop at the reference's trip, and their iterate is within a small fraction of the margin
    # delta of the reference's -- on mild, strong, Earth-scale, affine and tangled elements alike.  The tangled case
    # may certify few solves; it must not certify a wrong one.
    jitter, scale, offset, spread = CASES[case]
    rng = np.random.default_rng(31000 + case)
    pnt, vtx = elements(rng, 300_000, jitter, scale, offset, spread)
    for cap in (6, 9):
        st = fast_stats(host, pnt, vtx, cap)
        assert st["wrong"] == 0 and st["tripdiff"] == 0, (case, cap, st)
        assert st["worst_over_delta"] < 0.25, (case, cap, st)        # measured: 0.001 ... 0.11 (tangled elements)
        assert st["max_ratio"] <= 0.5                                  # certified solves contract two-fold per trip
    if case in (0, 2, 3):
        assert st["unsure"] < 0.01 * len(pnt), st                     # well-shaped elements: nearly everything certified
    assert st["accept"] + st["reject"] > 0.3 * len(pnt), st


def test_fast_solve_on_points_at_the_acceptance_threshold(host):
    # points placed at max|xi| = 1.025 -+ a few ulps to 1e-7: inside the band the verdict is "unsure", outside it is
    # certified and right
    rng = np.random.default_rng(5)
    n = 100_000
    vtx = (RST[None] + rng.uniform(-0.15, 0.15, size=(n, 8, 3))) * 0.5
    xi = rng.uniform(-0.9, 0.9, size=(n, 3))
    axis = rng.integers(0, 3, size=n)
    eps = rng.choice([0.0, 1e-15, -1e-15, 1e-13, -1e-13, 1e-10, -1e-10, 1e-7, -1e-7], size=n)
    xi[np.arange(n), axis] = rng.choice([-1.0, 1.0], size=n) * (1.025 + eps)
    N = 0.125 * (1 + RST[None, :, 0] * xi[:, None, 0]) * (1 + RST[None, :, 1] * xi[:, None, 1]) * (1 + RST[None, :, 2] * xi[:, None, 2])
    pnt = np.ascontiguousarray(np.einsum("np,npj->nj", N, vtx))
    st = fast_stats(host, pnt, np.ascontiguousarray(vtx))
    assert st["wrong"] == 0 and st["tripdiff"] == 0, st
    assert st["unsure"] > 0.1 * n and st["accept"] > 0.2 * n and st["reject"] > 0.2 * n, st


def test_fast_solve_degenerate_inputs_are_unsure_or_right(host):
    flat = RST.copy()
    flat[:, 2] = 0.0
    cube = RST.copy()
    pnts, vtxs = [], []
    for vtx, pnt in [(flat, [0.1, 0.2, 0.0]), (cube, [0.0, 0.0, 0.0]), (cube, [1.0, 1.0, 1.0]), (cube * 0.0, [0.0, 0.0, 0.0]),
                     (cube, [np.nan, 0.0, 0.0]), (cube * 1e-200, [1e-201, 0, 0]), (cube * 1e150, [1e149, 0, 0]),
                     (cube + 1e12, [1e12, 1e12, 1e12])]:
        pnts.append(pnt)
        vtxs.append(vtx)
    st = fast_stats(host, np.ascontiguousarray(pnts, float), np.ascontiguousarray(vtxs, float))
    assert st["wrong"] == 0 and st["tripdiff"] == 0, st


def test_fast_weights_agree_with_the_reference_polynomials(host):
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags=["C_CONTIGUOUS"])
    host.nh_fast_weights.restype = C.c_double
    host.nh_fast_weights.argtypes = [C.c_int64, f64p, C.c_void_p]
    xi = np.random.default_rng(2).uniform(-1.03, 1.03, size=(200_000, 3))
    worst = host.nh_fast_weights(len(xi), xi, C.cast(O.lib().mmo_hex8_weights, C.c_void_p))
    assert worst < 4e-16
