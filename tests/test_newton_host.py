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


# ----------------------------------------------------------------------------------------------------------------------
# Thin elements (Earth meshes' radial layers: 10 to 1e4 times wider than tall), near the origin and at Earth and UTM
# coordinates -- after make_spherical every coordinate is in metres at |x| ~ 6.4e6
# ----------------------------------------------------------------------------------------------------------------------
def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def slabs(rng, n, aspect, kind, width, offset, spread=0.6):
    """n hexahedra `width` wide and width / aspect thick (the t axis), with one point each at `spread` reference units
    (normal) around the centre.  kind: "plain" -- axis-aligned, corners jittered by 2 % of each extent; "sheared" -- an
    affine shear (the slab tilted by up to ~27 degrees against its own plane, the plane skewed), then a random rotation;
    "warped" -- non-affine: corners jittered by 25 % of each extent, both faces bent like a shell, then a random rotation."""
    ext = np.array([1.0, 1.0, 1.0 / aspect]) * (0.5 * width)
    jit = {"plain": 0.02, "sheared": 0.02, "warped": 0.25}[kind]
    ref = RST[None] + rng.uniform(-jit, jit, size=(n, 8, 3))
    if kind == "warped":
        ref[:, :, 2] += rng.uniform(-0.5, 0.5, size=(n, 1)) * (ref[:, :, 0] ** 2 + ref[:, :, 1] ** 2)
    pnt_ref = rng.normal(scale=spread, size=(n, 3))
    vtx, pnt = ref * ext, pnt_ref * ext
    if kind != "plain":
        if kind == "sheared":
            a, b, c = rng.uniform(-0.5, 0.5, size=(3, n, 1))
            vtx = np.stack([vtx[..., 0] + c * vtx[..., 1], vtx[..., 1], vtx[..., 2] + a * vtx[..., 0] + b * vtx[..., 1]], -1)
            pnt = np.stack([pnt[:, 0] + c[:, 0] * pnt[:, 1], pnt[:, 1],
                            pnt[:, 2] + a[:, 0] * pnt[:, 0] + b[:, 0] * pnt[:, 1]], -1)
        rot = rotations(rng, n)
        vtx = np.einsum("nij,npj->npi", rot, vtx)
        pnt = np.einsum("nij,nj->ni", rot, pnt)
    off = np.asarray(offset, float)
    return np.ascontiguousarray(pnt + vtx.mean(1) + off), np.ascontiguousarray(vtx + off)


THIN_ASPECTS = (10, 100, 300, 1000, 10_000)
THIN_KINDS = ("plain", "sheared", "warped")
EARTH = tuple(6.4e6 * np.array([0.36, -0.48, 0.8]))                                 # |x| = 6.4e6 m
THIN_PLACES = {
    "origin": ((0.0, 0.0, 0.0), 1.0),            # unit width
    "earth": (EARTH, 1000.0),                    # 1 km wide: 1 km x 100 m at aspect 10
    "crust": (EARTH, 1e5),                       # 100 km wide: global-mesh crust and mantle elements
    "mantle": (EARTH, 3e5),                      # 300 km wide
    "utm": ((4.5e5, 5.0e6, 1.2e3), 1.0),         # UTM-like metres, 1 m wide
}
THIN_SOLVES = 20_000


def fast_weight_ratio(host, pnt, vtx, cap=6):
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags=["C_CONTIGUOUS"])
    host.nh_fast_weight_ratio.restype = C.c_double
    host.nh_fast_weight_ratio.argtypes = [C.c_int64, f64p, f64p, C.c_void_p, C.c_void_p, C.c_int, f64p]
    out = np.zeros(4)
    L = O.lib()
    ratio = host.nh_fast_weight_ratio(len(pnt), pnt, vtx, C.cast(L.mmo_hex8_newton, C.c_void_p),
                                      C.cast(L.mmo_hex8_weights, C.c_void_p), cap, out)
    return ratio, int(out[0]), out[1], out[3]


# measured with cap 6 (not asserted: raising them is performance work), per aspect 10 / 100 / 300 / 1000 / 1e4
#   certified share          origin  plain 1.00 / 0.25 / 0.23 / 0.24 / 0     warped 1.00 / 0.78 / 0.25 / 0.24 / 0.09
#                            crust   plain 0.99 / 0.91 / 0.33 / 0    / 0     warped 0.99 / 0.26 / 0.20 / 0    / 0
#                            mantle  plain 1.00 / 0.96 / 0.41 / 0.15 / 0     warped 0.99 / 0.27 / 0.24 / 0.15 / 0
#                            earth, utm: 0 for every kind and aspect -- the residual band rho exceeds the reference's
#                            tolerance 1e-8 |x1 - x0|, so every solve goes back to the reference's arithmetic (the GPU's
#                            saturated tier-1 queue, tests/test_thin_elements_gpu.py)
#   weight error / bound     <= 0.064 over every certified accept (mantle warped, aspect 300); with a cap fitted at 1024
#                            instead of the derived 64 it reached 0.83 (crust warped, aspect 500), and without any cap 2.2
#   |xi - xi_ref| / delta    <= 1 / 300 on the certified accepts
THIN_FAMILIES = [(p, k, a) for p in THIN_PLACES for k in THIN_KINDS for a in THIN_ASPECTS]


def thin_family(place, kind, aspect):
    rng = np.random.default_rng([list(THIN_PLACES).index(place), THIN_KINDS.index(kind), aspect])
    offset, width = THIN_PLACES[place]
    return slabs(rng, THIN_SOLVES, aspect, kind, width, offset)


@pytest.mark.parametrize("place", list(THIN_PLACES))
def test_thin_elements_final_iterates_equal_the_oracle(host, place):
    fn = O.lib().mmo_hex8_newton
    for kind in THIN_KINDS:
        for aspect in THIN_ASPECTS:
            pnt, vtx = thin_family(place, kind, aspect)
            for staged, c1, c2 in ((0, 6, 9), (1, 6, 9), (1, 1, 3), (1, 2, 7)):
                bad, first, conv = compare(host, fn, 0, pnt, vtx, staged, c1, c2)
                assert bad == 0, (place, kind, aspect, staged, c1, c2, first)
            assert conv > 0.5 * len(pnt), (place, kind, aspect, conv)


@pytest.mark.parametrize("place", list(THIN_PLACES))
def test_thin_elements_fast_solve_never_certifies_a_wrong_verdict(host, place):
    for kind in THIN_KINDS:
        for aspect in THIN_ASPECTS:
            pnt, vtx = thin_family(place, kind, aspect)
            for cap in (6, 9):
                st = fast_stats(host, pnt, vtx, cap)
                assert st["wrong"] == 0 and st["tripdiff"] == 0, (place, kind, aspect, cap, st)
                assert st["worst_over_delta"] < 0.25, (place, kind, aspect, cap, st)


# (the places where the fast solve certifies accepts; at "earth" and "utm" it certifies none, see above)
@pytest.mark.parametrize("place", ["origin", "crust", "mantle"])
def test_thin_elements_fast_weights_within_the_stated_bound(host, place):
    # MM_FP_TOL's contract: every certified accept's weights (weights_hex8_fast of the fast iterate) within
    # max(1e-12, 64 eps max|x| / shortest edge) of the reference's (mmo_hex8_weights of the reference iterate); and the
    # error model kFastWcap is derived from (csrc/mm_newton_hex8.h): |xi - xi_ref| <= delta / 128 on every certified accept
    thin_accepts = 0
    for kind in THIN_KINDS:
        for aspect in THIN_ASPECTS:
            pnt, vtx = thin_family(place, kind, aspect)
            for cap in (6, 9):
                ratio, naccept, worst, xi_over_delta = fast_weight_ratio(host, pnt, vtx, cap)
                assert ratio <= 1.0, (place, kind, aspect, cap, ratio, naccept, worst)
                assert xi_over_delta <= 1 / 128, (place, kind, aspect, cap, xi_over_delta)
                # ... and the derivation's own prediction with the measured |xi - xi_ref| <= delta / 300:
                # 1.58 x kFastWcap / 300 = 0.34 of the bound (a cap fitted loosely, 1024, reaches 0.7 here)
                assert ratio <= 0.34, (place, kind, aspect, cap, ratio, naccept, worst)
                if aspect == 10:
                    assert naccept > 0.2 * len(pnt), (place, kind, aspect, cap, naccept)   # the check has work to do
                thin_accepts = thin_accepts + naccept if aspect >= 100 else thin_accepts
    assert thin_accepts > 0.01 * THIN_SOLVES, (place, thin_accepts)                          # ... also on thin slabs


@pytest.mark.parametrize("case", range(len(CASES)))
def test_fast_weights_within_the_stated_bound(host, case):
    # the same contract on the near-cubic families above (measured: <= 0.03 of the bound)
    jitter, scale, offset, spread = CASES[case]
    pnt, vtx = elements(np.random.default_rng(41000 + case), 200_000, jitter, scale, offset, spread)
    ratio, naccept, worst, xi_over_delta = fast_weight_ratio(host, pnt, vtx)
    assert ratio <= 1.0 and xi_over_delta <= 1 / 128, (case, ratio, naccept, worst, xi_over_delta)
    if case in (0, 2, 3):
        assert naccept > 0.3 * len(pnt)


def documented_band(pnt, vtx):
    """The reference's tolerance and the residual band rho csrc/mm_newton_hex8.h documents, restated here from its
    formulas (at xi = 0, in the coordinates' units): tol = 1e-8 max|corner 1 - corner 0|, rho = 64 eps |v| + 3 |J| delta
    with delta = 256 eps |v| |J^-1|; J, |v| and |J^-1| as the header bounds them (rows of 8 J, 8 x the coordinates,
    3 max|cofactor| / |det|)."""
    eps = np.finfo(np.float64).eps
    rows = [np.einsum("p,npj->nj", RST[:, a], vtx) for a in range(3)]          # rows of 8 J
    cof = np.concatenate([np.cross(rows[1], rows[2]), np.cross(rows[2], rows[0]), np.cross(rows[0], rows[1])], axis=1)
    det = np.einsum("nj,nj->n", rows[0], np.cross(rows[1], rows[2]))
    jmax = np.abs(np.concatenate(rows, axis=1)).max(1)
    v8 = 4 * jmax + np.maximum(np.abs(vtx.sum(1)).max(1), 8 * np.abs(pnt).max(1))
    delta = 256 * eps * v8 * 3 * np.abs(cof).max(1) / np.abs(det)
    rho = (3 * jmax * delta + 64 * eps * v8) / 8
    return 1e-8 * np.abs(vtx[:, 1] - vtx[:, 0]).max(1), rho


@pytest.mark.parametrize("scale,offset", [(1.0, (0.0, 0.0, 0.0)), (1.0, (30.0, -20.0, 50.0)), (29.5e3, (3.1e6, -2.2e6, 5.0e6))])
def test_fast_solve_is_unsure_inside_the_residual_band(host, scale, offset):
    # the first residual test (xi = 0: the point minus the centroid) placed at tol + u rho, u uniform in [-2, 2], in x (y
    # well inside tol): inside the documented band (|u| < 1) the verdict must be "unsure", outside it certified and right.
    # A narrower band -- kFastCres shrunk, or the 3 |J| delta term dropped -- certifies solves inside it.
    rng = np.random.default_rng(8)
    n = 50_000
    _, vtx = elements(rng, n, 0.1, scale, offset, 0.0)
    c = vtx.mean(1)
    tol, rho = documented_band(c, vtx)
    keep = rho < 0.6 * tol                    # the y residual, 0.3 tol, stays below tol - rho
    assert keep.mean() > 0.9 and (rho > 1e3 * np.spacing(np.abs(c).max(1))).all()
    vtx, c, tol, rho = np.ascontiguousarray(vtx[keep]), c[keep], tol[keep], rho[keep]
    n = len(c)
    sx, sy = rng.choice([-1.0, 1.0], size=(2, n))
    pnt = c.copy()
    pnt[:, 0] += sx * (tol + rng.uniform(-2.0, 2.0, n) * rho)
    pnt[:, 1] += sy * 0.3 * tol
    pnt = np.ascontiguousarray(pnt)
    tol, rho = documented_band(pnt, vtx)
    u = (np.abs(pnt[:, 0] - c[:, 0]) - tol) / rho                              # where the point really landed
    verdict = np.zeros(n, np.int8)
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags=["C_CONTIGUOUS"])
    host.nh_fast_verdicts.restype = None
    host.nh_fast_verdicts.argtypes = [C.c_int64, f64p, f64p, C.c_int, np.ctypeslib.ndpointer(dtype=np.int8)]
    host.nh_fast_verdicts(n, pnt, vtx, 6, verdict)
    inside = np.abs(u) < 0.995
    assert inside.sum() > 0.4 * n and (~inside).sum() > 0.4 * n
    assert (verdict[inside] == 2).all(), (np.flatnonzero(inside & (verdict != 2))[:5], u[inside & (verdict != 2)][:5])
    st = fast_stats(host, pnt, vtx)
    assert st["wrong"] == 0 and st["tripdiff"] == 0 and st["accept"] > 0.3 * n, st
