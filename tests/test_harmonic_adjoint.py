"""The transpose of the spherical-harmonic evaluation without a GPU: the NumPy statement (tests/harmonic_adjoint_cases.py)
against a dense matrix built from the forward statement, the header against the module's table, the conventions, the CGLS
recurrence against ``np.linalg.lstsq``, and the power per degree."""
import re

import numpy as np
import pytest

import harmonic_adjoint_cases as AC
import harmonic_cases as HC
import test_harmonics as TH
from multimesh_amd import harmonic_adjoint as A
from multimesh_amd import harmonics as H
from multimesh_amd import helpers

HEADER = TH.HEADER.replace("multimesh_harmonics.h", "multimesh_harmonic_adjoint.h")
U = 2.0 ** -53

#: |c_CGLS - c_lstsq| / |c_lstsq| of the 2000-point case below (rtol = 1e-12), both in NumPy: 7.8e-13 unweighted, 5.9e-13
#: weighted, 9.5e-13 damped were measured; ten times the largest, rounded.  The GPU fit is held to the same number
#: (tests/test_harmonic_adjoint_gpu.py).
FIT_TOLERANCE = 1.0e-11


def gamma(N):
    return N * U / (1.0 - N * U)


def fit_case():
    """The 2000-point global cover: (points, radii, f, weights), L = 3, m = 3: 60 unknowns."""
    pts, R = AC.shell_cloud(2000, seed=11, m=3)
    rng = np.random.default_rng(12)
    truth = HC.coefficients(3, 3, 1, seed=13)
    f = HC.model_apply(pts, R, truth, 3)[0][0] + 1e-3 * rng.standard_normal(2000)
    return pts, R, f, rng.uniform(0.5, 2.0, 2000)


# ------------------------------------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("weighted", (False, True))
def test_the_statement_is_the_transpose_of_the_dense_matrix(weighted):
    """H from the forward statement on unit coefficients (300 points in elements of 3 nodes and a cloud part, L = 3, m = 5
    with the 670), H^T g in extended precision against the statement.  The bound is derived: an entry of H carries 2
    roundings beyond fl(1 - t), a term of the statement 3 (4 with a weight), a sum over the n nodes n more, the segment sum
    and Lo + Hi 2: N = n + 12 rounded operations cover the longest path of the difference, so every entry agrees within
    gamma_N (|H|^T |g|), gamma_N = N u / (1 - N u)."""
    L, R = 3, HC.knots(5)
    pts = HC.elements(100, 3, seed=1, size=3e5, r_lo=HC.R_CMB - 2e5, r_hi=HC.R_MOHO + 2e5)
    n = 300
    rng = np.random.default_rng(2)
    g = rng.standard_normal(n)
    w = rng.uniform(0.5, 2.0, n) if weighted else None
    for extend in (False, True):
        Hd = AC.dense_matrix(pts, R, L, extend=extend)
        assert Hd.shape == (n, 5 * 2 * HC.nlm(L))
        wg = (g if w is None else w.astype(np.longdouble) * g).astype(np.longdouble)
        want = Hd.astype(np.longdouble).T @ wg
        bound = gamma(n + 12) * (np.abs(Hd).astype(np.longdouble).T @ np.abs(wg))
        got, nout = AC.model_transpose(pts, R, L, g[None, :], weight=w, extend=extend)
        err = np.abs(got.reshape(-1).astype(np.longdouble) - want)
        print(f"extend {extend}: largest error / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}, {nout} nodes outside")
        assert (err <= bound).all()
        assert (nout > 0) != extend and nout == HC.model_apply(pts, R, np.zeros((1, 5, 2, HC.nlm(L))), L, extend=extend)[1]
        assert not (np.signbit(got) & (got == 0.0)).any()                              # no output is -0.0


def test_segments_split_the_sums_and_nothing_else():
    """65 elements of P = 256 are two segments (Gs = 64): the statement equals the sum of the statements of the two parts
    (each a single segment)."""
    L, R = 1, HC.knots(4, discontinuity=False)
    pts = HC.elements(65, 256, seed=3, size=2e5)
    g = np.random.default_rng(4).standard_normal((1, 65 * 256))
    whole, _ = AC.model_transpose(pts, R, L, g, extend=True)
    first, _ = AC.model_transpose(pts[:64], R, L, g[:, :64 * 256], extend=True)
    second, _ = AC.model_transpose(pts[64:], R, L, g[:, 64 * 256:], extend=True)
    # (Lo_j + Hi_{j-1} is formed after the segments are added: compare the parts that a single side reaches)
    assert HC.same_bits_nan(whole[:, 0], first[:, 0] + second[:, 0])        # row 0: Lo alone
    assert HC.same_bits_nan(whole[:, -1], first[:, -1] + second[:, -1])     # the last row: Hi alone


# ----------------------------------------------------------------------------------------------- the header and the table
def test_the_extension_header_and_the_table_agree(monkeypatch):
    monkeypatch.setattr(TH, "HEADER", HEADER)
    protos = TH._declared_prototypes()
    assert list(protos) == list(A.SIGNATURES) == ["mm_harmonic_model_transpose"]
    lib = A.bind()
    assert lib is helpers.load_lib()
    for name, (ret, params) in protos.items():
        assert hasattr(lib, name), name
        restype, argtypes = A.SIGNATURES[name]
        assert (TH._ctypes_class(restype), [TH._ctypes_class(t) for t in argtypes]) == (ret, params), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert name not in helpers.SIGNATURES and name not in helpers.EXPORTED_SYMBOLS and name not in H.SIGNATURES
    text = open(HEADER).read()
    assert int(re.search(r"#define MM_HARMONIC_SEGMENT_NODES (\d+)", text).group(1)) == A.SEGMENT_NODES == AC.SEGMENT_NODES
    assert '#include "multimesh_harmonics.h"' in text


# ---------------------------------------------------------------------------------------------------------- conventions
@pytest.mark.parametrize("norm", ("ortho", "schmidt"))
@pytest.mark.parametrize("phase", (1, -1))
def test_the_gradient_takes_the_factor_of_the_coefficients(norm, phase):
    """<H c, g> = <c_user, s o H^T g> with c_device = s o c_user: the gradient with respect to the user's coefficients is
    scaled by the same factor as the coefficients, as harmonic_adjoint does it."""
    L, R = 4, HC.knots(5)
    rng = np.random.default_rng(7)
    mask = np.tril(np.ones((L + 1, L + 1), dtype=bool))
    cos_u, sin_u = (np.where(mask, rng.standard_normal((R.size, L + 1, L + 1)), 0.0) for _ in range(2))
    sin_u[:, :, 0] = 0.0
    cos_d, sin_d = H.convert_coefficients(cos_u, sin_u, L, frm=(norm, phase))
    pts = HC.elements(40, 5, seed=8, size=2e5)
    g = rng.standard_normal(200)
    f = HC.model_apply(pts, R, H.pack_coefficients(cos_d, sin_d, L)[None], L, extend=True)[0][0]
    grad, _ = AC.model_transpose(pts, R, L, g[None, :], extend=True)
    gc, gs = H.unpack_coefficients(grad[0], L)
    s = H._factors(L, norm, phase)
    lhs, rhs = f @ g, (cos_u * (s * gc)).sum() + (sin_u * (s * gs)).sum()
    scale = np.abs(f) @ np.abs(g)
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)
    wrong = (cos_u * (gc / s)).sum() + (sin_u * (gs / s)).sum()
    assert abs(lhs - wrong) > 1e-3 * scale                                   # (the inverse factor is not the gradient)


# ----------------------------------------------------------------------------------------------------------------- CGLS
@pytest.mark.parametrize("weighted,damping", ((False, 0.0), (True, 0.0), (True, 50.0)))
def test_cgls_against_lstsq(weighted, damping):
    pts, R, f, w = fit_case()
    w = w if weighted else np.ones_like(w)
    Hd = AC.dense_matrix(pts, R, 3, extend=True)
    assert Hd.shape == (2000, 60)
    rows = [np.sqrt(w)[:, None] * Hd] + ([np.sqrt(damping) * np.eye(60)] if damping else [])
    rhs = [np.sqrt(w) * f] + ([np.zeros(60)] if damping else [])
    want = np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0]
    got, iterations, residual = AC.cgls(Hd, f, w, damping=damping, rtol=1e-12, max_iter=200)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"weighted {weighted}, damping {damping}: {iterations} iterations, residual {residual:.2e}, |c - lstsq| / |lstsq| {err:.2e}")
    assert residual <= 1e-12 and iterations < 200 and err <= FIT_TOLERANCE
    assert (got.reshape(3, 2, 10)[:, 1, :4] == 0.0).all()                    # the sine plane at k = 0 stays zero


# ---------------------------------------------------------------------------------------------------------- degree_power
def test_degree_power():
    L, m = 5, 3
    cos, sin = np.zeros((m, L + 1, L + 1)), np.zeros((m, L + 1, L + 1))
    for l in range(L + 1):
        cos[:, l, l // 2] = [l + 1.0, 2.0, 0.0]
        if l:
            sin[1, l, l] = 3.0
    model = H.SphericalHarmonicModel(L, [1.0, 2.0, 3.0], {"VS": (cos, sin)})
    power = A.degree_power(model)["VS"]
    assert power.shape == (m, L + 1)
    assert np.array_equal(power[0], [(l + 1.0) ** 2 for l in range(L + 1)])
    assert np.array_equal(power[1], [4.0] + [13.0] * L) and np.array_equal(power[2], np.zeros(L + 1))
    # the convention is the 4-pi one whatever the model was given in
    ortho = H.SphericalHarmonicModel(L, [1.0, 2.0, 3.0], {"VS": (cos * np.sqrt(4 * np.pi), sin * np.sqrt(4 * np.pi))},
                                     normalization="ortho")
    assert np.allclose(A.degree_power(ortho, "VS")["VS"], power, rtol=1e-15, atol=0)
