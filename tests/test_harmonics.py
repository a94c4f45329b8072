"""Spherical-harmonic models without a GPU: the NumPy statement (tests/harmonic_cases.py) against what it must satisfy -- the
addition theorem, the closed forms of the low degrees, cos k phi and sin k phi --, the extension header against the module's
signature table, the host side of :mod:`multimesh_amd.harmonics` (conventions, packing, the radial basis, truncation) and the
argument errors that are decided before the device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import harmonic_cases as HC
from multimesh_amd import harmonics as H
from multimesh_amd import helpers
from test_parametrisation import _c_class, _ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multimesh_harmonics.h")
L40 = 40


@pytest.fixture(scope="module")
def sphere():
    """2000 directions, both poles among them: (ct, st, cp, sp, P at L = 40)."""
    pts = HC.directions(2000, seed=5)
    pts[0], pts[1] = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    ct, st, cp, sp = HC.direction(pts)
    return pts, ct, st, cp, sp, HC.legendre(ct, st, L40)


# ------------------------------------------------------------------------------------------------------- the statement
def test_addition_theorem(sphere):
    """sum_k P_lk^2 = 2 l + 1 for the 4-pi-normalised functions (the orders k >= 1 carry their factor 2 in P_lk)."""
    _, _, _, _, _, P = sphere
    worst = 0.0
    for l in range(L40 + 1):
        total = sum(P[HC.idx(l, k, L40)] ** 2 for k in range(l + 1))
        worst = max(worst, np.abs(total - (2 * l + 1)).max())
    print(f"largest |sum_k P_lk^2 - (2l + 1)| at L = {L40}: {worst:.3e}")
    assert worst <= 1e-10


def test_closed_forms_of_the_low_degrees(sphere):
    _, ct, st, _, _, _ = sphere
    P = HC.legendre(ct, st, 2)
    want = {(0, 0): np.ones_like(ct), (1, 0): np.sqrt(3.0) * ct, (1, 1): np.sqrt(3.0) * st,
            (2, 0): np.sqrt(5.0) * (1.5 * ct * ct - 0.5), (2, 1): np.sqrt(15.0) * ct * st,
            (2, 2): 0.5 * np.sqrt(15.0) * st * st}
    for (l, k), w in want.items():
        err = np.abs(P[HC.idx(l, k, 2)] - w).max()
        assert err <= 8 * np.finfo(float).eps * np.sqrt(5.0) * 1.5, (l, k, err)   # (a handful of roundings of values <= 3.4)


def test_fourier_factors(sphere):
    pts, _, _, cp, sp, _ = sphere
    Ck, Sk = HC.fourier(cp, sp, L40)
    phi = np.arctan2(pts[:, 1], pts[:, 0])
    k = np.arange(L40 + 1)[:, None]
    err = max(np.abs(Ck - np.cos(k * phi)).max(), np.abs(Sk - np.sin(k * phi)).max())
    print(f"largest error of C_k, S_k at L = {L40}: {err:.3e}")
    assert err <= 1e-13
    assert np.array_equal(Ck[0], np.ones_like(cp)) and np.array_equal(Sk[0], np.zeros_like(cp))
    assert np.array_equal(Ck[1, :2], [1.0, 1.0]) and np.array_equal(Sk[1, :2], [0.0, 0.0])   # the poles: longitude 0


def test_special_directions():
    ct, st, cp, sp = HC.direction([[0, 0, 0], [0, 0, 2], [0, 0, -3], [5, 0, 0], [0, -4, 0]])
    assert list(ct) == [0, 1, -1, 0, 0] and list(st) == [1, 0, 0, 1, 1]
    assert list(cp) == [1, 1, 1, 1, 0] and list(sp) == [0, 0, 0, 0, -1]


def test_a_zonal_degree_two_model_is_its_closed_form():
    """The whole statement on a model with one coefficient: s = lerp of c_20(r) * P_20(cos theta)."""
    R = np.array([1.0, 2.0, 4.0])
    coef = np.zeros((1, 3, 2, HC.nlm(3)))
    coef[0, :, 0, HC.idx(2, 0, 3)] = [1.0, 3.0, -1.0]
    pts = HC.directions(50, seed=2) * np.linspace(1.0, 4.0, 50)[:, None]
    out, nout = HC.model_apply(pts, R, coef, 3)
    r = np.sqrt((pts * pts).sum(axis=1))
    c20 = np.interp(r, R, [1.0, 3.0, -1.0])
    want = c20 * np.sqrt(5.0) * (1.5 * (pts[:, 2] / r) ** 2 - 0.5)
    assert nout == 0 and np.abs(out[0] - want).max() <= 1e-14 * 3.0 * np.sqrt(5.0)


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
    assert list(protos) == list(H.SIGNATURES) == ["mm_harmonic_model_apply"]
    lib = H.bind()
    assert lib is helpers.load_lib()
    for name, (ret, params) in protos.items():
        assert hasattr(lib, name), name
        restype, argtypes = H.SIGNATURES[name]
        assert (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes]) == (ret, params), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert name not in helpers.SIGNATURES and name not in helpers.EXPORTED_SYMBOLS
    text = open(HEADER).read()
    assert int(re.search(r"#define MM_HARMONIC_MAX_LMAX (\d+)", text).group(1)) == H.MAX_LMAX
    assert int(re.search(r"#define MM_HARMONIC_MAX_P (\d+)", text).group(1)) == H.MAX_P
    for name, number in H.MODES.items():
        assert int(re.search(rf"#define MM_HARMONIC_{name.upper()} (\d+)", text).group(1)) == number


# ------------------------------------------------------------------------------------------------- the host side of the module
def _square(L, m, seed):
    """(cos, sin) f64[m, L+1, L+1], zero where k > l."""
    rng = np.random.default_rng(seed)
    mask = np.tril(np.ones((L + 1, L + 1), dtype=bool))
    return np.where(mask, rng.standard_normal((m, L + 1, L + 1)), 0.0), np.where(mask, rng.standard_normal((m, L + 1, L + 1)), 0.0)


def test_packing_follows_idx():
    L, m = 6, 3
    cos, sin = _square(L, m, 1)
    packed = H.pack_coefficients(cos, sin, L)
    assert packed.shape == (m, 2, HC.nlm(L)) == (m, 2, H.coefficient_count(L))
    seen = set()
    for l in range(L + 1):
        for k in range(l + 1):
            q = HC.idx(l, k, L)
            assert q == H.coefficient_index(l, k, L)
            seen.add(q)
            assert np.array_equal(packed[:, 0, q], cos[:, l, k]) and np.array_equal(packed[:, 1, q], sin[:, l, k])
    assert seen == set(range(HC.nlm(L)))
    back = H.unpack_coefficients(packed, L)
    assert np.array_equal(back[0], cos) and np.array_equal(back[1], sin)
    # the degrees of one order are contiguous, the order is the major index
    assert [HC.idx(l, 2, L) for l in range(2, L + 1)] == list(range(HC.idx(2, 2, L), HC.idx(2, 2, L) + L - 1))


@pytest.mark.parametrize("norm", H.NORMALIZATIONS)
@pytest.mark.parametrize("phase", [1, -1])
def test_conventions_round_trip(norm, phase):
    L = 9
    cos, sin = _square(L, 2, 3)
    there = H.convert_coefficients(cos, sin, L, frm=(norm, phase), to=("4pi", 1))
    back = H.convert_coefficients(*there, L, frm=("4pi", 1), to=(norm, phase))
    for a, b in zip(back, (cos, sin)):
        assert (np.abs(a - b) <= 4 * 2.0 ** -53 * np.abs(b)).all()       # two roundings each way
    l = np.arange(L + 1)[:, None]
    k = np.arange(L + 1)[None, :]
    scale = {"4pi": 1.0, "ortho": 1.0 / np.sqrt(4 * np.pi), "schmidt": 1.0 / np.sqrt(2.0 * l + 1.0)}[norm]
    sign = np.where(k % 2 == 1, phase, 1.0)
    assert np.allclose(there[0], cos * scale * sign, rtol=1e-15, atol=0) and np.allclose(there[1], sin * scale * sign, rtol=1e-15, atol=0)
    if norm == "4pi":                                                    # a change of phase alone is exact
        assert np.array_equal(there[0], cos * sign) and np.array_equal(back[0], cos)


def test_the_ortho_convention_is_orthonormal():
    """One "ortho" coefficient c_lk with the phase gives the function c (-1)^k Y_lk / sqrt(4 pi) in the device's terms: its
    mean square over the sphere is c^2 / (4 pi)."""
    L = 4
    cos, sin = np.zeros((2, L + 1, L + 1)), np.zeros((2, L + 1, L + 1))
    cos[:, 3, 1] = 2.0
    model = H.SphericalHarmonicModel(L, [1.0, 2.0], {"f": (cos, sin)}, normalization="ortho", csphase=-1)
    assert model.cos["f"][0, 3, 1] == -2.0 / np.sqrt(4 * np.pi)
    _, coef = model.packed()
    pts = HC.directions(20000, seed=9) * 1.5
    out, _ = HC.model_apply(pts, model.radii, coef, L)
    assert abs((out[0] ** 2).mean() * 4 * np.pi - 4.0) < 0.15           # (Monte Carlo: 3 sigma is about 0.1)


def test_from_radial_basis_with_an_identity_basis():
    L, m = 5, 4
    cos, sin = _square(L, m, 7)
    radii = [1.0, 2.0, 2.0, 3.0]
    model = H.SphericalHarmonicModel.from_radial_basis(L, np.eye(m), radii, {"dvs": (cos, sin)})
    assert np.array_equal(model.cos["dvs"], cos) and np.array_equal(model.sin["dvs"], sin)
    assert model.layers == [(0, 1), (2, 3)] and model.parameters == ["dvs"]
    two = H.SphericalHarmonicModel.from_radial_basis(L, [[1.0, 0.5, 0.5, 0.0], [0.0, 0.5, 0.5, 1.0]], radii,
                                                     {"dvs": (cos[:2], sin[:2])})
    assert np.allclose(two.cos["dvs"][1], 0.5 * cos[0] + 0.5 * cos[1], rtol=1e-15)
    with pytest.raises(ValueError, match=r"basis must be \[K, m\]"):
        H.SphericalHarmonicModel.from_radial_basis(L, np.eye(3), radii, {"dvs": (cos, sin)})


def test_truncate_drops_the_higher_degrees():
    L, m = 8, 3
    cos, sin = _square(L, m, 11)
    model = H.SphericalHarmonicModel(L, [1.0, 2.0, 3.0], {"a": (cos, sin), "b": (sin, cos)})
    low = model.truncate(3)
    assert low.lmax == 3 and low.parameters == ["a", "b"]
    names, packed = low.packed(["b"])
    assert names == ["b"] and packed.shape == (1, m, 2, HC.nlm(3))
    assert np.array_equal(packed[0], H.pack_coefficients(sin[:, :4, :4], cos[:, :4, :4], 3))
    # the truncated model is the model with its higher coefficients set to zero
    pts = HC.cloud(40, seed=3, r_lo=1.0, r_hi=3.0)
    zeroed = model.packed(["a"])[1].copy()
    for l in range(4, L + 1):
        for k in range(l + 1):
            zeroed[..., HC.idx(l, k, L)] = 0.0
    want, _ = HC.model_apply(pts, model.radii, zeroed, L)
    got, _ = HC.model_apply(pts, low.radii, low.packed(["a"])[1], 3)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    with pytest.raises(ValueError, match="cannot truncate"):
        model.truncate(9)


def test_what_the_model_refuses():
    cos, sin = _square(2, 3, 1)
    ok = {"a": (cos, sin)}
    with pytest.raises(ValueError, match="lmax must be an integer"):
        H.SphericalHarmonicModel(256, [1.0, 2.0, 3.0], ok)
    with pytest.raises(ValueError, match="lmax must be an integer"):
        H.SphericalHarmonicModel(-1, [1.0, 2.0, 3.0], ok)
    with pytest.raises(ValueError, match="descend"):
        H.SphericalHarmonicModel(2, [1.0, 3.0, 2.0], ok)
    with pytest.raises(ValueError, match="single row"):
        H.SphericalHarmonicModel(2, [1.0, 1.0, 2.0], ok)
    with pytest.raises(ValueError, match=r"must be two arrays \(3, 3, 3\)"):
        H.SphericalHarmonicModel(2, [1.0, 2.0, 3.0], {"a": (cos[:2], sin[:2])})
    with pytest.raises(ValueError, match="normalization must be one of"):
        H.SphericalHarmonicModel(2, [1.0, 2.0, 3.0], ok, normalization="unnorm")
    with pytest.raises(ValueError, match="csphase must be"):
        H.SphericalHarmonicModel(2, [1.0, 2.0, 3.0], ok, csphase=0)
    model = H.SphericalHarmonicModel(2, [1.0, 2.0, 3.0], ok)
    with pytest.raises(ValueError, match=r"has no \['b'\]"):
        model.packed(["b"])
    with pytest.raises(ValueError, match="mode must be one of"):
        H.import_harmonic_model(model, None, mode="multiply")


# --------------------------------------------------------------------------------------------------- argument checks
CTX = C.c_void_p(0x1000)            # a dummy: a refused call never looks at the context
PTS, RAD, COEF, IN, OUT = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000, 0x500000))   # never read either


def _call(lib, ctx=CTX, pts=PTS, ngroups=10, P_=8, rad=RAD, m=5, lmax=4, coef=COEF, ncomp=2, mode=0, extend=0, src=IN,
          dst=OUT, count=None):
    return lib.mm_harmonic_model_apply(ctx, pts, ngroups, P_, rad, m, lmax, coef, ncomp, mode, extend, src, dst, count)


#: every MM_ERR_ARG case of the header that is decided before the device is touched (the table's own cases need its radii:
#: tests/test_harmonics_gpu.py)
REFUSED = {
    "null ctx": dict(ctx=None),
    "negative ngroups": dict(ngroups=-1),
    "ngroups at 2^48": dict(ngroups=1 << 48),
    "P zero": dict(P_=0),
    "P above 256": dict(P_=257),
    "m one": dict(m=1),
    "m at 2^24": dict(m=1 << 24),
    "lmax negative": dict(lmax=-1),
    "lmax above 255": dict(lmax=256),
    "ncomp negative": dict(ncomp=-1),
    "ncomp at 65536": dict(ncomp=65536),
    "mode negative": dict(mode=-1),
    "mode three": dict(mode=3),
    "extend two": dict(extend=2),
    "extend negative": dict(extend=-1),
    "null radius": dict(rad=None),
    "null coef": dict(coef=None),
    "values at 2^48": dict(ngroups=1 << 44, P_=8, ncomp=2),
    "coef at 2^48": dict(m=(1 << 24) - 1, lmax=255, ncomp=256),
    "null points": dict(pts=None),
    "null out": dict(dst=None),
    "null in, mode 1": dict(mode=1, src=None),
    "null in, mode 2": dict(mode=2, src=None),
}


def test_the_extent_cases_sit_on_the_limit():
    assert 2 * (1 << 44) * 8 == 1 << 48
    assert 256 * ((1 << 24) - 1) * 2 * HC.nlm(255) >= 1 << 48 > 128 * ((1 << 24) - 1) * 2 * HC.nlm(255)


@pytest.mark.parametrize("what", list(REFUSED))
def test_refuses_without_a_gpu(what):
    lib = H.bind()
    assert _call(lib, **REFUSED[what]) == -1, what
    message = lib.mm_last_error()
    assert b"mm_harmonic_model_apply" in message and len(message) > len(b"mm_harmonic_model_apply: "), message
    assert lib.mm_last_status() == -1


def test_python_refuses_before_the_library_is_asked():
    class NoDevice:                      # the checks below come before anything of the context is used
        lib = None

    with pytest.raises(ValueError, match="lmax must be an integer"):
        H.harmonic_model_apply(NoDevice(), np.zeros((4, 3)), [1.0, 2.0], np.zeros((1, 2, 2, 1)), 300)
    with pytest.raises(ValueError, match="lmax must be an integer"):
        H.harmonic_model_apply(NoDevice(), np.zeros((4, 3)), [1.0, 2.0], np.zeros((1, 2, 2, 1)), 2.5)
