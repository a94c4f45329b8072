"""Parametrisations without a GPU: the routes, the NumPy statement (tests/parametrisation_cases.py) against itself -- the
there-and-back routes within their derived bound, the transposed Jacobians against difference quotients --, the extension
header against the module's signature table, the argument checks of the two entry points, and ``detect``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parametrisation_cases as PC
from multimesh_amd import helpers, io as mio
from multimesh_amd import parametrisation as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "multimesh_params.h")
SYMBOLS = ("mm_convert_parameters", "mm_convert_kernels")

# the route of every ordered pair as step numbers of the header:
# 1 iso_velocity->iso_lame  2 iso_lame->iso_velocity  3 iso_lame->iso_bulk  4 iso_bulk->iso_lame
# 5 vti_velocity->vti_love  6 vti_love->vti_velocity  7 iso_velocity->vti_velocity  8 vti_love->iso_bulk
V, L, B, T, A = "iso_velocity", "iso_lame", "iso_bulk", "vti_velocity", "vti_love"
ROUTE_TABLE = {
    (V, L): (1,), (V, B): (1, 3), (V, T): (7,), (V, A): (7, 5),
    (L, V): (2,), (L, B): (3,), (L, T): (2, 7), (L, A): (2, 7, 5),
    (B, V): (4, 2), (B, L): (4,), (B, T): (4, 2, 7), (B, A): (4, 2, 7, 5),
    (T, V): (5, 8, 4, 2), (T, L): (5, 8, 4), (T, B): (5, 8), (T, A): (5,),
    (A, V): (8, 4, 2), (A, L): (8, 4), (A, B): (8,), (A, T): (6,),
}
STEP_NAMES = {1: f"{V}->{L}", 2: f"{L}->{V}", 3: f"{L}->{B}", 4: f"{B}->{L}", 5: f"{T}->{A}", 6: f"{A}->{T}", 7: f"{V}->{T}",
              8: f"{A}->{B}"}


# -------------------------------------------------------------------------------------------------------------- routes
def test_the_tables_agree():
    assert list(P.PARAMETRISATIONS) == list(PC.NAMES) == [V, L, B, T, A]
    assert {k: tuple(v) for k, v in P.PARAMETRISATIONS.items()} == PC.COMPONENTS
    assert tuple(P.STEPS) == tuple(PC.STEPS[s] for s in range(1, 9))
    assert PC.ROUTES == ROUTE_TABLE


def test_route_of_all_twenty_pairs():
    pairs = [(a, b) for a in P.PARAMETRISATIONS for b in P.PARAMETRISATIONS if a != b]
    assert len(pairs) == 20 and set(pairs) == set(ROUTE_TABLE)
    for a, b in pairs:
        assert P.route(a, b) == tuple(STEP_NAMES[s] for s in ROUTE_TABLE[a, b]), (a, b)
        assert 1 <= len(P.route(a, b)) <= 4
    assert P.route(V, V) == ()
    with pytest.raises(ValueError, match="unknown parametrisation"):
        P.route(V, "tti")


# ------------------------------------------------------------------------------------------------- the forward statement
N_MODELS = 10_000


def test_embed_is_a_copy_of_the_bits():
    m = PC.models(V, N_MODELS, seed=1)
    out = PC.convert(m, V, T)
    for row, src in zip(out, (0, 0, 1, 1, None, 2)):
        want = np.ones(N_MODELS) if src is None else m[src]
        assert np.array_equal(row.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("a,b", PC.THERE_AND_BACK, ids=lambda x: x)
def test_there_and_back_within_the_derived_bound(a, b):
    """a -> b -> a returns the input: RHO bit for bit, every other component within the bound of the cases file in its own
    unit (velocities in VP, moduli in RHO * VP^2 -- LAMBDA cancels, so not in LAMBDA --, ETA in 1)."""
    m = PC.models(a, N_MODELS, seed=2)
    back = PC.convert(PC.convert(m, a, b), b, a)
    assert np.array_equal(back[-1].view(np.uint64), m[-1].view(np.uint64))
    unit = PC.scales(a, m)
    err = (np.abs(back - m)[:-1] / unit[:-1]).max()
    bound = PC.there_and_back_bound(a, b)
    print(f"{a} -> {b} -> {a}: largest scaled error {err:.3e}, bound {bound:.3e}")
    assert bound < 1e-10                                   # (the bound says something: a wrong formula errs at 1e-2)
    assert err <= bound, (a, b, err, bound)


def test_there_and_back_covers_what_it_should():
    assert len(PC.THERE_AND_BACK) == 14
    assert (V, T) in PC.THERE_AND_BACK and (V, A) in PC.THERE_AND_BACK      # Voigt of an embedded isotropic model
    assert (T, V) not in PC.THERE_AND_BACK and (A, B) not in PC.THERE_AND_BACK


# ------------------------------------------------------------------------------------------------ the transposed Jacobian
H = 1e-5
N_FD = 400


def _adjoint_gap(steps, frm, seed):
    """(|<J d, K> - <d, J^T K>|, sum of |K_i J_ij d_j|) per model, in np.longdouble: J d by central difference quotients
    of the forward statement with the relative step H, J^T K and the entries of J by the transposed statement."""
    ld = np.longdouble
    rng = np.random.default_rng(seed)
    m = PC.models(frm, N_FD, seed).astype(ld)
    out = PC.run(steps, m)
    delta = (rng.uniform(-1.0, 1.0, m.shape).astype(ld)) * m            # a relative perturbation of every component
    k = (rng.choice([-1.0, 1.0], out.shape) * rng.uniform(0.5, 1.0, out.shape)).astype(ld) / np.abs(out)
    h = ld(H)
    quotient = (PC.run(steps, m + h * delta) - PC.run(steps, m - h * delta)) / (2 * h)
    lhs = (quotient * k).sum(axis=0)
    rhs = (delta * PC.run_transposed(steps, m, k)).sum(axis=0)
    terms = np.zeros(N_FD, dtype=ld)
    for i in range(out.shape[0]):
        unit = np.zeros_like(out)
        unit[i] = 1
        row = PC.run_transposed(steps, m, unit)                          # J[i, :]
        terms += np.abs(k[i]) * (np.abs(row) * np.abs(delta)).sum(axis=0)
    return np.abs(lhs - rhs), terms


@pytest.mark.parametrize("step", sorted(PC.STEPS))
def test_transposed_jacobian_of_every_step(step):
    gap, terms = _adjoint_gap((step,), PC.STEPS[step][0], seed=10 + step)
    print(f"step {step}: largest gap / terms {float((gap / terms).max()):.3e}")
    assert (terms > 0).all() and (gap <= 1e-8 * terms).all(), float((gap / terms).max())


@pytest.mark.parametrize("a,b", PC.PAIRS, ids=lambda x: x)
def test_transposed_jacobian_of_every_route(a, b):
    gap, terms = _adjoint_gap(PC.ROUTES[a, b], a, seed=40 + 5 * PC.NAMES.index(a) + PC.NAMES.index(b))
    print(f"{a} -> {b}: largest gap / terms {float((gap / terms).max()):.3e}")
    assert (terms > 0).all() and (gap <= 1e-8 * terms).all(), float((gap / terms).max())


def test_a_wrong_entry_would_show():
    """The check has teeth: one sign of one entry of one step changed errs at order one."""
    steps = PC.ROUTES[T, V]
    right = PC.transposed
    try:
        def wrong(step, m, k):
            out = right(step, m, k)
            if step == 8:
                out[3] = -out[3]
            return out

        PC.transposed = wrong
        gap, terms = _adjoint_gap(steps, T, seed=77)
    finally:
        PC.transposed = right
    assert (gap > 1e-3 * terms).any()


# ------------------------------------------------------------------------------------------- the header and the table
def _header_code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))


_SCALARS = {"int": "int", "int64_t": "int64", "long long": "int64", "size_t": "size_t", "double": "double", "void": "void"}


def _c_class(decl, is_return=False):
    decl = " ".join(decl.replace("*", " * ").split())
    if "*" in decl:
        return "char*" if is_return and decl == "const char *" else "pointer"
    words = [w for w in decl.split() if w != "const"]
    if not is_return and " ".join(words) not in _SCALARS:
        words = words[:-1]                                   # the parameter's name
    return _SCALARS[" ".join(words)]


def _declared_prototypes():
    protos = {}
    for statement in _header_code().split(";"):
        m = re.fullmatch(r"\s*([^()]*?)\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^()]*)\)\s*", re.split(r"[{}]", statement)[-1])
        if not m:
            continue
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        protos[name] = (_c_class(ret, is_return=True), [_c_class(p) for p in params])
    return protos


def _ctypes_class(t):
    if t is C.c_void_p or issubclass(t, C._Pointer):
        return "pointer"
    if t in (C.c_int64, C.c_longlong):
        return "int64"
    return {C.c_int: "int", C.c_size_t: "size_t", C.c_double: "double"}[t]


def test_the_extension_header_and_the_table_agree():
    protos = _declared_prototypes()
    assert list(protos) == list(P.SIGNATURES) == list(SYMBOLS)
    lib = P.bind()
    assert lib is helpers.load_lib()
    for name, (ret, params) in protos.items():
        assert hasattr(lib, name), name
        restype, argtypes = P.SIGNATURES[name]
        assert (_ctypes_class(restype), [_ctypes_class(t) for t in argtypes]) == (ret, params), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert name not in helpers.SIGNATURES and name not in helpers.EXPORTED_SYMBOLS
    # the numbers and limits the module repeats
    text = open(HEADER).read()
    assert int(re.search(r"#define MM_PARAM_MAX_P (\d+)", text).group(1)) == P.MAX_P
    for number, name in enumerate(P.PARAMETRISATIONS):
        assert int(re.search(rf"#define MM_PARAM_{name.upper()} (\d+)", text).group(1)) == number


# --------------------------------------------------------------------------------------------------- argument checks
CTX = C.c_void_p(0x1000)           # a dummy: a refused call never looks at the context
IN, OUT, KIN = C.c_void_p(0x100000), C.c_void_p(0x900000), C.c_void_p(0x500000)   # never read on the host either


def _cols(*c):
    return (C.c_int * len(c))(*c)


def _values_call(lib, ctx=CTX, frm=0, to=1, ngroups=10, P_=8, src=IN, sgs=8, scs=80, scols=_cols(0, 1, 2), dst=OUT, dgs=8,
                 dcs=80, dcols=_cols(0, 1, 2)):
    return lib.mm_convert_parameters(ctx, frm, to, ngroups, P_, src, sgs, scs, scols, dst, dgs, dcs, dcols, None)


def _kernels_call(lib, ctx=CTX, frm=0, to=1, ngroups=10, P_=8, model=IN, mgs=8, mcs=80, mcols=_cols(0, 1, 2), kin=KIN,
                  kgs=8, kcs=80, kcols=_cols(0, 1, 2), kout=OUT, ogs=8, ocs=80, ocols=_cols(0, 1, 2)):
    return lib.mm_convert_kernels(ctx, frm, to, ngroups, P_, model, mgs, mcs, mcols, kin, kgs, kcs, kcols, kout, ogs, ocs,
                                  ocols, None)


SIX = _cols(0, 1, 2, 3, 4, 5)
REFUSED_VALUES = {
    "null ctx": dict(ctx=None),
    "null in": dict(src=None),
    "null out": dict(dst=None),
    "null in cols": dict(scols=None),
    "null out cols": dict(dcols=None),
    "from below": dict(frm=-1),
    "from above": dict(frm=5),
    "to below": dict(to=-1),
    "to above": dict(to=5),
    "from == to": dict(frm=2, to=2),
    "negative ngroups": dict(ngroups=-1),
    "P zero": dict(P_=0),
    "P negative": dict(P_=-3),
    "P above 4096": dict(P_=4097, sgs=4097, scs=40970, dgs=4097, dcs=40970),
    "negative in column": dict(scols=_cols(0, -1, 2)),
    "negative out column": dict(dcols=_cols(0, 1, -2)),
    "negative in group stride": dict(sgs=-8),
    "negative in comp stride": dict(scs=-80),
    "negative out group stride": dict(dgs=-8),
    "negative out comp stride": dict(dcs=-80),
    "equal out columns": dict(dcols=_cols(0, 1, 1)),
    "equal out columns of six": dict(to=3, dcols=_cols(0, 1, 2, 3, 4, 1)),
    "in extent at 2^48": dict(ngroups=2, sgs=(1 << 48) - 8 - 160),
    "in extent past 2^48 by the column": dict(scols=_cols(0, 1, 1 << 30), scs=1 << 20),
    "out extent at 2^48": dict(ngroups=1 << 45, dcs=1 << 48),
    "ngroups at 2^48": dict(ngroups=1 << 48),
    "partial overlap: out starts inside in": dict(dst=C.c_void_p(0x100000 + 8 * 8)),
    "partial overlap: same start, other strides": dict(dst=IN, dgs=8, dcs=88),
    "partial overlap: in starts inside out": dict(src=C.c_void_p(0x900000 + 8 * 100)),
}
REFUSED_KERNELS = {
    "null ctx": dict(ctx=None),
    "null model": dict(model=None),
    "null kin": dict(kin=None),
    "null kout": dict(kout=None),
    "null model cols": dict(mcols=None),
    "null kin cols": dict(kcols=None),
    "null kout cols": dict(ocols=None),
    "from above": dict(frm=7),
    "to below": dict(to=-2),
    "from == to": dict(frm=4, to=4),
    "negative ngroups": dict(ngroups=-5),
    "P zero": dict(P_=0),
    "P above 4096": dict(P_=5000),
    "negative model column": dict(mcols=_cols(-1, 1, 2)),
    "negative kin column": dict(kcols=_cols(0, -1, 2)),
    "negative kout column": dict(ocols=_cols(0, 1, -1)),
    "negative model stride": dict(mgs=-1),
    "negative kin stride": dict(kcs=-1),
    "negative kout stride": dict(ogs=-1),
    "equal kout columns": dict(ocols=_cols(2, 1, 2)),
    "kin extent at 2^48": dict(ngroups=2, kgs=(1 << 48) - 8 - 160),
    "kout extent at 2^48": dict(ngroups=1 << 45, ocs=1 << 48),
    "partial overlap: kout inside model": dict(kout=C.c_void_p(0x100000 + 8)),
    "partial overlap: kout inside kin": dict(kout=C.c_void_p(0x500000 + 8 * 16)),
    "partial overlap: kout is kin with other strides": dict(kout=KIN, ocs=96),
}


def test_the_extent_cases_sit_on_the_limit():
    """(ngroups - 1) * group_stride + max(cols) * comp_stride + P of the two stride cases is exactly 2^48."""
    assert (2 - 1) * ((1 << 48) - 8 - 160) + 2 * 80 + 8 == 1 << 48


@pytest.mark.parametrize("what", list(REFUSED_VALUES))
def test_convert_parameters_refuses_without_a_gpu(what):
    lib = P.bind()
    assert _values_call(lib, **REFUSED_VALUES[what]) == -1, what
    message = lib.mm_last_error()
    assert b"mm_convert_parameters" in message and len(message) > len(b"mm_convert_parameters: "), message
    assert lib.mm_last_status() == -1


@pytest.mark.parametrize("what", list(REFUSED_KERNELS))
def test_convert_kernels_refuses_without_a_gpu(what):
    lib = P.bind()
    assert _kernels_call(lib, **REFUSED_KERNELS[what]) == -1, what
    message = lib.mm_last_error()
    assert b"mm_convert_kernels" in message and len(message) > len(b"mm_convert_kernels: "), message


def test_one_below_the_extent_limit_and_no_groups_pass_the_checks():
    """What is refused is the argument that is named: the same calls with ngroups == 0 -- valid, and decided before the
    device is touched -- return MM_OK, also with null arrays and with the strides of the extent cases."""
    lib = P.bind()
    assert _values_call(lib, ngroups=0) == 0
    assert _values_call(lib, ngroups=0, src=None, dst=None) == 0
    assert _values_call(lib, ngroups=0, dst=IN) == 0
    assert _kernels_call(lib, ngroups=0, model=None, kin=None, kout=None) == 0
    assert _values_call(lib, ngroups=0, dcols=_cols(0, 0, 1)) == -1            # the columns are checked all the same


# -------------------------------------------------------------------------------------------------------------- detect
def test_detect():
    assert P.detect(mio.pick_parameters("ISO")) == V
    assert P.detect(mio.pick_parameters("TTI")) == T
    from multimesh_amd import api

    assert P.detect(api.TTI_PARAMS) == T
    assert P.detect(["LAMBDA", "MU", "RHO", "QMU", "whatever"]) == L
    assert P.detect(["A", "C", "L", "N", "F", "RHO"]) == A
    with pytest.raises(ValueError, match=r"several.*iso_lame.*iso_bulk"):
        P.detect(["LAMBDA", "KAPPA", "MU", "RHO"])
    with pytest.raises(ValueError, match=r"several.*iso_velocity.*vti_velocity"):
        P.detect(mio.pick_parameters("ISO") + mio.pick_parameters("TTI"))
    for names in ([], ["QKAPPA", "QMU"], ["VP", "VS"], ["VPV", "VPH", "VSV", "VSH", "RHO"]):
        with pytest.raises(ValueError, match="no complete parametrisation.*iso_velocity.*vti_love"):
            P.detect(names)
