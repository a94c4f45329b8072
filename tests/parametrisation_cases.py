"""The NumPy statement of mm_convert_parameters and mm_convert_kernels (include/multimesh_params.h), written from the
header and not from the kernels.  Nothing here imports the code under test.

Every step is spelt out with each operation rounded on its own: ``x * x`` for a square, sums left to right as written,
``(2.0 * mu) / 3.0``.  The functions are generic in the float type (the tests run them in ``np.longdouble`` for the
difference quotients).  A state is a list of arrays, one per component, in the order of ``COMPONENTS``.

  forward(step, m)        the components of the step's target parametrisation from those of its source
  transposed(step, m, k)  J^T k at the step's input m: kernels with respect to the source from those of the target
  convert / convert_kernels   a route: the composition, forward; then the transposes in reverse at the kept inputs
"""
import numpy as np

from grid_import_cases import same_bits  # noqa: F401  (NaN in the same places, every other value bit for bit)

COMPONENTS = {
    "iso_velocity": ("VP", "VS", "RHO"),
    "iso_lame": ("LAMBDA", "MU", "RHO"),
    "iso_bulk": ("KAPPA", "MU", "RHO"),
    "vti_velocity": ("VPV", "VPH", "VSV", "VSH", "ETA", "RHO"),
    "vti_love": ("A", "C", "L", "N", "F", "RHO"),
}
NAMES = tuple(COMPONENTS)

# step -> (from, to), in the header's numbering
STEPS = {
    1: ("iso_velocity", "iso_lame"),
    2: ("iso_lame", "iso_velocity"),
    3: ("iso_lame", "iso_bulk"),
    4: ("iso_bulk", "iso_lame"),
    5: ("vti_velocity", "vti_love"),
    6: ("vti_love", "vti_velocity"),
    7: ("iso_velocity", "vti_velocity"),
    8: ("vti_love", "iso_bulk"),
}

# the route of every ordered pair, written out: the fewest steps around the ring
# iso_velocity -- iso_lame -- iso_bulk <- vti_love -- vti_velocity <- iso_velocity
ROUTES = {
    ("iso_velocity", "iso_lame"): (1,),
    ("iso_velocity", "iso_bulk"): (1, 3),
    ("iso_velocity", "vti_velocity"): (7,),
    ("iso_velocity", "vti_love"): (7, 5),
    ("iso_lame", "iso_velocity"): (2,),
    ("iso_lame", "iso_bulk"): (3,),
    ("iso_lame", "vti_velocity"): (2, 7),
    ("iso_lame", "vti_love"): (2, 7, 5),
    ("iso_bulk", "iso_velocity"): (4, 2),
    ("iso_bulk", "iso_lame"): (4,),
    ("iso_bulk", "vti_velocity"): (4, 2, 7),
    ("iso_bulk", "vti_love"): (4, 2, 7, 5),
    ("vti_velocity", "iso_velocity"): (5, 8, 4, 2),
    ("vti_velocity", "iso_lame"): (5, 8, 4),
    ("vti_velocity", "iso_bulk"): (5, 8),
    ("vti_velocity", "vti_love"): (5,),
    ("vti_love", "iso_velocity"): (8, 4, 2),
    ("vti_love", "iso_lame"): (8, 4),
    ("vti_love", "iso_bulk"): (8,),
    ("vti_love", "vti_velocity"): (6,),
}
PAIRS = tuple(ROUTES)


def route_names(pair):
    return tuple(f"{STEPS[s][0]}->{STEPS[s][1]}" for s in ROUTES[pair])


_QUIET = dict(invalid="ignore", over="ignore", divide="ignore", under="ignore")


# ------------------------------------------------------------------------------------------------------- the statement
def forward(step, m):
    with np.errstate(**_QUIET):
        if step == 1:
            vp, vs, rho = m
            mu = rho * (vs * vs)
            return [rho * (vp * vp) - 2.0 * mu, mu, rho]
        if step == 2:
            lam, mu, rho = m
            vs = np.sqrt(mu / rho)
            vp = np.sqrt((lam + 2.0 * mu) / rho)
            return [vp, vs, rho]
        if step == 3:
            lam, mu, rho = m
            return [lam + (2.0 * mu) / 3.0, mu, rho]
        if step == 4:
            kappa, mu, rho = m
            return [kappa - (2.0 * mu) / 3.0, mu, rho]
        if step == 5:
            vpv, vph, vsv, vsh, eta, rho = m
            A = rho * (vph * vph)
            C = rho * (vpv * vpv)
            L = rho * (vsv * vsv)
            N = rho * (vsh * vsh)
            return [A, C, L, N, eta * (A - 2.0 * L), rho]
        if step == 6:
            A, C, L, N, F, rho = m
            return [np.sqrt(C / rho), np.sqrt(A / rho), np.sqrt(L / rho), np.sqrt(N / rho), F / (A - 2.0 * L), rho]
        if step == 7:
            vp, vs, rho = m
            return [vp.copy(), vp.copy(), vs.copy(), vs.copy(), np.ones_like(vp), rho]
        if step == 8:
            A, C, L, N, F, rho = m
            kappa = (((C + 4.0 * A) - 4.0 * N) + 4.0 * F) / 9.0
            mu = ((((A + C) + 6.0 * L) + 5.0 * N) - 2.0 * F) / 15.0
            return [kappa, mu, rho]
    raise ValueError(step)


def transposed(step, m, k):
    """J^T k of ``step`` at its input ``m``: the plain derivatives of the formulas of :func:`forward`."""
    with np.errstate(**_QUIET):
        if step == 1:
            vp, vs, rho = m
            klam, kmu, krho = k
            r2 = 2.0 * rho
            return [(r2 * vp) * klam, (r2 * vs) * (kmu - 2.0 * klam),
                    (krho + (vp * vp - 2.0 * (vs * vs)) * klam) + (vs * vs) * kmu]
        if step == 2:
            lam, mu, rho = m
            kvp, kvs, krho = k
            r2 = 2.0 * rho
            vs = np.sqrt(mu / rho)
            vp = np.sqrt((lam + 2.0 * mu) / rho)
            return [kvp / (r2 * vp), kvp / (rho * vp) + kvs / (r2 * vs), (krho - (vp / r2) * kvp) - (vs / r2) * kvs]
        if step == 3:
            kkappa, kmu, krho = k
            return [kkappa, kmu + (2.0 * kkappa) / 3.0, krho]
        if step == 4:
            klam, kmu, krho = k
            return [klam, kmu - (2.0 * klam) / 3.0, krho]
        if step == 5:
            vpv, vph, vsv, vsh, eta, rho = m
            kA, kC, kL, kN, kF, krho = k
            r2 = 2.0 * rho
            A = rho * (vph * vph)
            L = rho * (vsv * vsv)
            ef = eta * kF
            a = kA + ef
            l = kL - 2.0 * ef
            return [(r2 * vpv) * kC, (r2 * vph) * a, (r2 * vsv) * l, (r2 * vsh) * kN, (A - 2.0 * L) * kF,
                    (((krho + (vph * vph) * a) + (vpv * vpv) * kC) + (vsv * vsv) * l) + (vsh * vsh) * kN]
        if step == 6:
            A, C, L, N, F, rho = m
            kvpv, kvph, kvsv, kvsh, keta, krho = k
            r2 = 2.0 * rho
            vpv, vph, vsv, vsh = np.sqrt(C / rho), np.sqrt(A / rho), np.sqrt(L / rho), np.sqrt(N / rho)
            d = A - 2.0 * L
            eta = F / d
            g = eta / d
            return [kvph / (r2 * vph) - g * keta, kvpv / (r2 * vpv), kvsv / (r2 * vsv) + (2.0 * g) * keta,
                    kvsh / (r2 * vsh), keta / d,
                    (((krho - (vpv / r2) * kvpv) - (vph / r2) * kvph) - (vsv / r2) * kvsv) - (vsh / r2) * kvsh]
        if step == 7:
            kvpv, kvph, kvsv, kvsh, keta, krho = k
            return [kvpv + kvph, kvsv + kvsh, krho]
        if step == 8:
            kkappa, kmu, krho = k
            a = kkappa / 9.0
            b = kmu / 15.0
            return [4.0 * a + b, a + b, 6.0 * b, 5.0 * b - 4.0 * a, 4.0 * a - 2.0 * b, krho]
    raise ValueError(step)


def run(steps, m):
    """The steps in turn on the state ``m`` (a list or an array [C, n]) -> array [C_to, n]."""
    m = list(m)
    for s in steps:
        m = forward(s, m)
    return np.stack(m)


def run_transposed(steps, m, k):
    """J^T k of the composition of ``steps`` at ``m``: forward with every step's input kept, transposes in reverse."""
    m, k = list(m), list(k)
    inputs = []
    for s in steps[:-1]:
        inputs.append(m)
        m = forward(s, m)
    inputs.append(m)
    for s, at in zip(reversed(steps), reversed(inputs)):
        k = transposed(s, at, k)
    return np.stack(k)


def convert(values, frm, to):
    v = np.asarray(values, dtype=np.float64)
    return run(ROUTES[frm, to], v.reshape(v.shape[0], -1)).reshape((len(COMPONENTS[to]),) + v.shape[1:])


def convert_kernels(kernels, model, frm, to):
    m = np.asarray(model, dtype=np.float64)
    k = np.asarray(kernels, dtype=np.float64)
    return run_transposed(ROUTES[frm, to], m.reshape(m.shape[0], -1), k.reshape(k.shape[0], -1)).reshape(m.shape)


def n_bad(out):
    """The number of nodes with at least one component that is not finite, of an array [C, ...]."""
    out = np.asarray(out)
    return int((~np.isfinite(out.reshape(out.shape[0], -1))).any(axis=0).sum())


# ---------------------------------------------------------------------------------------------------------- the models
def iso_models(n, seed):
    """f64[3, n] in iso_velocity: VP in [2000, 9000], VS / VP in [0.4, 0.6], RHO in [1000, 6000]."""
    rng = np.random.default_rng(seed)
    vp = rng.uniform(2000.0, 9000.0, n)
    return np.stack([vp, vp * rng.uniform(0.4, 0.6, n), rng.uniform(1000.0, 6000.0, n)])


def vti_models(n, seed):
    """f64[6, n] in vti_velocity: an isotropic model of :func:`iso_models` with every velocity changed by a factor within
    +-5 % of its own, and ETA in [0.8, 1.1]."""
    rng = np.random.default_rng(seed + 1000)
    vp, vs, rho = iso_models(n, seed)
    f = rng.uniform(0.95, 1.05, (4, n))
    return np.stack([vp * f[0], vp * f[1], vs * f[2], vs * f[3], rng.uniform(0.8, 1.1, n), rho])


def models(name, n, seed):
    """f64[C, n] in the parametrisation ``name``: the models above, through the statement."""
    if name in ("iso_velocity", "iso_lame", "iso_bulk"):
        v = iso_models(n, seed)
        return v if name == "iso_velocity" else convert(v, "iso_velocity", name)
    v = vti_models(n, seed)
    return v if name == "vti_velocity" else convert(v, "vti_velocity", name)


# --------------------------------------------------------------------------------------------- the there-and-back bound
# Scaled units: with VPM the largest P velocity of a node and S = RHO * VPM^2, velocities are measured in VPM, moduli in S,
# ETA in 1; RHO is copied by every step and must come back bit for bit.  Over the models above (VS / VP in [0.4, 0.6],
# velocities within +-5 %, ETA <= 1.1) the scaled velocities lie in [0.9, 1] (P) and [0.36, 0.67] (S: 0.4 * 0.95 / 1.05 and
# 0.6 * 1.05 / 0.95), the scaled moduli below 1 (A, C, LAMBDA + 2 MU), 0.44 (L, N, MU), and
# d = (A - 2 L) / S >= (0.95^2 - 2 (0.6 * 1.05)^2) / 1.05^2 = 0.098.
#
# A rounding replaces an intermediate x by x (1 + e), |e| <= u = 2^-53: an error of at most u |x| <= u * MAGNITUDE, the
# largest intermediate being the partial sum A + C + 6 L + 5 N <= 2 + 11 * 0.44 < 7 of step 8.  To first order the error
# then goes through the rest of its step and the later steps like a perturbation of an input, and is multiplied by at most
# the infinity norm of each scaled Jacobian -- the largest row sum of |dy_i / dx_j| -- or by 1 where that is smaller:
#   1  LAMBDA: 2 vp + 4 vs <= 2 + 4 * 0.6 = 4.4 (isotropic: vp = 1, vs <= 0.6); MU: 2 vs                       GAIN 4.4
#   2  VP: 1 / (2 vp) + 1 / vp = 1.5; VS: 1 / (2 vs) <= 1 / 0.8                                                GAIN 1.5
#   3, 4  1 + 2 / 3                                                                                             GAIN 5/3
#   5  A, C: 2 vp <= 2; L, N: 2 vs <= 1.34; F: eta (2 vph + 4 vsv) + d <= 1.1 * (2 + 2.68) + 1 = 6.15           GAIN 6.2
#   6  P: 1 / (2 * 0.9); S: 1 / (2 * 0.36) = 1.39; ETA: (eta + 2 eta + 1) / d <= (3 * 1.1 + 1) / 0.098 = 43.9   GAIN 44
#   7  copies                                                                                                   GAIN 1
#   8  KAPPA: (1 + 4 + 4 + 4) / 9; MU: (1 + 1 + 6 + 5 + 2) / 15 = 1                                             GAIN 13/9
# ROUNDINGS counts the arithmetic operations of each step's statement.  So the scaled error of a there-and-back route is at
# most  (sum of its roundings) * u * MAGNITUDE * (product of its gains), and twice that covers the second-order terms
# (the first-order bound is below 1e-11, its square far below u).  LAMBDA and KAPPA are differences of larger terms: the
# bound is relative to S = RHO * VP^2, not to LAMBDA.  Nothing here was fitted to what the code gives.
U = 2.0 ** -53
MAGNITUDE = 7.0
GAIN = {1: 4.4, 2: 1.5, 3: 5.0 / 3.0, 4: 5.0 / 3.0, 5: 6.2, 6: 44.0, 7: 1.0, 8: 13.0 / 9.0}
ROUNDINGS = {1: 6, 2: 6, 3: 3, 4: 3, 5: 11, 6: 11, 7: 0, 8: 15}

ISO = ("iso_velocity", "iso_lame", "iso_bulk")
#: (a, b): a -> b -> a returns its input -- from an isotropic parametrisation through any other (the embedded model is
#: isotropic and its Voigt average is itself), between the two VTI ones; VTI -> isotropic loses the anisotropy
THERE_AND_BACK = tuple((a, b) for a in NAMES for b in NAMES if a != b and (a in ISO or b not in ISO))


def there_and_back_bound(a, b):
    steps = ROUTES[a, b] + ROUTES[b, a]
    gain = 1.0
    for s in steps:
        gain *= max(1.0, GAIN[s])
    return 2.0 * sum(ROUNDINGS[s] for s in steps) * U * MAGNITUDE * gain


def scales(name, values):
    """f64[C, n]: the unit of every component of ``values`` [C, n] in ``name`` (0 for RHO: it must be exact)."""
    v = np.asarray(values, dtype=np.float64)
    rho = v[-1]
    if name == "iso_velocity":
        vpm = v[0]
    elif name == "vti_velocity":
        vpm = np.maximum(v[0], v[1])
    elif name == "iso_lame":
        vpm = np.sqrt((v[0] + 2.0 * v[1]) / rho)
    elif name == "iso_bulk":
        vpm = np.sqrt((v[0] + 4.0 * v[1] / 3.0) / rho)
    else:
        vpm = np.sqrt(np.maximum(v[0], v[1]) / rho)
    unit = {"velocity": vpm, "modulus": rho * vpm * vpm}
    kinds = {"iso_velocity": "vv", "iso_lame": "mm", "iso_bulk": "mm", "vti_velocity": "vvvv1", "vti_love": "mmmmm"}[name]
    rows = [unit["velocity"] if c == "v" else unit["modulus"] if c == "m" else np.ones_like(rho) for c in kinds]
    return np.stack(rows + [np.zeros_like(rho)])


# ----------------------------------------------------------------------------------------------------- the special rows
def special_rows(name, values):
    """``values`` f64[C, n] (n >= 16) in ``name`` with special rows written over its first nodes: VS = 0 (a fluid),
    RHO = 0, A - 2 L = 0, a negative MU, NaN, +inf, -inf, -0.0 and a denormal, as far as ``name`` has the component."""
    v = np.array(values, dtype=np.float64)
    comps = COMPONENTS[name]
    shear = [i for i, c in enumerate(comps) if c in ("VS", "VSV", "VSH", "MU", "L", "N")]
    rho = comps.index("RHO")
    v[shear, 0] = 0.0                                   # a fluid node
    v[rho, 1] = 0.0
    if name == "vti_love":
        v[0, 2] = 2.0 * v[2, 2]                         # A - 2 L = 0 exactly
    elif name == "vti_velocity":
        v[1, 2], v[2, 2], v[rho, 2] = np.sqrt(2.0), 1.0, 1.0   # (A - 2 L as close to 0 as velocities allow: one ulp of 2)
    v[shear[0], 3] = -abs(v[shear[0], 3]) - 1.0         # a negative shear component (MU < 0: sqrt of a negative)
    v[0, 4] = np.nan
    v[0, 5] = np.inf
    v[1, 6] = -np.inf
    v[shear[0], 7] = -0.0
    v[0, 8] = 5e-324
    v[rho, 9] = 2.2250738585072014e-308 / 4.0           # a denormal density
    v[:, 10] = 0.0
    v[:, 11] = -0.0
    v[rho, 12] = np.inf
    v[:, 13] = np.nan
    return v
