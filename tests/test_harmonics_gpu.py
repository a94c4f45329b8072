"""mm_harmonic_model_apply on the GPU: bit for bit the NumPy statement of tests/harmonic_cases.py (NaN positions are
compared, NaN payloads are not) -- sizes around the wave and the workgroup and past the launch cap, degrees 0 to 40,
1 to 5 components, the special points of the header, the three modes in and out of place, the count of nodes outside the
table, what the host refuses, a caller's stream with caller-owned tensors, and the drivers of
:mod:`multimesh_amd.harmonics` on a GLL mesh, a hex mesh and a Salvus model in memory."""
import numpy as np
import pytest

import harmonic_cases as HC
from multimesh_amd import harmonics as H
from multimesh_amd import io as mio
from multimesh_amd import synth
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

MM_ERR_ARG = -1
CAP_LANES = 2048 * 256          # kMaxBlocks workgroups of 256 lanes: beyond, the workgroups stride


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()      # before this module's context opens the device: torch then finds it whichever test runs first
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    with Context(0) as c:
        yield c


def _check(ctx, pts, R, coef, L, mode=0, extend=False, values_in=None, start=0, in_place=False):
    """The device against the statement: values and count.  Returns the statement's (out, noutside)."""
    want, nout = HC.model_apply(pts, R, coef, L, mode=mode, extend=extend, values_in=values_in)
    count = ctx.to_device(np.array([start], dtype=np.int64))
    src = None if values_in is None else ctx.to_device(np.asarray(values_in, dtype=np.float64).reshape(coef.shape[0], -1))
    out = H.harmonic_model_apply(ctx, pts, R, coef, L, mode=mode, extend=extend, values_in=src,
                                 out=src if in_place else None, noutside=count)
    got = out.numpy().reshape(coef.shape[0], -1)
    assert (out.ptr == src.ptr) if in_place else True
    assert HC.same_bits_nan(got, want), f"{(~(got == want) & ~(np.isnan(got) & np.isnan(want))).sum()} of {got.size} values differ"
    assert int(count.numpy()[0]) == start + nout
    return want, nout


# ----------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_sizes_around_the_wave_and_the_workgroup(ctx, n):
    L, R = 7, HC.knots(7)
    coef = HC.coefficients(L, R.size, 2, seed=n)
    _check(ctx, HC.cloud(n, seed=n), R, coef, L)
    if n % 5 == 0 and n:
        _check(ctx, HC.elements(n // 5, 5, seed=n), R, coef, L)


def test_past_the_launch_cap(ctx):
    """More points than kMaxBlocks * 256 lanes at P = 1: the stride loop runs (and its second step ends in a partial tile)."""
    L, R = 4, HC.knots(5)
    n = CAP_LANES + 1000
    _check(ctx, HC.cloud(n, seed=1, r_lo=HC.R_CMB - 2e5), R, HC.coefficients(L, R.size, 1, seed=3), L)


# --------------------------------------------------------------------------------------------- degrees and components
@pytest.mark.parametrize("P", (1, 27, 125))
@pytest.mark.parametrize("L", (0, 1, 2, 7, 40))
def test_degrees(ctx, L, P):
    R = HC.knots(9)
    G = -(-257 // P)
    pts = HC.cloud(257, seed=L) if P == 1 else HC.elements(G, P, seed=L + P)
    _check(ctx, pts, R, HC.coefficients(L, R.size, 2, seed=L + 100), L, extend=True)


@pytest.mark.parametrize("ncomp", (1, 3, 4, 5))
def test_components(ctx, ncomp):
    """1, 3, 4: the unrolled forms; 5: four and one more launch.  The count is taken once."""
    L, R = 7, HC.knots(7)
    pts = HC.elements(11, 27, seed=ncomp, r_lo=HC.R_CMB - 3e5, r_hi=HC.R_MOHO + 3e5)
    _, nout = _check(ctx, pts, R, HC.coefficients(L, R.size, ncomp, seed=ncomp), L, start=5)
    assert nout > 0 and nout % 27 == 0


# -------------------------------------------------------------------------------------------------------- special points
def test_special_points(ctx):
    L, R = 7, HC.knots(7)
    coef = HC.coefficients(L, R.size, 3, seed=9)
    r = 5.0e6
    pts = HC.cloud(70, seed=4)
    pts[:12] = [[0, 0, r], [0, 0, -r], [1e-9, 0, r], [0, -1e-9, -r], [0, 0, 0], [r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0],
                [np.nan, 1.0, r], [np.inf, 0, r], [1.0, -np.inf, 2.0]]
    pts[12] = [0, 0, HC.R_670]                          # on the discontinuity, P = 1: the upper side
    pts[13], pts[14] = [0, 0, R[0] - 1e5], [0, 0, R[-1] + 1e5]
    for extend in (False, True):
        want, nout = _check(ctx, pts, R, coef, L, extend=extend)
        assert np.isnan(want[:, 9]).all() and (nout == 0) == extend
    # at degree 40 the sectoral terms underflow next to the pole: gradual underflow is part of the statement
    coef40 = HC.coefficients(40, R.size, 1, seed=10)
    near = np.array([[1e-9, 0, r], [3e-3, -4e-3, -r], [1e-300, 0, r], [0, 5e-324, r], [1e3, 1e3, r]])
    _check(ctx, near, R, coef40, 40)


def test_a_node_on_the_discontinuity_takes_the_side_of_its_element(ctx):
    L, R = 4, HC.knots(7)
    coef = HC.coefficients(L, R.size, 1, seed=2)
    u = HC.directions(1, seed=6)[0]
    shared = HC.R_670 * u
    below = np.array([shared, (HC.R_670 - 4e4) * u, (HC.R_670 - 8e4) * u])
    above = np.array([shared, (HC.R_670 + 4e4) * u, (HC.R_670 + 8e4) * u])
    want, _ = _check(ctx, np.stack([below, above]), R, coef, L)
    assert want[0, 0] != want[0, 3]                     # the two copies of the node differ: each took its own side


def test_uniform_and_straddling_waves(ctx):
    """64 whole elements of 4 nodes within one knot interval (every wave shares i: the scalar path); then elements whose
    nodes span several intervals, and a wave whose first lanes lie outside the table (the per-lane path)."""
    L = 7
    R = HC.knots(7, discontinuity=False)
    coef = HC.coefficients(L, R.size, 4, seed=1)
    mid = 0.5 * (R[2] + R[3])
    inside = HC.elements(64, 4, seed=3, size=1e4, r_lo=mid - 1e4, r_hi=mid + 1e4)
    _check(ctx, inside, R, coef, L)
    span = np.stack([HC.shell_element(27, R[0] + 1e3, R[-1] - 1e3, seed=s) for s in range(12)])
    _check(ctx, span, R, coef, L)
    mixed = np.concatenate([HC.elements(3, 27, seed=8, r_lo=R[-1] + 2e5, r_hi=R[-1] + 3e5), span])
    _, nout = _check(ctx, mixed, R, coef, L)
    assert nout == 3 * 27
    _check(ctx, mixed, HC.knots(7), coef, L, extend=True)


# ------------------------------------------------------------------------------------------------------ modes and counts
@pytest.mark.parametrize("mode,in_place", ((0, False), (1, False), (1, True), (2, False), (2, True)))
def test_modes(ctx, mode, in_place):
    L, R = 7, HC.knots(7)
    pts = HC.elements(20, 27, seed=mode, r_lo=HC.R_CMB - 2e5, r_hi=HC.R_MOHO + 2e5)
    vin = np.random.default_rng(mode).uniform(3000.0, 9000.0, (3, 20 * 27))
    vin[0, 5], vin[1, 6] = np.nan, np.inf
    _check(ctx, pts, R, HC.coefficients(L, R.size, 3, seed=5), L, mode=mode, values_in=None if mode == 0 else vin,
           start=1234567, in_place=in_place)


def test_nothing_to_do_is_valid(ctx):
    L, R = 3, HC.knots(5)
    lib = H.bind(ctx.lib)
    Rd, c = ctx.to_device(R), ctx.to_device(HC.coefficients(L, R.size, 1, seed=1))
    p, out = ctx.to_device(HC.cloud(8, seed=1)), ctx.to_device(np.full(8, -7.0))
    count = ctx.to_device(np.array([3], dtype=np.int64))
    assert lib.mm_harmonic_model_apply(ctx.handle, p.ptr, 8, 1, Rd.ptr, R.size, L, None, 0, 0, 0, None, None, count.ptr) == 0
    assert lib.mm_harmonic_model_apply(ctx.handle, None, 0, 1, Rd.ptr, R.size, L, c.ptr, 1, 0, 0, None, None, count.ptr) == 0
    assert (out.numpy() == -7.0).all() and int(count.numpy()[0]) == 3
    assert H.harmonic_model_apply(ctx, np.zeros((0, 3)), R, HC.coefficients(L, R.size, 2, seed=1), L).shape == (2, 0)


# ------------------------------------------------------------------------------------------------- what the host refuses
def test_a_bad_table_is_refused_with_nothing_written(ctx):
    L = 3
    lib = H.bind(ctx.lib)
    p, out = ctx.to_device(HC.cloud(8, seed=1)), ctx.to_device(np.full(8, -7.0))
    count = ctx.to_device(np.array([3], dtype=np.int64))
    tables = {"descending": [1.0, 3.0, 2.0, 4.0], "not finite": [1.0, 2.0, np.inf, np.inf], "a NaN": [1.0, np.nan, 3.0, 4.0],
              "three equal radii": [1.0, 2.0, 2.0, 2.0, 3.0], "a discontinuity at the start": [1.0, 1.0, 2.0, 3.0],
              "a discontinuity at the end": [1.0, 2.0, 3.0, 3.0]}
    for what, R in tables.items():
        Rd = ctx.to_device(np.array(R))
        c = ctx.to_device(HC.coefficients(L, len(R), 1, seed=1))
        rc = lib.mm_harmonic_model_apply(ctx.handle, p.ptr, 8, 1, Rd.ptr, len(R), L, c.ptr, 1, 0, 0, None, out.ptr, count.ptr)
        assert rc == MM_ERR_ARG, what
        assert b"mm_harmonic_model_apply" in lib.mm_last_error()
        with pytest.raises(ValueError, match="mm_harmonic_model_apply"):
            H.harmonic_model_apply(ctx, p, Rd, c, L, out=out)
    ctx.synchronize()
    assert (out.numpy() == -7.0).all() and int(count.numpy()[0]) == 3
    # the cases that need no table (tests/test_harmonics.py lists them all) are refused on a live context as well
    Rd, c = ctx.to_device(HC.knots(5)), ctx.to_device(HC.coefficients(L, 5, 1, seed=1))
    for kw in (dict(P=300), dict(lmax=256), dict(mode=3), dict(extend=2), dict(m=1)):
        a = dict(P=1, lmax=L, mode=0, extend=0, m=5)
        a.update(kw)
        rc = lib.mm_harmonic_model_apply(ctx.handle, p.ptr, 8 // a["P"] if a["P"] <= 8 else 1, a["P"], Rd.ptr, a["m"], a["lmax"],
                                         c.ptr, 1, a["mode"], a["extend"], None, out.ptr, count.ptr)
        assert rc == MM_ERR_ARG, kw
    assert (out.numpy() == -7.0).all() and int(count.numpy()[0]) == 3


# ------------------------------------------------------------------------------- a caller's stream and caller's tensors
def test_on_a_callers_stream_with_the_callers_tensors(torch):
    """Late producer, early consumer, as tests/test_caller_stream_gpu.py: under a side stream the inputs hold zeros while
    the stream spins, the true values are copied in on that stream, the library is called and its outputs are cloned and
    overwritten right after, with no host synchronisation of the test's in between (the library's own wait for its table
    check is on that stream).  The points are a view that starts 8 bytes into its buffer (off 16-byte alignment)."""
    L, R = 7, HC.knots(7)
    pts = HC.elements(40, 27, seed=12, r_lo=HC.R_CMB - 2e5, r_hi=HC.R_MOHO + 2e5)
    coef = HC.coefficients(L, R.size, 2, seed=12)
    vin = np.random.default_rng(3).uniform(3000.0, 9000.0, (2, 40 * 27))
    want, nout = HC.model_apply(pts, R, coef, L, mode=2, values_in=vin)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    staged = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pts, R, coef, vin)]
    torch.cuda.synchronize()
    with Context(0, stream=side.cuda_stream) as ctx, torch.cuda.stream(side):
        buffer = torch.zeros(pts.size + 1, dtype=torch.float64, device="cuda")
        tp = buffer[1:].view(pts.shape)
        assert tp.data_ptr() % 16 == 8 and tp.is_contiguous()
        tR, tc, tv = (torch.zeros(x.shape, dtype=torch.float64, device="cuda") for x in (R, coef, vin))
        tout = torch.full(want.shape, -7.0, dtype=torch.float64, device="cuda")
        count = torch.full((1,), 10, dtype=torch.int64, device="cuda")
        torch.cuda._sleep(30_000_000)
        for t, s in zip((tp, tR, tc, tv), staged):
            t.copy_(s, non_blocking=True)
        H.harmonic_model_apply(ctx, tp, tR, tc, L, mode=2, values_in=tv, out=tout, noutside=count)
        got, counted = tout.clone(), count.clone()
        tout.fill_(-7.0), count.fill_(-7)
    side.synchronize()
    assert HC.same_bits_nan(got.cpu().numpy(), want) and int(counted.item()) == 10 + nout and nout > 0


# ----------------------------------------------------------------------------------------------------- the Python layer
def _model(L=7, seed=20, names=("VSV", "VSH"), normalization="4pi", csphase=1):
    rng = np.random.default_rng(seed)
    R = HC.knots(7)
    mask = np.tril(np.ones((L + 1, L + 1), dtype=bool))
    coefficients = {p: tuple(np.where(mask, 0.01 * rng.standard_normal((R.size, L + 1, L + 1)), 0.0) for _ in range(2))
                    for p in names}
    return H.SphericalHarmonicModel(L, R, coefficients, normalization=normalization, csphase=csphase)


MODE_NUMBER = {"replace": 0, "add": 1, "relative": 2}


@pytest.mark.parametrize("mode", ("replace", "add", "relative"))
def test_import_onto_meshes(ctx, mode):
    model = _model()
    names, coef = model.packed()
    # a GLL chunk whose upper two element layers lie above the model's last knot
    chunk = synth.earth_chunk(order=2, nlat=3, nlon=3, radii=(6_000_000.0, 6_300_000.0, 6_500_000.0))
    gp = chunk["points"]
    E, Pn = gp.shape[:2]
    rng = np.random.default_rng(1)
    old = {p: rng.uniform(3000.0, 5000.0, (E, Pn)) for p in ("VSV", "VSH", "RHO")}
    mesh = GllMesh(gp, 2, {p: v.copy() for p, v in old.items()})
    vin = np.stack([old[p] for p in names]).reshape(2, -1)
    want, nout = HC.model_apply(gp, model.radii, coef, model.lmax, mode=MODE_NUMBER[mode], values_in=vin)
    assert H.import_harmonic_model(model, mesh, mode=mode, context=ctx) == nout and 0 < nout < E * Pn
    for p, w in zip(names, want):
        assert HC.same_bits_nan(mesh.element_nodal_fields[p], w.reshape(E, Pn)), p
    assert HC.same_bits_nan(mesh.element_nodal_fields["RHO"], old["RHO"])
    # hex8 nodes: P = 1
    points, conn = synth.hex_mesh(6, seed=1, lo=(4.0e6, -1e5, -1e5), hi=(6.0e6, 1e5, 1e5))
    oldh = rng.uniform(3000.0, 5000.0, (2, len(points)))
    hexmesh = HexMesh(points, conn, {"VSV": oldh[0].copy(), "QMU": oldh[1].copy()})
    wanth, nouth = HC.model_apply(points, model.radii, coef[:1], model.lmax, mode=MODE_NUMBER[mode], values_in=oldh[:1])
    assert H.import_harmonic_model(model, hexmesh, params="VSV", mode=mode, context=ctx) == nouth == 0
    assert HC.same_bits_nan(hexmesh.nodal_fields["VSV"], wanth[0]) and HC.same_bits_nan(hexmesh.nodal_fields["QMU"], oldh[1])
    # a Salvus model in memory: only the named columns change
    data = np.ascontiguousarray(np.stack([old["RHO"], old["VSH"], old["VSV"]]).transpose(1, 0, 2))
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=gp)
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=data), ["RHO", "VSH", "VSV"])
    assert H.import_harmonic_model(model, f, params=["VSV", "VSH"], mode=mode, context=ctx) == nout
    got = np.array(f["MODEL/data"][()])
    assert HC.same_bits_nan(got[:, 2, :], want[0].reshape(E, Pn)) and HC.same_bits_nan(got[:, 1, :], want[1].reshape(E, Pn))
    assert HC.same_bits_nan(got[:, 0, :], old["RHO"])
    with pytest.raises(ValueError, match="not in MODEL/data"):
        H.import_harmonic_model(_model(names=("VPV",)), f, mode=mode, context=ctx)


def test_import_refuses_before_anything_is_written(ctx):
    model = _model()
    chunk = synth.earth_chunk(order=2, nlat=2, nlon=2)
    mesh = GllMesh(chunk["points"], 2, {})
    with pytest.raises(ValueError, match="no field"):
        H.import_harmonic_model(model, mesh, mode="add", context=ctx)
    assert mesh.element_nodal_fields == {}
    assert H.import_harmonic_model(model, mesh, extend=True, context=ctx) == 0 and sorted(mesh.element_nodal_fields) == ["VSH", "VSV"]


def test_evaluate_and_the_conventions(ctx):
    """A model given as "ortho" with the Condon-Shortley phase evaluates to the bits of its "4pi" conversion."""
    ortho = _model(seed=30, normalization="ortho", csphase=-1)
    same = H.SphericalHarmonicModel(ortho.lmax, ortho.radii, {p: (ortho.cos[p], ortho.sin[p]) for p in ortho.parameters})
    pts = HC.elements(9, 27, seed=2)
    a = H.evaluate_harmonic_model(ortho, pts, context=ctx)
    b = H.evaluate_harmonic_model(same, pts, context=ctx)
    assert a.shape == (2, 9, 27) and HC.same_bits_nan(a, b)
    want, _ = HC.model_apply(pts, ortho.radii, ortho.packed()[1], ortho.lmax)
    assert HC.same_bits_nan(a.reshape(2, -1), want)
    chunk = synth.earth_chunk(order=2, nlat=2, nlon=2)
    mesh = GllMesh(chunk["points"], 2, {})
    on_mesh = H.evaluate_harmonic_model(ortho, mesh, params="VSH", extend=True, context=ctx)
    want, _ = HC.model_apply(chunk["points"], ortho.radii, ortho.packed(["VSH"])[1], ortho.lmax, extend=True)
    assert on_mesh.shape == (1,) + chunk["points"].shape[:2] and HC.same_bits_nan(on_mesh.reshape(1, -1), want)
    low = H.evaluate_harmonic_model(ortho.truncate(3), pts[:, 0, :], context=ctx)
    want, _ = HC.model_apply(pts[:, 0, :], ortho.radii, ortho.truncate(3).packed()[1], 3)
    assert low.shape == (2, 9) and HC.same_bits_nan(low, want)
