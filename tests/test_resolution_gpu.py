"""mm_gll_resolution and mm_arg_extreme on the GPU, bit for bit against the NumPy statements of tests/resolution_cases.py:
every tile size at the element counts around a tile, blocks that stride, thin Earth-scale elements with a fluid layer, the
validity rules, the public functions of multimesh_amd.resolution, a caller's stream and tensors, argument mistakes."""
import numpy as np
import pytest
import torch   # (before the library is loaded, as in a run of the whole suite: its HIP runtime is the process's first)

import resolution_cases as RC
from multimesh_amd import resolution, synth
from multimesh_amd.api import GllMesh
from multimesh_amd.boundary import EXODUS_TO_TENSOR
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def _mesh(order, dim, nelem, seed=5):
    """nelem elements of a jittered synth.gll_mesh"""
    side = 1
    while side ** dim < nelem:
        side += 1
    gp = synth.gll_mesh(max(side, 1) + 1, order, seed=seed, jitter=0.25, dim=dim)
    return np.ascontiguousarray(gp[:nelem])


def _check(ctx, gp, order, fast=None, slow=None, what=None):
    """One call with and one without node_h against the statement; returns the statement's rows."""
    ref, ref_info, ref_h = RC.resolution(gp, order, fast, slow)
    out, info, h = ctx.gll_resolution(order, gp, fast=fast, slow=slow, want_node_spacing=True)
    out2, info2 = ctx.gll_resolution(order, gp, fast=fast, slow=slow)
    out, out2 = out.numpy(), out2.numpy()
    assert out.shape == ref.shape and RC.same_bits(out, ref), what
    assert RC.same_bits(h.numpy(), ref_h), what
    assert info.numpy().tolist() == ref_info.tolist() == info2.numpy().tolist(), what
    assert RC.same_bits(out2, out), what                      # node_h requested or not: the same rows
    return ref, ref_info


@pytest.mark.parametrize("order,dim,P,tile", RC.TILES)
def test_every_tile_size_around_a_tile(ctx, order, dim, P, tile):
    assert P == (order + 1) ** dim and tile == 256 // P
    full = _mesh(order, dim, 3 * tile + 1)
    fast, slow = RC.velocities(full, 2, 11), RC.velocities(full, 2, 12, lo=1500.0, hi=4500.0)
    for nelem in RC.element_counts(tile):
        gp = np.ascontiguousarray(full[:nelem])
        f, s = np.ascontiguousarray(fast[:, :nelem]), np.ascontiguousarray(slow[:, :nelem])
        _check(ctx, gp, order, what=(nelem, "sizes"))
        _check(ctx, gp, order, f, s, what=(nelem, "2 fast, 2 slow"))


def test_blocks_that_stride_over_more_than_one_tile(ctx):
    nelem = 2048 * 32 + 5
    gp = _mesh(1, 3, nelem)
    assert gp.shape == (nelem, 8, 3)
    fast = RC.velocities(gp, 1, 13)
    ref, _ = _check(ctx, gp, 1, fast, what="2048 * 32 + 5 elements")
    value, index, nvalid = ctx.arg_extreme(ref[3])
    assert int(index.numpy()[0]) == int(np.argmin(ref[3])) and int(nvalid.numpy()[0]) == nelem


@pytest.fixture(scope="module")
def chunks():
    """order -> (points of a thin, Earth-scale chunk; its layer per element)"""
    out = {}
    for order in (2, 4):
        c = synth.earth_chunk(order, nlat=3, nlon=4, radii=(3_480_000.0, 3_500_000.0, 3_530_000.0, 3_531_000.0),
                              nrad=(1, 2, 1), ellipticity=3.3e-3, topography=3e-4)
        out[order] = (c["points"], c["layer"])
    return out


@pytest.mark.parametrize("order", [2, 4])
def test_an_earth_chunk_with_a_fluid_layer(ctx, chunks, order):
    gp, layer = chunks[order]
    fluid = layer == 1.0
    assert fluid.any() and not fluid.all()
    fast, slow = RC.velocities(gp, 2, 21, lo=8000.0, hi=13000.0), RC.velocities(gp, 2, 22, lo=4000.0, hi=7000.0)
    slow[:, fluid] = 0.0
    ref, info = _check(ctx, gp, order, fast, slow, what="TTI-like")
    assert info.tolist() == [0, 0]
    # the fluid elements are resolved by their P wavelength
    assert np.array_equal(ref[4][fluid], ref[2][fluid] / fast.min(axis=0).min(axis=1)[fluid])
    _check(ctx, gp, order, fast[:1], slow[:1], what="ISO-like")
    _check(ctx, gp, order, fast[:1], what="nslow = 0")
    _check(ctx, gp, order, what="sizes")


def test_validity(ctx):
    gp = _mesh(2, 3, 30)
    fast, slow = RC.velocities(gp, 2, 31), RC.velocities(gp, 1, 32)
    gp[3, 26, 2] = np.nan
    fast[1, 9, 0] = np.inf
    fast[0, 10, 13] = 0.0
    slow[0, 20, 26] = -1.0
    gp[25, 14] = gp[25, 13]                                    # two coincident nodes: valid, step = 0
    ref, info = _check(ctx, gp, 2, fast, slow, what="validity")
    assert info.tolist() == [1, 4]
    assert np.isnan(ref[:, 3]).all() and np.isnan(ref[3:, [9, 10, 20]]).all() and np.isfinite(ref[:3, [9, 10, 20]]).all()
    assert ref[0, 25] == 0.0 and ref[3, 25] == 0.0
    valid = np.setdiff1d(np.arange(30), [3, 9, 10, 20])
    assert np.isfinite(ref[:, valid]).all()
    ref3, info3 = _check(ctx, gp, 2, what="validity, sizes only")
    assert info3.tolist() == [1, 1]


def _rows(n, nrows, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(nrows, n))
    if n >= 255:
        v[:, ::17] = np.nan
        v[0, 7], v[0, n - 3] = -np.inf, np.inf
    return v


@pytest.mark.parametrize("n", RC.ARG_EXTREME_N)
@pytest.mark.parametrize("nrows", [1, 3])
def test_arg_extreme(ctx, n, nrows):
    v = _rows(n, nrows, 100 + n)
    if n > 1 and nrows == 3:
        v[1] = np.nan                                           # a row that is all NaN
        v[2] = 2.5                                              # a row that is all equal: index 0
    for want_max in (False, True):
        ref = RC.arg_extreme(v, want_max)
        for _ in range(2):                                      # equal on two consecutive runs
            got = ctx.arg_extreme(v if nrows > 1 else v[0], want_max=want_max)
            value, index, nvalid = (g.numpy() for g in got)
            assert RC.same_bits(value, ref[0]) and np.array_equal(index, ref[1]) and np.array_equal(nvalid, ref[2]), (n, want_max)
    if n > 1 and nrows == 3:
        assert ref[1].tolist()[1:] == [-1, 0]


@pytest.mark.parametrize("n", [2, 257, 100_003])
def test_arg_extreme_ties_at_both_ends(ctx, n):
    for zeros in ((-0.0, 0.0), (0.0, -0.0)):
        for want_max in (False, True):
            v = np.full(n, -1.0 if want_max else 1.0)           # the zeros are the extreme; they compare equal
            v[0], v[-1] = zeros
            value, index, nvalid = (g.numpy() for g in ctx.arg_extreme(v, want_max=want_max))
            ref = RC.arg_extreme(v, want_max)
            assert index.tolist() == [0] == ref[1].tolist() and nvalid.tolist() == [n]
            assert RC.same_bits(value, ref[0]) and np.signbit(value[0]) == np.signbit(zeros[0])
            v[0] = np.nan                                       # the tie's first end gone: the other end
            assert ctx.arg_extreme(v, want_max=want_max)[1].numpy().tolist() == [n - 1]


def test_the_public_functions(ctx, chunks):
    gp, layer = chunks[2]
    fast, slow = RC.velocities(gp, 3, 41, lo=8000.0, hi=13000.0), RC.velocities(gp, 2, 42, lo=4000.0, hi=7000.0)
    slow[:, layer == 1.0] = 0.0
    fields = {"VPV": fast[0], "VPH": fast[1], "VP": fast[2], "VSV": slow[0], "VSH": slow[1], "RHO": np.ones(gp.shape[:2])}
    mesh = GllMesh(gp, 2, fields)
    ref, _ = RC.resolution(gp, 2, fast[[2, 0, 1]], slow)[:2]   # the order of FAST_NAMES; a maximum has none
    spacing, emin, emax, ninvalid = resolution.element_sizes(mesh, context=ctx)
    assert RC.same_bits(np.stack([spacing, emin, emax]), ref[:3]) and ninvalid == 0
    dt, element, step, ninvalid = resolution.time_step(mesh, courant=0.55, context=ctx)
    assert dt == 0.55 * np.nanmin(ref[3]) and element == np.nanargmin(ref[3]) and RC.same_bits(step, ref[3]) and ninvalid == 0
    period, element, period_e = resolution.resolved_period(mesh, elements_per_wavelength=1.5, context=ctx)
    assert period == 1.5 * np.nanmax(ref[4]) and element == np.nanargmax(ref[4]) and RC.same_bits(period_e, ref[4])
    epw, least, element, nbelow = resolution.elements_per_wavelength(mesh, 20.0, minimum=2.5, context=ctx)
    assert RC.same_bits(epw, 20.0 / ref[4]) and least == 20.0 / np.nanmax(ref[4]) and element == np.nanargmax(ref[4])
    assert nbelow == int((20.0 / ref[4] < 2.5).sum())
    check = resolution.check_model(mesh, 20.0, courant=0.55, elements_per_wavelength=1.5, context=ctx)
    assert (check.dt, check.dt_element, check.resolved_period, check.period_element) == (dt, np.nanargmin(ref[3]), period, element)
    assert RC.same_bits(np.stack([check.spacing, check.edge_min, check.edge_max, check.step, check.period_e]), ref)
    assert check.nbelow == int((20.0 / ref[4] < 1.5).sum()) and check.ninvalid_model == 0 and check.ok == (check.nbelow == 0)
    assert "time step" in str(check) and "resolved period" in str(check)
    # named fields and arrays
    iso = resolution.time_step(mesh, fast="VP", context=ctx)
    assert RC.same_bits(iso[2], RC.resolution(gp, 2, fast[2:3])[0][3])
    arr = resolution.resolved_period(GllMesh(gp, 2), fast=fast[:1], slow=slow[0], context=ctx)
    assert RC.same_bits(arr[2], RC.resolution(gp, 2, fast[:1], slow[:1])[0][4])


def test_a_hex_mesh_equals_its_order_1_form(ctx):
    pts, conn = synth.hex_mesh(6, seed=3)
    rng = np.random.default_rng(5)
    vp, vs = rng.uniform(5000.0, 8000.0, len(pts)), rng.uniform(2500.0, 4500.0, len(pts))
    hexm = HexMesh(pts, conn, {"VP": vp, "VS": vs})
    tensor = conn[:, EXODUS_TO_TENSOR]
    gll = GllMesh(pts[tensor], 1, {"VP": vp[tensor], "VS": vs[tensor]})
    a, b = resolution.check_model(hexm, 1e-4, context=ctx), resolution.check_model(gll, 1e-4, context=ctx)
    ref = RC.resolution(pts[tensor], 1, vp[tensor][None], vs[tensor][None])[0]
    for name, row in zip(("spacing", "edge_min", "edge_max", "step", "period_e"), ref):
        assert RC.same_bits(getattr(a, name), row) and RC.same_bits(getattr(b, name), row), name
    assert (a.dt, a.dt_element, a.resolved_period, a.period_element) == (b.dt, b.dt_element, b.resolved_period, b.period_element)
    assert RC.same_bits(resolution.time_step(hexm, fast=vp, context=ctx)[2], ref[3])      # nodal values, gathered


def test_a_callers_stream_and_tensors():
    """The late producer, early consumer pattern of tests/test_caller_stream_gpu.py: under a side stream the inputs hold
    zeros while the stream spins, the true inputs are copied in on that stream, the library is called, and its outputs are
    read through the context (a copy on its stream) with no synchronisation of the test's in between.  A launch that is not
    ordered on the context's stream reads the zeros."""
    gp = _mesh(2, 3, 3 * 9 + 1)
    fast, slow = RC.velocities(gp, 2, 51), RC.velocities(gp, 2, 52, lo=1500.0, hi=4500.0)
    ref, ref_info, ref_h = RC.resolution(gp, 2, fast, slow)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    staging = [torch.from_numpy(a).cuda() for a in (gp, fast, slow)]
    torch.cuda.synchronize()
    with Context(0, stream=side.cuda_stream) as c:
        with torch.cuda.stream(side):
            late = [torch.zeros_like(t) for t in staging]
            torch.cuda._sleep(10_000_000)                      # a few ms: far longer than the calls below
            for t, s in zip(late, staging):
                t.copy_(s, non_blocking=True)
            out, info, h = c.gll_resolution(2, late[0], fast=late[1], slow=late[2], want_node_spacing=True)
            value, index, nvalid = c.arg_extreme(out.rows(3, 4))
            got = [a.numpy() for a in (out, info, h, value, index, nvalid)]
        side.synchronize()
    assert RC.same_bits(got[0], ref) and got[1].tolist() == ref_info.tolist() and RC.same_bits(got[2], ref_h)
    want = RC.arg_extreme(ref[3])
    assert RC.same_bits(got[3], want[0]) and np.array_equal(got[4], want[1]) and np.array_equal(got[5], want[2])


def test_argument_mistakes(ctx):
    gp = _mesh(2, 3, 4)
    fast = RC.velocities(gp, 1, 61)
    with pytest.raises(ValueError, match="slow velocities need a fast one"):
        ctx.gll_resolution(2, gp, slow=fast)
    with pytest.raises(ValueError, match="order must be 1, 2 or 4"):
        ctx.gll_resolution(3, np.zeros((2, 64, 3)))
    with pytest.raises(ValueError, match=r"gll_points must be \[nelem"):
        ctx.gll_resolution(2, gp[:, :8])
    with pytest.raises(ValueError, match=r"fast must be \[C, E, P\]"):
        ctx.gll_resolution(2, gp, fast=fast[:, :3])
    with pytest.raises(ValueError, match=r"slow must be \[C, E, P\]"):
        ctx.gll_resolution(2, gp, fast=fast, slow=np.ones((1, 4, 8)))
    with pytest.raises(ValueError, match="nrows must lie in"):
        ctx.arg_extreme(np.zeros((70000, 1)))
    out, info = ctx.gll_resolution(2, gp, fast=fast)            # the context works on
    assert RC.same_bits(out.numpy(), RC.resolution(gp, 2, fast)[0])
