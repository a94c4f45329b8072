"""mm_convert_parameters and mm_convert_kernels on the GPU: bit for bit the NumPy statement of
tests/parametrisation_cases.py for all 20 ordered pairs -- field planes and MODEL/data-style columns, in place and out of
place, across the launch cap, with special rows (a fluid, RHO = 0, A - 2 L = 0, a negative MU, NaN, +-inf, -0.0,
denormals) --, the count of non-finite nodes, a caller's stream with caller-owned tensors, and the mesh and file drivers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parametrisation_cases as PC
from multimesh_amd import io as mio
from multimesh_amd import parametrisation as P
from multimesh_amd import synth
from multimesh_amd.api import GllMesh
from multimesh_amd.device import Context
from multimesh_amd.mesh import HexMesh

pytestmark = pytest.mark.gpu

SMALL = (0, 1, 63, 64, 65, 255, 256, 257)
BIG = (4197, 125)            # 524 625 nodes: past 2048 workgroups x 256 lanes = 524 288, so the stride loop runs
C_TOTAL = 8


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()      # before this module's context opens the device: torch then finds it whichever test runs first
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    with Context(0) as c:
        yield c


def _model(name, n, seed):
    m = PC.models(name, n, seed)
    return PC.special_rows(name, m) if n >= 16 else m


def _kernels(name, n, seed):
    rng = np.random.default_rng(seed)
    k = rng.normal(size=(len(PC.COMPONENTS[name]), n)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(len(PC.COMPONENTS[name]), n))
    if n >= 32:
        k[0, 20], k[1, 21], k[:, 22], k[-1, 23], k[0, 24] = np.nan, np.inf, 0.0, -0.0, 5e-324
    return k


_REFERENCE = {}


def _reference(a, b, n, seed=5):
    """(model in a, its conversion to b, kernels in b, their transform to a, nbad of each) -- computed once per case."""
    key = (a, b, n, seed)
    if key not in _REFERENCE:
        m, k = _model(a, n, seed), _kernels(b, n, seed + 1)
        out, kout = PC.convert(m, a, b), PC.convert_kernels(k, m, a, b)
        for x in (m, k, out, kout):
            x.setflags(write=False)
        _REFERENCE[key] = (m, out, k, kout, PC.n_bad(out), PC.n_bad(kout))
    return _REFERENCE[key]


# ------------------------------------------------------------------------------------------------ planes, the array core
@pytest.mark.parametrize("a,b", PC.PAIRS, ids=lambda x: x)
def test_planes_equal_the_statement(ctx, a, b):
    for n in SMALL:
        m, want, k, kwant, nbad, kbad = _reference(a, b, n)
        out, count = P.convert_values(m, a, b, context=ctx)
        assert isinstance(out, np.ndarray) and PC.same_bits(out, want) and count == nbad, (n, count, nbad)
        kout, count = P.convert_kernels(k, m, a, b, context=ctx)
        assert PC.same_bits(kout, kwant) and count == kbad, (n, count, kbad)
        if n >= 16:
            assert nbad > 0 and kbad > 0


@pytest.mark.parametrize("a,b", PC.PAIRS, ids=lambda x: x)
def test_planes_past_the_launch_cap(ctx, a, b):
    """[C, E, P] with E * P past the cap: the stride loop, and the split of a node's number into group and node."""
    E, Pn = BIG
    assert E * Pn > 2048 * 256
    m, want, k, kwant, nbad, kbad = _reference(a, b, E * Pn)
    shape = (-1, E, Pn)
    out, count = P.convert_values(ctx.to_device(m.reshape(shape)), a, b, context=ctx)
    assert out.shape == (len(PC.COMPONENTS[b]), E, Pn)
    assert PC.same_bits(out.numpy().reshape(want.shape), want) and count == nbad
    kout, count = P.convert_kernels(k.reshape(shape), ctx.to_device(m.reshape(shape)), a, b, context=ctx)
    assert PC.same_bits(kout.numpy().reshape(kwant.shape), kwant) and count == kbad


@pytest.mark.parametrize("a,b", PC.PAIRS, ids=lambda x: x)
def test_planes_in_place(ctx, a, b):
    """One array f64[6, n] read as ``a`` and written as ``b`` with the same strides; the kernels over their own input."""
    n = 257
    m, want, k, kwant, nbad, kbad = _reference(a, b, n)
    ca, cb = len(m), len(want)
    rest = np.random.default_rng(3).normal(size=(6, n))
    host = rest.copy()
    host[:ca] = m
    d = ctx.to_device(host)
    count = ctx.zeros((1,), np.int64)
    P.convert_on_device(ctx, a, b, n, 1, (d, 1, n, range(ca)), (d, 1, n, range(cb)), nbad=count)
    got = d.numpy()
    assert PC.same_bits(got[:cb], want) and int(count.numpy()[0]) == nbad
    assert PC.same_bits(got[max(ca, cb):], rest[max(ca, cb):])
    if cb < ca:
        assert PC.same_bits(got[cb:ca], m[cb:])                 # what the output does not cover keeps the input
    host[:cb] = k
    host[cb:] = rest[cb:]
    d = ctx.to_device(host)
    P.convert_on_device(ctx, a, b, n, 1, (ctx.to_device(m), 1, n, range(ca)), (d, 1, n, range(ca)),
                        kernels=(d, 1, n, range(cb)), nbad=count)
    assert PC.same_bits(d.numpy()[:ca], kwant) and int(count.numpy()[0]) == nbad + kbad


# ---------------------------------------------------------------------------------------------- MODEL/data-style columns
def _columns(rng, ncomp):
    return [int(c) for c in rng.permutation(C_TOTAL)[:ncomp]]


@pytest.mark.parametrize("Pn", (8, 27, 125))
@pytest.mark.parametrize("a,b", PC.PAIRS, ids=lambda x: x)
def test_model_data_columns(ctx, a, b, Pn):
    """f64[E, 8, P] arrays with the components in permuted columns: out of place into another array, and in place; the
    columns that are not written keep their bits."""
    E = 37
    n = E * Pn
    m, want, k, kwant, nbad, kbad = _reference(a, b, n)
    ca, cb = len(m), len(want)
    rng = np.random.default_rng(Pn + 7 * PC.PAIRS.index((a, b)))
    in_cols, out_cols, k_cols, ko_cols = _columns(rng, ca), _columns(rng, cb), _columns(rng, cb), _columns(rng, ca)
    gs = C_TOTAL * Pn

    def rows(values, cols):
        """f64[E, 8, P] of noise with ``values`` [C, n] in the columns ``cols``"""
        data = rng.normal(size=(E, C_TOTAL, Pn))
        data[:, cols, :] = values.reshape(len(cols), E, Pn).transpose(1, 0, 2)
        return data

    def check(got, before, cols, values):
        others = [c for c in range(C_TOTAL) if c not in cols]
        assert PC.same_bits(got[:, cols, :].transpose(1, 0, 2).reshape(len(cols), n), values)
        assert PC.same_bits(got[:, others, :], before[:, others, :])

    src, dst = rows(m, in_cols), rng.normal(size=(E, C_TOTAL, Pn))
    d_src, d_dst = ctx.to_device(src), ctx.to_device(dst)
    count = ctx.zeros((1,), np.int64)
    P.convert_on_device(ctx, a, b, E, Pn, (d_src, gs, Pn, in_cols), (d_dst, gs, Pn, out_cols), nbad=count)
    check(d_dst.numpy(), dst, out_cols, want)
    assert PC.same_bits(d_src.numpy(), src) and int(count.numpy()[0]) == nbad
    P.convert_on_device(ctx, a, b, E, Pn, (d_src, gs, Pn, in_cols), (d_src, gs, Pn, out_cols), nbad=count)   # in place
    check(d_src.numpy(), src, out_cols, want)
    assert int(count.numpy()[0]) == 2 * nbad                    # the counter was not zeroed in between

    d_model, kin, kout = ctx.to_device(rows(m, in_cols)), rows(k, k_cols), rng.normal(size=(E, C_TOTAL, Pn))
    d_kin, d_kout = ctx.to_device(kin), ctx.to_device(kout)
    model_layout = (d_model, gs, Pn, in_cols)
    P.convert_on_device(ctx, a, b, E, Pn, model_layout, (d_kout, gs, Pn, ko_cols), kernels=(d_kin, gs, Pn, k_cols))
    check(d_kout.numpy(), kout, ko_cols, kwant)
    assert PC.same_bits(d_kin.numpy(), kin)
    P.convert_on_device(ctx, a, b, E, Pn, model_layout, (d_kin, gs, Pn, ko_cols), kernels=(d_kin, gs, Pn, k_cols))
    check(d_kin.numpy(), kin, ko_cols, kwant)


# ------------------------------------------------------------------------------------------------------- special rows
def test_special_rows_are_ieee_and_counted(ctx):
    """What the specials give is what the statement gives; a fluid node stays finite in the moduli, and the count is the
    statement's, added to a counter that is not zeroed."""
    n = 300
    for a, b in ((PC.NAMES[0], PC.NAMES[1]), (PC.NAMES[1], PC.NAMES[0]), (PC.NAMES[4], PC.NAMES[3]), (PC.NAMES[3], PC.NAMES[0])):
        m, want, _, _, nbad, _ = _reference(a, b, n)
        assert 0 < nbad < n
        d, out = ctx.to_device(m), ctx.empty(want.shape, np.float64)
        count = ctx.to_device(np.array([1000], dtype=np.int64))
        for calls in (1, 2):
            P.convert_on_device(ctx, a, b, n, 1, (d, 1, n, range(len(m))), (out, 1, n, range(len(want))), nbad=count)
            assert int(count.numpy()[0]) == 1000 + calls * nbad
        assert PC.same_bits(out.numpy(), want)
    fluid = PC.convert(_reference(PC.NAMES[0], PC.NAMES[1], n)[0], PC.NAMES[0], PC.NAMES[1])[:, 0]
    assert np.isfinite(fluid).all() and fluid[1] == 0.0


def test_what_the_library_refuses_is_a_value_error(ctx):
    d = ctx.zeros((6, 64), np.float64)
    planes = (d, 1, 64, range(3))
    with pytest.raises(ValueError, match="from == to"):
        P.convert_on_device(ctx, "iso_lame", "iso_lame", 64, 1, planes, planes)
    with pytest.raises(ValueError, match="two output columns are equal"):
        P.convert_on_device(ctx, "iso_lame", "iso_bulk", 64, 1, planes, (d, 1, 64, [0, 1, 1]))
    with pytest.raises(ValueError, match="overlaps"):
        P.convert_on_device(ctx, "iso_lame", "iso_bulk", 32, 1, (d, 1, 32, range(3)), (d.reshape(384).rows(8, 384), 1, 32, range(3)))
    with pytest.raises(ValueError, match=r"must be \[3, \.\.\.\]"):
        P.convert_values(np.zeros((6, 4)), "iso_lame", "iso_bulk", context=ctx)
    assert not d.numpy().any()


# ------------------------------------------------------------------------------- a caller's stream and caller's tensors
def test_on_a_callers_stream_with_the_callers_tensors(torch):
    """Late producer, early consumer, as tests/test_caller_stream_gpu.py: under a side stream the inputs hold zeros while
    the stream spins, the true values are copied in on that stream, the library is called and its outputs are cloned and
    overwritten right after, with no host synchronisation of the test's in between.  The model is a view that starts 8
    bytes into its buffer (off 16-byte alignment)."""
    a, b = "vti_velocity", "iso_velocity"
    n = 4099
    m, want, k, kwant, nbad, kbad = _reference(a, b, n)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    staged_m, staged_k = torch.from_numpy(m.copy()).cuda(), torch.from_numpy(k.copy()).cuda()
    torch.cuda.synchronize()
    with Context(0, stream=side.cuda_stream) as ctx, torch.cuda.stream(side):
        buffer = torch.zeros(m.size + 1, dtype=torch.float64, device="cuda")
        tm = buffer[1:].view(m.shape)
        assert tm.data_ptr() % 16 == 8 and tm.is_contiguous()
        tk = torch.zeros(k.shape, dtype=torch.float64, device="cuda")
        tout = torch.full(want.shape, -7.0, dtype=torch.float64, device="cuda")
        tkout = torch.full(m.shape, -7.0, dtype=torch.float64, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda._sleep(30_000_000)
        tm.copy_(staged_m, non_blocking=True)
        tk.copy_(staged_k, non_blocking=True)
        dm, dk = ctx.asdevice(tm, np.float64), ctx.asdevice(tk, np.float64)
        dcount = ctx.asdevice(count, np.int64)
        P.convert_on_device(ctx, a, b, n, 1, (dm, 1, n, range(6)), (ctx.asdevice(tout, np.float64), 1, n, range(3)), nbad=dcount)
        P.convert_on_device(ctx, a, b, n, 1, (dm, 1, n, range(6)), (ctx.asdevice(tkout, np.float64), 1, n, range(6)),
                            kernels=(dk, 1, n, range(3)), nbad=dcount)
        got, kgot, counted = tout.clone(), tkout.clone(), count.clone()
        tout.fill_(-7.0), tkout.fill_(-7.0), count.fill_(-7)
        out2, nbad2 = P.convert_values(tm, a, b, context=ctx)            # the array core: a device input, a device output
        assert nbad2 == nbad and PC.same_bits(out2.numpy(), want)
    side.synchronize()
    assert PC.same_bits(got.cpu().numpy(), want) and PC.same_bits(kgot.cpu().numpy(), kwant)
    assert int(counted.item()) == nbad + kbad


# ------------------------------------------------------------------------------------------------------------ the drivers
def test_convert_model_on_meshes(ctx):
    order = 2
    gp = synth.gll_mesh(4, order, seed=2)
    E, Pn = gp.shape[:2]
    m = PC.models("iso_velocity", E * Pn, seed=8)
    q = np.random.default_rng(1).uniform(50.0, 600.0, (2, E, Pn))
    fields = dict(zip(("VP", "VS", "RHO"), m.reshape(3, E, Pn)), QKAPPA=q[0], QMU=q[1])
    mesh = GllMesh(gp, order, fields)
    assert P.convert_model(mesh, "vti_velocity", context=ctx) == 0
    want = PC.convert(m, "iso_velocity", "vti_velocity")
    assert sorted(mesh.element_nodal_fields) == sorted(PC.COMPONENTS["vti_velocity"] + ("QKAPPA", "QMU"))
    for name, w in zip(PC.COMPONENTS["vti_velocity"], want):
        assert PC.same_bits(mesh.element_nodal_fields[name], w.reshape(E, Pn)), name
    assert PC.same_bits(mesh.element_nodal_fields["VPV"], m[0].reshape(E, Pn))        # the embed keeps the values
    assert PC.same_bits(mesh.element_nodal_fields["QMU"], q[1])
    assert P.convert_model(mesh, "iso_bulk", context=ctx) == 0                        # detected: vti_velocity
    back = PC.convert(want, "vti_velocity", "iso_bulk")
    assert sorted(mesh.element_nodal_fields) == sorted(("KAPPA", "MU", "RHO", "QKAPPA", "QMU"))
    assert PC.same_bits(mesh.element_nodal_fields["KAPPA"], back[0].reshape(E, Pn))

    points, conn = synth.hex_mesh(6, seed=1)
    mh = PC.models("iso_lame", len(points), seed=9)
    mh[1, 5] = 0.0                                                                    # a fluid node: VS = 0, finite
    mh[2, 6] = 0.0                                                                    # no density: not finite
    hexmesh = HexMesh(points, conn, dict(zip(("LAMBDA", "MU", "RHO"), mh), QMU=np.full(len(points), 300.0)))
    wanth = PC.convert(mh, "iso_lame", "iso_velocity")
    assert P.convert_model(hexmesh, "iso_velocity", frm="iso_lame", context=ctx) == PC.n_bad(wanth) == 1
    assert sorted(hexmesh.nodal_fields) == ["QMU", "RHO", "VP", "VS"]
    for name, w in zip(("VP", "VS", "RHO"), wanth):
        assert PC.same_bits(hexmesh.nodal_fields[name], w), name
    assert hexmesh.nodal_fields["VS"][5] == 0.0
    with pytest.raises(ValueError, match="no complete parametrisation"):
        P.convert_model(HexMesh(points, conn, {"VP": mh[0]}), "iso_lame", context=ctx)


def test_convert_model_file_in_memory(ctx):
    order = 2
    gp = synth.gll_mesh(3, order, seed=4)
    E, Pn = gp.shape[:2]
    rng = np.random.default_rng(12)
    m = PC.models("iso_velocity", E * Pn, seed=10).reshape(3, E, Pn)
    q = rng.uniform(50.0, 600.0, (2, E, Pn))
    data = np.ascontiguousarray(np.concatenate([m, q]).transpose(1, 0, 2))           # [E, 5, P]
    f = mio.MemoryH5()
    f.create_dataset("MODEL/coordinates", data=gp)
    mio.set_dimension_labels(f.create_dataset("MODEL/data", data=data), ["VP", "VS", "RHO", "QKAPPA", "QMU"])
    assert P.convert_model_file(f, "vti_velocity", context=ctx) == 0
    ds = f["MODEL/data"]
    assert mio.dimension_labels(ds, 1) == ["VPV", "VPH", "VSV", "VSH", "ETA", "RHO", "QKAPPA", "QMU"]
    assert ds.shape == (E, 8, Pn)
    got = np.array(ds[()])
    core, nbad = P.convert_values(m, "iso_velocity", "vti_velocity", context=ctx)
    assert nbad == 0 and PC.same_bits(got[:, :6, :].transpose(1, 0, 2), core)
    assert PC.same_bits(core, PC.convert(m, "iso_velocity", "vti_velocity"))
    assert PC.same_bits(got[:, 6, :], q[0]) and PC.same_bits(got[:, 7, :], q[1])
    assert P.convert_model_file(f, "iso_lame", frm="vti_velocity", context=ctx) == 0
    assert mio.dimension_labels(f["MODEL/data"], 1) == ["LAMBDA", "MU", "RHO", "QKAPPA", "QMU"]
    want = PC.convert(core, "vti_velocity", "iso_lame")
    assert PC.same_bits(np.array(f["MODEL/data"][()])[:, :3, :].transpose(1, 0, 2), want)
    assert PC.same_bits(np.array(f["MODEL/data"][()])[:, 4, :], q[1])


# ------------------------------------------------------------------------------------------------- guarded allocations
_GUARDED = r"""
import sys
import numpy as np
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import parametrisation_cases as PC
from multimesh_amd import parametrisation as P
from multimesh_amd.device import Context

ctx = Context(0)
pairs = (("vti_velocity", "iso_velocity"), ("iso_velocity", "vti_velocity"), ("iso_bulk", "vti_love"), ("vti_love", "vti_velocity"))
for a, b in pairs:
    ca, cb = len(PC.COMPONENTS[a]), len(PC.COMPONENTS[b])
    for E, Pn in ((512, 8), (512, 27), (512, 125), (1, 1), (2, 1), (101, 1), (1, 27), (2, 125), (101, 8)):
        n = E * Pn                                                     # 512 elements: every array ends on a page boundary
        m = PC.models(a, n, seed=n)
        k = np.random.default_rng(n).normal(size=(cb, n))
        want, kwant = PC.convert(m, a, b), PC.convert_kernels(k, m, a, b)
        out, nbad = P.convert_values(m.reshape(ca, E, Pn), a, b, context=ctx)
        assert nbad == 0 and PC.same_bits(out.reshape(cb, n), want), (a, b, E, Pn)
        kout, _ = P.convert_kernels(k.reshape(cb, E, Pn), m.reshape(ca, E, Pn), a, b, context=ctx)
        assert PC.same_bits(kout.reshape(ca, n), kwant), (a, b, E, Pn)
        # rows [E, C, P] with exactly the parametrisation's columns: the last column's last run ends the allocation
        src = ctx.to_device(np.ascontiguousarray(m.reshape(ca, E, Pn).transpose(1, 0, 2)))
        dst = ctx.empty((E, cb, Pn), np.float64)
        P.convert_on_device(ctx, a, b, E, Pn, (src, ca * Pn, Pn, range(ca)), (dst, cb * Pn, Pn, range(cb)))
        assert PC.same_bits(dst.numpy().transpose(1, 0, 2).reshape(cb, n), want), (a, b, E, Pn)
        kin = ctx.to_device(np.ascontiguousarray(k.reshape(cb, E, Pn).transpose(1, 0, 2)))
        kdst = ctx.empty((E, ca, Pn), np.float64)
        P.convert_on_device(ctx, a, b, E, Pn, (src, ca * Pn, Pn, range(ca)), (kdst, ca * Pn, Pn, range(ca)),
                            kernels=(kin, cb * Pn, Pn, range(cb)))
        assert PC.same_bits(kdst.numpy().transpose(1, 0, 2).reshape(ca, n), kwant), (a, b, E, Pn)
print("ok")
"""


def test_parametrisation_under_guarded_allocations():
    """MM_GUARD_ALLOC=1 (multimesh_amd/csrc/mm_context.hip): every array ends at the end of its mapping, so an access past
    one would fault at once.  A net, not a provocation: ordinary models, sizes whose arrays end on a page boundary and sizes
    of one, two and 101 groups.  The switch is read once per process, so the checks run in a child process, as in
    tests/test_precondition_guarded_gpu.py."""
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _GUARDED], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
