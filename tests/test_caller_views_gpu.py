"""Every device entry point on caller tensors that start part-way into a buffer, off 16-byte alignment.

``include/multimesh_hip.h`` promises a caller's array the alignment of its elements and no more, and ``Context.asdevice``
wraps any contiguous torch tensor by its ``data_ptr()``.  Here every caller tensor of a call -- inputs, outputs, arrays
updated in place -- is a view ``buf[B + 1 : B + 1 + n]`` of a flat buffer of its own, ``[front border | payload | back
border]`` with B = 32 elements: the payload starts 8 bytes past a 16-byte boundary for f64 / i64, 4 for i32, 1 for u8
(asserted, so the test cannot pass by accident on aligned memory).  A control runs the same call on ``buf[B : B + n]``,
aligned and with the same borders, which tells a border failure from an alignment failure.  The borders hold a bit pattern
no kernel produces (a quiet NaN with payload 0x7ff8dead0000beef, 0x5a5a... for integers), the outputs the sentinel -7.

After the call and one stream synchronise both borders of every buffer, inputs included, must be bit-identical to what
was written, and the results must equal, bit for bit, the same call on NumPy inputs (the library's own 256-byte-aligned
allocations) and the CPU statement as the case's table compares it.  No tolerance is introduced.

The 64 elements of border see a stray write within 256 B of an array (512 B for 8-byte elements) on either side.  Overruns
farther past the end remain the job of the MM_GUARD_ALLOC child-process tests (test_guarded_gpu.py and its siblings).

Which accesses of the library touch a caller's pointer 16 bytes at a time, and how each is made well defined at 8-byte
alignment, is the table in DESIGN.md section 1 ("Caller pointers and alignment")."""
import ctypes as C
import types

import numpy as np
import pytest

import boundary_cases as BC
import resolution_cases as RS
import transpose_cases as T
from multimesh_amd import helpers as H
from multimesh_amd import synth
from multimesh_amd.device import Context, DeviceArray
from oracle import oracle as O
from test_caller_stream_gpu import (CASES, SENTINEL, Case, _bits, _close12, _equal, _flatten, _hex8, _lazy, _run_reference,
                                    _same_as)

pytestmark = pytest.mark.gpu

B = 32
NAN_BITS = 0x7FF8DEAD0000BEEF
_FILL = {8: 0x5A5A5A5A5A5A5A5A, 4: 0x5A5A5A5A, 1: 0x5A}
N_FREE = 3 * 4096 + 5                    # two waves' worth of 4096-target workgroups and a ragged tail


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


# ------------------------------------------------------------------------------------------------------- buffers
class Buffers:
    """The flat buffers of one call and their borders as written."""

    def __init__(self, torch, misaligned):
        self.torch, self.shift, self.bufs = torch, 1 if misaligned else 0, []

    def view(self, shape, dtype, fill=None):
        """A payload view of ``shape`` in a new buffer; ``fill``: a NumPy array to hold, or None: the sentinel."""
        torch = self.torch
        dtype = np.dtype(dtype)
        tdtype = getattr(torch, "bool" if dtype == np.bool_ else dtype.name)
        n = int(np.prod(shape, dtype=np.int64))
        buf = torch.empty(2 * B + 1 + n, dtype=tdtype, device="cuda")
        raw = buf.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[dtype.itemsize])
        pattern = NAN_BITS if dtype == np.float64 else _FILL[dtype.itemsize]
        raw.fill_(pattern if pattern < 1 << 63 else pattern - (1 << 64))
        lo = B + self.shift
        view = buf[lo:lo + n].view(tuple(int(s) for s in shape))
        if fill is None:
            view.fill_(SENTINEL)
        else:
            view.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=dtype)).cuda().view(view.shape))
        assert view.is_contiguous() and buf.data_ptr() % 16 == 0
        assert view.data_ptr() % 16 == (self.shift * dtype.itemsize) % 16            # 8 for f64 / i64, 4 for i32, 1 for u8
        self.bufs.append((raw, lo, n, raw[:lo].clone(), raw[lo + n:].clone()))
        return view

    def check_borders(self, what):
        torch = self.torch
        torch.cuda.synchronize()
        for j, (raw, lo, n, front, back) in enumerate(self.bufs):
            assert torch.equal(raw[:lo], front), (what, "front border of buffer", j)
            assert torch.equal(raw[lo + n:], back), (what, "back border of buffer", j)


def _numpy(t):
    return t.cpu().numpy().copy()


# --------------------------------------------------------------------------------------- the stream table, on views
def _run_on_views(torch, ctx, case, misaligned, what):
    """The call with every caller tensor a view of its own buffer -> results as NumPy / numbers."""
    bufs = Buffers(torch, misaligned)
    a = {k: bufs.view(v.shape, v.dtype, v) for k, v in case.inputs.items()}
    o = {k: bufs.view(shape, dt) for k, (shape, dt) in case.outs.items()}
    args = types.SimpleNamespace(**a)
    torch.cuda.synchronize()
    results = _flatten(case.call(ctx, args, types.SimpleNamespace(**o)))
    ctx.synchronize()
    watched = dict(o, **{k: a[k] for k in case.inout})
    out, taken = [], set()
    for r in results:
        if isinstance(r, str):
            taken.add(r)
            out.append(_numpy(a[r]))
        elif isinstance(r, DeviceArray):
            names = [k for k, t in watched.items() if t.data_ptr() == r.ptr]
            if names:
                taken.add(names[0])
                flat = _numpy(watched[names[0]]).reshape(-1)
                out.append(np.ascontiguousarray(flat[:r.size]).reshape(r.shape))
            else:
                out.append(r.numpy())
        else:
            out.append(r)
    assert taken == set(watched), f"the call did not return the caller's arrays {sorted(set(watched) - taken)} themselves"
    bufs.check_borders(what)
    for k, v in case.inputs.items():                        # an input the call does not update still holds its values
        if k not in case.inout:
            assert _bits(_numpy(a[k]).reshape(v.shape), v), (what, "input changed", k)
    del args
    return out


# ------------------------------------------------------------ this file's own cases: entry points the stream table lacks
# Straight at the ABI where the Python layer allocates an output itself: every output is then a caller's view as well.
def _abi_case(inputs, outs, run, expect, inout=(), compare=None):
    """``run(ctx, h, p, dst)``: ``p(name)`` is the device pointer of an input, ``dst(name)`` the DeviceArray of an output
    (the caller's view, or an allocation of the library's in the NumPy-input run)."""
    def call(ctx, a, o):
        a.keep = []

        def arr(name):
            x = getattr(a, name)
            d = ctx.asdevice(x, np.asarray(inputs[name]).dtype)
            a.keep.append(d)
            return d

        def dst(name):
            shape, dt = outs[name]
            t = getattr(o, name)
            d = ctx.asdevice(t, dt) if t is not None else ctx.to_device(np.full(shape, SENTINEL, dtype=dt))
            a.keep.append(d)
            return d

        return run(ctx, ctx.handle, lambda name: arr(name).ptr, dst)

    return Case(inputs, call, expect, outs=outs, inout=inout, compare=compare)


def _ok(ctx, rc):
    assert rc >= 0, (rc, ctx.lib.mm_last_error())
    return int(rc)


UP = (0.0, 0.0, 1.0)


@_lazy
def _boundary():
    d = types.SimpleNamespace()
    d.gp = synth.gll_mesh(6, 2, seed=2)                     # 125 elements
    d.corners = np.ascontiguousarray(d.gp[:, BC.corner_nodes(2)])
    d.ids, d.nnodes = BC.corner_ids(d.corners)
    d.faces, d.nonmanifold = BC.boundary_faces(d.ids)
    d.side = BC.classify(d.corners, d.faces, up=UP)
    return d


def _case_boundary_faces():
    d = _boundary()
    E = len(d.ids)

    def run(ctx, h, p, dst):
        faces, info = dst("faces"), dst("info")
        nb = _ok(ctx, ctx.lib.mm_boundary_faces(h, p("ids"), E, d.nnodes, faces.ptr, info.ptr))
        return faces.rows(0, nb), info, nb

    return _abi_case(dict(ids=d.ids), dict(faces=((6 * E,), np.int64), info=((1,), np.int64)), run,
                     lambda ref: [d.faces, np.array([d.nonmanifold]), len(d.faces)], compare=_equal)


def _case_boundary_classify():
    d = _boundary()

    def run(ctx, h, p, dst):
        side = dst("side")
        _ok(ctx, ctx.lib.mm_boundary_classify(h, p("corners"), len(d.corners), p("faces"), len(d.faces), 0, *UP, 0.5, side.ptr))
        return side

    return _abi_case(dict(corners=d.corners, faces=d.faces), dict(side=((len(d.faces),), np.int32)), run,
                     lambda ref: [d.side], compare=_equal)


def _case_boundary_nodes():
    d = _boundary()
    mask = 0b101

    def run(ctx, h, p, dst):
        out = dst("out")
        n = _ok(ctx, ctx.lib.mm_boundary_nodes(h, p("points"), len(d.gp), 2, p("faces"), p("side"), len(d.faces), mask, out.ptr))
        return out.rows(0, n), n

    def expect(ref):
        nodes = BC.boundary_nodes(d.gp, 2, d.faces, d.side, mask)
        assert 0 < len(nodes) < 9 * len(d.faces)
        return [nodes, len(nodes)]

    return _abi_case(dict(points=d.gp, faces=d.faces, side=d.side), dict(out=((9 * len(d.faces), 3), np.float64)), run, expect)


def _case_cutoff_distance():
    rng = np.random.default_rng(11)
    src, pts, cutoff = rng.uniform(0.0, 1.0, (1001, 3)), rng.uniform(-0.5, 1.5, (N_FREE, 3)), 0.06
    pts[:10] = src[:10]
    pts[10, 0], pts[11, 2] = np.nan, np.inf

    def run(ctx, h, p, dst):
        dist = dst("dist")
        return dist, _ok(ctx, ctx.lib.mm_cutoff_distance(h, p("pts"), len(pts), p("src"), len(src), cutoff, dist.ptr))

    return _abi_case(dict(pts=pts, src=src), dict(dist=((len(pts),), np.float64)), run,
                     lambda ref: list(BC.cutoff_distance(pts, src, cutoff)))


def _case_distance_taper():
    rng = np.random.default_rng(8)
    n = N_FREE
    d = rng.uniform(0.0, 3.0, n)
    d[:7] = [0.0, 1.0, 2.0, 1.0 - 2 ** -53, 2.0 + 2 ** -51, 1.5, 3.0]
    a, b, elem = rng.normal(size=(3, n)), rng.normal(size=(3, n)), rng.integers(-1, 5, n)
    a[:, elem < 0] = np.nan                                 # a row that was not located never leaks

    def run(ctx, h, p, dst):
        out, weight = dst("out"), dst("weight")
        count = _ok(ctx, ctx.lib.mm_distance_taper(h, p("d"), n, 1.0, 2.0, 3, p("a"), p("b"), p("elem"), out.ptr, weight.ptr))
        return out, count, weight

    def expect(ref):
        out, w, count = BC.distance_taper(d, 1.0, 2.0, a, b=b, elem=elem)
        return [out, count, w]

    return _abi_case(dict(d=d, a=a, b=b, elem=elem), dict(out=((3, n), np.float64), weight=((n,), np.float64)), run, expect)


def _case_gll_resolution(want_node_h):
    gp = synth.gll_mesh(6, 2, seed=5, jitter=0.25)
    fast, slow = RS.velocities(gp, 2, 11), RS.velocities(gp, 2, 12, lo=1500.0, hi=4500.0)
    slow[:, ::7] = 0.0                                      # fluid elements: resolved by the least fast velocity
    gp[3, 5, 1] = np.nan                                    # one geometry-invalid element
    E, P = gp.shape[:2]
    outs = dict(out=((5, E), np.float64), info=((2,), np.int64))
    if want_node_h:
        outs["node_h"] = ((E, P), np.float64)

    def run(ctx, h, p, dst):
        out, info = dst("out"), dst("info")
        node_h = dst("node_h") if want_node_h else None
        _ok(ctx, ctx.lib.mm_gll_resolution(h, 2, 3, p("gp"), E, p("fast"), 2, p("slow"), 2, node_h.ptr if node_h else None,
                                           out.ptr, info.ptr))
        return (out, info, node_h) if want_node_h else (out, info)

    def expect(ref):
        out, info, h = RS.resolution(gp, 2, fast, slow)
        assert info.tolist() == [1, 1]
        return [out, info, h] if want_node_h else [out, info]

    return _abi_case(dict(gp=gp, fast=fast, slow=slow), outs, run, expect)


def _case_arg_extreme(want_max):
    rng = np.random.default_rng(17)
    v = rng.normal(size=(3, N_FREE))
    v[0, ::3], v[1, :] = np.nan, np.nan                     # a row without a valid value gives NaN and -1
    v[2, [5, 4000, N_FREE - 1]] = 9.0 if want_max else -9.0  # ties: the lowest index wins

    def run(ctx, h, p, dst):
        value, index, nvalid = dst("value"), dst("index"), dst("nvalid")
        _ok(ctx, ctx.lib.mm_arg_extreme(h, p("v"), 3, N_FREE, want_max, value.ptr, index.ptr, nvalid.ptr))
        return value, index, nvalid

    def expect(ref):
        want = RS.arg_extreme(v, bool(want_max))
        assert want[1].tolist()[1:] == [-1, 5]
        return list(want)

    return _abi_case(dict(v=v), dict(value=((3,), np.float64), index=((3,), np.int64), nvalid=((3,), np.int64)), run, expect)


# the four mm_pcg_* kernels, with the statements of tests/test_diffusion_gpu.py::test_vector_updates_bit_for_bit
def _pcg_vectors():
    rng = np.random.default_rng(7)
    n = N_FREE
    return n, rng.uniform(0.5, 1.5, size=n), [T.wide(rng, (3, n)) for _ in range(5)]


def _case_pcg_combine(with_mass, with_kp):
    n, mass, (p_, kp, _, _, _) = _pcg_vectors()
    tau = 0.125 if with_mass else -0.125
    inputs = dict(mass=mass, p=p_) if with_mass else {}
    if with_kp:
        inputs["kp"] = kp

    def run(ctx, h, p, dst):
        out = dst("out")
        _ok(ctx, ctx.lib.mm_pcg_combine(h, p("mass") if with_mass else None, p("p") if with_mass else None, tau,
                                        p("kp") if with_kp else None, n, 3, out.ptr))
        return out

    def expect(ref):
        if with_mass and with_kp:
            return [mass[None] * p_ + tau * kp]
        return [mass[None] * p_] if with_mass else [tau * kp]

    return _abi_case(inputs, dict(out=((3, n), np.float64)), run, expect)


def _pcg_state(**slots):
    state = np.random.default_rng(3).uniform(1.0, 2.0, size=(3, H.MM_PCG_STATE))
    for name, values in slots.items():
        state[:, getattr(H, "MM_PCG_" + name)] = values
    return state


def _slots(**slots):
    """compare: the slots of state_d the statement names hold exactly these values"""
    def compare(got, want):
        return all(list(np.asarray(got)[:, getattr(H, "MM_PCG_" + name)]) == list(values) for name, values in slots.items())

    return compare


def _case_pcg_scalars(phase, state, nactive, slots):
    outs = dict(nactive=((1,), np.int64)) if nactive is not None else {}

    def run(ctx, h, p, dst):
        nact = dst("nactive") if nactive is not None else None
        _ok(ctx, ctx.lib.mm_pcg_scalars(h, p("state"), 3, phase, 1e-3, nact.ptr if nact else None))
        return ("state", nact) if nact else ("state",)

    def expect(ref):
        return [state, np.array([nactive])] if nactive is not None else [state]

    return _abi_case(dict(state=state), outs, run, expect, inout=("state",), compare=[_slots(**slots), _equal])


def _case_pcg_direction():
    n, _, (p_, _, z, _, _) = _pcg_vectors()
    state = _pcg_state(ACTIVE=[0.0, 0.0, 1.0], BETA=[0.0, 0.0, 0.25])

    def run(ctx, h, p, dst):
        _ok(ctx, ctx.lib.mm_pcg_direction(h, p("state"), p("z"), n, 3, p("p")))
        return "p"

    def expect(ref):
        want = p_.copy()
        want[2] = z[2] + 0.25 * p_[2]                       # an inactive system is not touched
        return [want]

    return _abi_case(dict(state=state, z=z, p=p_), {}, run, expect, inout=("p",))


def _case_pcg_advance():
    n, _, (p_, ap, _, x, r) = _pcg_vectors()
    alpha = np.array([0.0, 4.1e-6 / 3.0, 2.0 / 7.0])
    state = _pcg_state(ACTIVE=[0.0, 1.0, 1.0], ALPHA=alpha)

    def run(ctx, h, p, dst):
        _ok(ctx, ctx.lib.mm_pcg_advance(h, p("state"), p("p"), p("ap"), n, 3, p("x"), p("r")))
        return "x", "r"

    def expect(ref):
        x_ref, r_ref = x + alpha[:, None] * p_, r - alpha[:, None] * ap
        x_ref[0], r_ref[0] = x[0], r[0]
        return [x_ref, r_ref]

    return _abi_case(dict(state=state, p=p_, ap=ap, x=x, r=r), {}, run, expect, inout=("x", "r"))


OWN_CASES = {
    "boundary_faces": _case_boundary_faces,
    "boundary_classify": _case_boundary_classify,
    "boundary_nodes": _case_boundary_nodes,
    "cutoff_distance": _case_cutoff_distance,
    "distance_taper": _case_distance_taper,
    "gll_resolution_node_h": lambda: _case_gll_resolution(True),
    "gll_resolution": lambda: _case_gll_resolution(False),
    "arg_extreme_min": lambda: _case_arg_extreme(0),
    "arg_extreme_max": lambda: _case_arg_extreme(1),
    "pcg_combine": lambda: _case_pcg_combine(True, True),
    "pcg_combine_mass_alone": lambda: _case_pcg_combine(True, False),
    "pcg_combine_kp_alone": lambda: _case_pcg_combine(False, True),
    # START: every system active, RZ_OLD = ALPHA = BETA = 0
    "pcg_scalars_start": lambda: _case_pcg_scalars(H.MM_PCG_PHASE_START, _pcg_state(), 3,
                                                   dict(ACTIVE=[1.0] * 3, RZ_OLD=[0.0] * 3, ALPHA=[0.0] * 3, BETA=[0.0] * 3)),
    # BETA: sqrt(RZ) <= rtol * sqrt(BB): 1e-3 <= 1e-3 * 2 converges; 2.02e-3 just above; far above
    "pcg_scalars_beta": lambda: _case_pcg_scalars(
        H.MM_PCG_PHASE_BETA, _pcg_state(ACTIVE=[1.0] * 3, RZ_OLD=[0.0] * 3, BB=[4.0, 4.0, 9.0], RZ=[1.0e-6, 4.1e-6, 2.0]), 2,
        dict(ACTIVE=[0.0, 1.0, 1.0], BETA=[0.0] * 3, RZ=[1.0e-6, 4.1e-6, 2.0])),
    "pcg_scalars_beta_later": lambda: _case_pcg_scalars(
        H.MM_PCG_PHASE_BETA, _pcg_state(ACTIVE=[0.0, 1.0, 1.0], RZ_OLD=[5.0, 4.1e-6, 2.0], BB=[4.0, 4.0, 9.0], RZ=[5.0, 1.0e-6, 0.5]),
        1, dict(ACTIVE=[0.0, 0.0, 1.0], BETA=[0.0, 0.0, 0.5 / 2.0])),
    "pcg_scalars_alpha": lambda: _case_pcg_scalars(
        H.MM_PCG_PHASE_ALPHA, _pcg_state(ACTIVE=[0.0, 1.0, 1.0], RZ_OLD=[1.0e-6, 4.1e-6, 2.0], PAP=[1.0, 3.0, 7.0]), None,
        dict(ALPHA=[0.0, 4.1e-6 / 3.0, 2.0 / 7.0])),
    "pcg_direction": _case_pcg_direction,
    "pcg_advance": _case_pcg_advance,
}
ALL_CASES = dict(CASES, **OWN_CASES)


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_stream_table_on_views(torch, ctx, name):
    case = ALL_CASES[name]()
    _run_reference(ctx, case)                               # (the first call grows the scratch pool)
    ref, _ = _run_reference(ctx, case)
    compare = case.compare or _bits
    want = case.expect(ref)
    _same_as(ref, want, compare, (name, "NumPy inputs against the CPU"))
    for misaligned in (False, True):
        what = (name, "misaligned views" if misaligned else "aligned views")
        got = _run_on_views(torch, ctx, case, misaligned, what)
        _same_as(got, ref, _bits, what + ("against NumPy inputs",))
        _same_as(got, want, compare, what + ("against the CPU",))


# -------------------------------------------------------------------------------------------- mm_gather at the ABI
def test_gather_p8_in_every_alignment_of_ids_and_weights(torch, ctx):
    """P = 8: ``ids`` and ``w`` both on 16 bytes take gather8_kernel, any other combination gatherP_kernel with P = 8
    (no tail, one full octet) -- the same bits: NumPy's pairwise order of an 8-term row, from the identity 0.0."""
    rng = np.random.default_rng(808)
    n, nsrc = N_FREE, 1000
    field = rng.normal(size=(3, nsrc))
    field[:, 0] = -np.abs(field[:, 0])                      # failed points read node 0: -x * 0.0 = -0.0, and 0.0 + -0.0 = 0.0
    ids = rng.integers(0, nsrc, (n, 8))
    w = rng.uniform(-1.0, 1.0, (n, 8))
    failed = np.arange(n) % 97 == 0
    ids[failed], w[failed] = 0, 0.0
    for ncomp in (1, 3):
        want = np.stack([np.sum(field[c][ids] * w, axis=1) for c in range(ncomp)])
        assert not np.signbit(want[:, failed]).any()
        for point_major in (0, 1):
            expect = np.ascontiguousarray(want.T) if point_major else want
            for ids_off, w_off in ((True, False), (False, True), (True, True), (False, False)):
                what = ("mm_gather", ncomp, point_major, "ids off" if ids_off else "ids on", "w off" if w_off else "w on")
                bi, bw, bo = Buffers(torch, ids_off), Buffers(torch, w_off), Buffers(torch, True)
                f_t = bo.view((ncomp, nsrc), np.float64, field[:ncomp])
                ids_t, w_t = bi.view(ids.shape, np.int64, ids), bw.view(w.shape, np.float64, w)
                out_t = bo.view(expect.shape, np.float64)
                rc = ctx.lib.mm_gather(ctx.handle, f_t.data_ptr(), nsrc, ncomp, ids_t.data_ptr(), w_t.data_ptr(), n, 8,
                                       out_t.data_ptr(), point_major)
                assert rc == 0, (what, ctx.lib.mm_last_error())
                ctx.synchronize()
                for b in (bi, bw, bo):
                    b.check_borders(what)
                assert _bits(_numpy(out_t), expect), what


# --------------------------------------------------------------------------------------- mm_locate_hex8 at the ABI
@pytest.fixture(scope="module")
def located():
    """k -> the oracle's rows with the sentinel in the rows of failed targets, and the failed count"""
    d = _hex8()
    rows = {}
    for k in (1, 8, 20):
        nn = np.ascontiguousarray(d.nn[:, :k])
        enc, w, nf = O.locate_hex8(nn, d.conn_r, d.pa, d.pb)
        failed = ~w.any(axis=1)                             # (the oracle leaves the rows of failed targets as they were: zero)
        assert failed.sum() == nf
        enc, w = enc.copy(), w.copy()
        enc[failed], w[failed] = SENTINEL, float(SENTINEL)
        rows[k] = (nn, enc, w, nf, failed)
    assert rows[1][3] > 0 and rows[20][3] < rows[1][3]
    return rows


@pytest.mark.parametrize("mode", ["exact", "tol"])
@pytest.mark.parametrize("exodus", [0, 1])
@pytest.mark.parametrize("k", [1, 8, 20])
def test_locate_hex8_on_views(torch, ctx, located, k, exodus, mode):
    d = _hex8()
    nn, enc_o, w_o, nf_o, failed = located[k]
    conn = d.ca if exodus else d.conn_r                     # (conn_is_exodus applies synth.reorder_hex8 on the fly)
    got = {}
    ctx.set_fp_mode(mode)
    try:
        for misaligned in (False, True):
            what = ("mm_locate_hex8", k, exodus, mode, misaligned)
            bufs = Buffers(torch, misaligned)
            nn_t, conn_t = bufs.view(nn.shape, np.int64, nn), bufs.view(conn.shape, np.int64, conn)
            nodes_t, pts_t = bufs.view(d.pa.shape, np.float64, d.pa), bufs.view(d.pb.shape, np.float64, d.pb)
            enc_t, w_t = bufs.view(enc_o.shape, np.int64), bufs.view(w_o.shape, np.float64)
            nf = ctx.lib.mm_locate_hex8(ctx.handle, k, len(d.pb), nn_t.data_ptr(), conn_t.data_ptr(), len(conn), exodus,
                                        enc_t.data_ptr(), nodes_t.data_ptr(), w_t.data_ptr(), pts_t.data_ptr())
            assert nf == nf_o, (what, nf, nf_o, ctx.lib.mm_last_error())
            bufs.check_borders(what)
            assert np.array_equal(_numpy(conn_t), conn) and np.array_equal(_numpy(nn_t), nn), what
            got[misaligned] = (_numpy(enc_t), _numpy(w_t))
    finally:
        ctx.set_fp_mode("exact")
    for misaligned, (enc, w) in got.items():
        assert np.array_equal(enc, enc_o), (k, exodus, mode, misaligned)        # failed rows keep the -7
        assert (w[failed] == SENTINEL).all()
        if mode == "exact":
            assert _bits(w, w_o), (k, exodus, mode, misaligned)
        else:                                               # MM_FP_TOL as include/multimesh_hip.h states it
            assert np.abs(w - w_o).max() <= 1e-12, (k, exodus, mode, misaligned)
    assert _bits(got[True][1], got[False][1]) and _bits(got[True][0], got[False][0])


def test_locate_hex8_refuses_misaligned_connectivity_of_unknown_size(torch, ctx):
    """nelem = 0 (no bounds guard): the library cannot copy an array whose size it does not know"""
    d = _hex8()
    nn = np.ascontiguousarray(d.nn[:64, :8])
    for misaligned in (True, False):
        bufs = Buffers(torch, misaligned)
        conn_t, nn_t = bufs.view(d.conn_r.shape, np.int64, d.conn_r), bufs.view(nn.shape, np.int64, nn)
        nodes_t, pts_t = bufs.view(d.pa.shape, np.float64, d.pa), bufs.view((64, 3), np.float64, d.pb[:64])
        enc_t, w_t = bufs.view((64, 8), np.int64), bufs.view((64, 8), np.float64)
        rc = ctx.lib.mm_locate_hex8(ctx.handle, 8, 64, nn_t.data_ptr(), conn_t.data_ptr(), 0, 0, enc_t.data_ptr(),
                                    nodes_t.data_ptr(), w_t.data_ptr(), pts_t.data_ptr())
        bufs.check_borders(("nelem = 0", misaligned))
        if misaligned:
            assert rc == -1 and b"mm_locate_hex8: connectivity_d off 16-byte alignment needs nelem" in ctx.lib.mm_last_error()
            assert (_numpy(enc_t) == SENTINEL).all() and (_numpy(w_t) == SENTINEL).all()       # nothing is written
        else:                                               # ... and the next call is served
            enc, w, nf = O.locate_hex8(nn, d.conn_r, d.pa, d.pb[:64])
            ok = w.any(axis=1)
            assert rc == nf and np.array_equal(_numpy(enc_t)[ok], enc[ok]) and _bits(_numpy(w_t)[ok], w[ok])


# ----------------------------------------------------------------------------------------- mm_knn_query at the ABI
def _clouds(dim):
    rng = np.random.default_rng(31003 + dim)
    uniform = rng.uniform(size=(128 * 100, dim)), rng.uniform(-0.1, 1.1, size=(N_FREE, dim))
    centres = rng.uniform(size=(7, dim))                    # the clustered cloud of tests/test_guarded_gpu.py
    src = centres[rng.integers(0, len(centres), size=128 * 40)] + rng.normal(scale=0.03, size=(128 * 40, dim))
    lo, hi = src.min(axis=0), src.max(axis=0)
    return {"uniform": uniform, "clustered": (src, rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(N_FREE, dim)))}


def _query_on_views(torch, ctx, index, tgt, k, want_dist, misaligned, what):
    """-> (idx, dist or None, the kernels that ran) of one mm_knn_query on views, borders checked"""
    bufs = Buffers(torch, misaligned)
    pts_t = bufs.view(tgt.shape, np.float64, tgt)
    idx_t = bufs.view((len(tgt), k), np.int64)
    dist_t = bufs.view((len(tgt), k), np.float64) if want_dist else None
    rc = ctx.lib.mm_knn_query(ctx.handle, index.handle, pts_t.data_ptr(), len(tgt), k, idx_t.data_ptr(),
                              dist_t.data_ptr() if want_dist else None)
    assert rc == 0, (what, ctx.lib.mm_last_error())
    ctx.synchronize()
    ran = ctx.last_knn_kernels()
    bufs.check_borders(what)
    return _numpy(idx_t), _numpy(dist_t) if want_dist else None, ran


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("k", [3, 4, 8, 20, 33, 64])
def test_knn_query_on_views(torch, ctx, k, dim):
    for cloud, (src, tgt) in _clouds(dim).items():
        idx_o, dist_o = O.knn_ckdtree(src, tgt, k)
        idx_o, dist_o = idx_o.reshape(len(tgt), k), dist_o.reshape(len(tgt), k)
        index = ctx.knn_build(src)
        for want_dist in (False, True):
            for misaligned in (False, True):
                what = ("mm_knn_query", cloud, dim, k, want_dist, misaligned)
                idx, dist, _ = _query_on_views(torch, ctx, index, tgt, k, want_dist, misaligned, what)
                assert np.array_equal(idx, idx_o), what
                assert not want_dist or _close12(dist, dist_o), what
        index.free()


def test_strip_cell_lane_and_list_kernels_write_misaligned_rows_of_an_even_k(torch, ctx):
    """The row writers that store two entries at a time -- the strip, cell and lane kernels and the list kernel their
    hand-overs go to -- all run on misaligned views with an even k (its own queries: no other test is needed for it)."""
    ran = {}
    for dim in (3, 2):                                      # (a grid that is flat in z keeps the cell kernel, a deep one the strips)
        for cloud, (src, tgt) in _clouds(dim).items():
            index = ctx.knn_build(src)
            for k in (4, 8, 20):
                what = ("mm_knn_query", cloud, dim, k, "misaligned")
                idx, dist, kernels = _query_on_views(torch, ctx, index, tgt, k, True, True, what)
                idx_o, dist_o = O.knn_ckdtree(src, tgt, k)
                assert np.array_equal(idx, idx_o.reshape(idx.shape)) and _close12(dist, dist_o.reshape(dist.shape)), what
                ran[cloud, dim, k] = sorted(kernels)
            index.free()
    print(ran)
    assert {"strip", "cell", "lane", "list"} <= set().union(*ran.values()), ran


# ------------------------------------------------------------------------- the fused entries' operator rows and source
@pytest.mark.parametrize("resident", [False, True])
def test_interpolate_hex8_operator_rows_and_borrowed_mesh_on_views(torch, ctx, resident):
    """mm_interpolate_hex8 with enc_d / w_d views, and mm_interpolate_hex8_on on a source whose borrowed nodes_d /
    connectivity_d are views"""
    d = _hex8()
    n, ncomp = len(d.pb), len(d.fields)
    got = {}
    for misaligned in (False, True):
        what = ("mm_interpolate_hex8_on" if resident else "mm_interpolate_hex8", misaligned)
        bufs = Buffers(torch, misaligned)
        nodes_t, conn_t = bufs.view(d.pa.shape, np.float64, d.pa), bufs.view(d.ca.shape, np.int64, d.ca)
        pts_t, f_t = bufs.view(d.pb.shape, np.float64, d.pb), bufs.view(d.fields.shape, np.float64, d.fields)
        out_t, enc_t, w_t = bufs.view((n, ncomp), np.float64), bufs.view((n, 8), np.int64), bufs.view((n, 8), np.float64)
        if resident:
            h = C.c_void_p()
            rc = ctx.lib.mm_source_create(ctx.handle, nodes_t.data_ptr(), len(d.pa), conn_t.data_ptr(), len(d.ca), C.byref(h))
            assert rc == 0, (what, ctx.lib.mm_last_error())
            try:
                for _ in range(2):                          # (the second call replays the first one's target sort)
                    nf = ctx.lib.mm_interpolate_hex8_on(ctx.handle, h, pts_t.data_ptr(), n, f_t.data_ptr(), ncomp, 20,
                                                        out_t.data_ptr(), enc_t.data_ptr(), w_t.data_ptr())
                    assert nf == d.nf, (what, nf, ctx.lib.mm_last_error())
            finally:
                ctx.lib.mm_source_destroy(ctx.handle, h)
        else:
            nf = ctx.lib.mm_interpolate_hex8(ctx.handle, nodes_t.data_ptr(), len(d.pa), conn_t.data_ptr(), len(d.ca),
                                             pts_t.data_ptr(), n, f_t.data_ptr(), ncomp, 20, out_t.data_ptr(),
                                             enc_t.data_ptr(), w_t.data_ptr())
            assert nf == d.nf, (what, nf, ctx.lib.mm_last_error())
        bufs.check_borders(what)
        assert np.array_equal(_numpy(conn_t), d.ca) and _bits(_numpy(nodes_t), d.pa), what
        got[misaligned] = (_numpy(out_t), _numpy(enc_t), _numpy(w_t))
        assert np.array_equal(got[misaligned][0], d.vals) and np.array_equal(got[misaligned][1], d.enc), what
        assert np.array_equal(got[misaligned][2], d.w), what
    for x, y in zip(got[True], got[False]):
        assert _bits(x, y)
