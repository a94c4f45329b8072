"""The device API on a caller's stream and on the caller's own tensors.

Every other GPU test runs its context on the null stream and hands it NumPy arrays.  Here one context runs on a
non-blocking stream of torch's pool, ``side``, and every call takes torch tensors in place.  The pattern is "late
producer, early consumer": under ``side`` the inputs are allocated holding harmless wrong values (zeros), the outputs
holding a sentinel (-7), the stream spins, the true inputs are copied in *on that stream*, the library is called, and the
outputs are cloned and overwritten right after it -- with no host synchronisation of the test's in between.  A launch,
memset or copy of the library that is not ordered on the context's stream reads the zeros, or is read before it wrote,
and the values are wrong; nothing faults.  The values are held to what the family's own GPU test holds them to (its CPU
oracle or NumPy statement, compared as it compares) and, bit for bit, to the same call on a null-stream context with
NumPy inputs.

The spin must outlast the window in which a misplaced launch would run, at most the call itself: it is sized from a
measurement, at least 2.5 times the slowest call of the table on the null-stream context (and 5 ms), re-measured with
torch events on ``side`` and asserted to be at least twice that call and under 100 ms.  Measured on an MI355X: a spin of
65 061 413 cycles = 27.2 ms; the slowest call, two diffusion steps of ``smooth`` (PCG with a read-back per iteration),
10.9 ms."""
import math
import threading
import time
import types

import numpy as np
import pytest

import diffusion_cases as DC
import gradient_cases as GC
import grid_import_cases as G
import mass_cases as M
import order_cases as OC
import precondition_cases as PC
import radial_cases as RC
import transpose_cases as T
from multimesh_amd import api, helpers, synth
from multimesh_amd.device import POINT_TAPER_BATCH, Context, DeviceArray
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = -7
SPIN_FACTOR, SPIN_FLOOR_MS, SPIN_LIMIT_MS = 2.5, 5.0, 100.0


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def side(torch):
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    return s


@pytest.fixture(scope="module")
def ctx_side(side):
    with Context(0, stream=side.cuda_stream) as c:
        yield c


@pytest.fixture(scope="module")
def ctx_ref():
    with Context(0) as c:
        yield c


# ------------------------------------------------------------------------------------------------------------- helpers
def _bits(a, b):
    """Equal shapes and, for floats, equal bits (NaN in the same places: its payload is not part of a statement)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float64 and b.dtype == np.float64:
        return RC.same_bits_nan(a, b)
    return bool(np.array_equal(a, b))


def _equal(a, b):
    """``==`` on every entry, what the hex8 / GLL parity tests assert against the oracle."""
    return np.shape(a) == np.shape(b) and bool(np.array_equal(a, b))


def _close12(a, b):
    """kNN distances against the k-d tree's, as tests/test_parity_gpu.py holds them"""
    return np.shape(a) == np.shape(b) and bool(np.allclose(a, b, rtol=1e-12, atol=0))


class Case:
    """One call: ``inputs`` name -> NumPy array (uploaded late), ``outs`` name -> (shape, dtype) of the caller's output
    tensors, ``inout`` the inputs the call updates in place, ``call(ctx, a, o)`` -> tuple of results (device arrays,
    NumPy arrays, numbers, or the name of an ``inout`` array), ``expect(ref)`` -> the CPU's values of the same tuple
    (None: not stated by the oracle) given the null-stream results, ``compare`` per result (default: bits)."""

    def __init__(self, inputs, call, expect, outs=None, inout=(), compare=None):
        self.inputs = {k: np.ascontiguousarray(v) for k, v in inputs.items()}
        self.call, self.expect, self.outs, self.inout, self.compare = call, expect, outs or {}, tuple(inout), compare


def _flatten(results):
    return list(results) if isinstance(results, tuple) else [results]


def _run_reference(ctx, case):
    """The call on the null-stream context with NumPy inputs -> (results as NumPy / numbers, seconds of the call)."""
    a = types.SimpleNamespace(**{k: (ctx.to_device(v) if k in case.inout else v) for k, v in case.inputs.items()})
    o = types.SimpleNamespace(**{k: None for k in case.outs})
    ctx.synchronize()
    t0 = time.perf_counter()
    results = _flatten(case.call(ctx, a, o))
    ctx.synchronize()
    seconds = time.perf_counter() - t0
    out = []
    for r in results:
        if isinstance(r, str):
            r = getattr(a, r)
        out.append(r.numpy() if isinstance(r, DeviceArray) else r)
    return out, seconds


def _run_on_side(torch, side, ctx, case, cycles):
    """The late producer, early consumer pattern -> results as NumPy / numbers."""
    staging = {k: torch.from_numpy(v).cuda() for k, v in case.inputs.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        a = {k: torch.zeros_like(t) for k, t in staging.items()}
        o = {k: torch.full(tuple(shape), SENTINEL, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
             for k, (shape, dt) in case.outs.items()}
        torch.cuda._sleep(cycles)
        for k, t in a.items():
            t.copy_(staging[k], non_blocking=True)
        args = types.SimpleNamespace(**a)                   # (kept to the end: a handle a call leaves on it is freed late)
        results = _flatten(case.call(ctx, args, types.SimpleNamespace(**o)))
        watched = dict(o, **{k: a[k] for k in case.inout})
        clones = {k: t.clone() for k, t in watched.items()}
        for t in watched.values():
            t.fill_(SENTINEL)
        taken = set()
        got = []
        for r in results:
            if isinstance(r, str):
                taken.add(r)
                got.append(("tensor", r, a[r].shape))
            elif isinstance(r, DeviceArray):
                names = [k for k, t in watched.items() if t.data_ptr() == r.ptr]
                if names:
                    taken.add(names[0])
                    got.append(("tensor", names[0], r.shape))
                else:
                    got.append(("value", r.numpy()))
            else:
                got.append(("value", r))
    side.synchronize()
    del args
    assert taken == set(watched), f"the call did not return the caller's arrays {sorted(set(watched) - taken)} themselves"
    out = []
    for item in got:
        if item[0] == "tensor":
            flat = clones[item[1]].cpu().numpy().reshape(-1)
            size = int(np.prod(item[2], dtype=np.int64))
            out.append(np.ascontiguousarray(flat[:size]).reshape(tuple(item[2])))
        else:
            out.append(item[1])
    return out


def _same_as(got, want, compare, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            continue
        if isinstance(w, (int, np.integer)):
            assert int(g) == int(w), (what, i, g, w)
        else:
            ok = compare[i](g, w) if isinstance(compare, (list, tuple)) else compare(g, w)
            assert ok, (what, i, np.shape(g), np.shape(w), int((np.asarray(g) != np.asarray(w)).sum())
                        if np.shape(g) == np.shape(w) else "shapes differ")


# ------------------------------------------------------------------------------------------------------- the case table
def _lazy(fn):
    cache = {}

    def get():
        if "v" not in cache:
            cache["v"] = fn()
        return cache["v"]

    return get


@_lazy
def _hex8():
    d = types.SimpleNamespace()
    d.pa, d.ca = synth.hex_mesh(20, seed=1)
    d.pb, _ = synth.hex_mesh(22, seed=7)                                    # 10 648 targets
    d.fields = np.ascontiguousarray(synth.vector_field(d.pa)[:2])
    d.cen = O.centroid(d.ca, d.pa)
    d.nn, _ = O.knn_ckdtree(d.cen, d.pb, 20)
    d.conn_r = synth.reorder_hex8(d.ca)
    d.enc, d.w, d.nf = O.locate_hex8(d.nn, d.conn_r, d.pa, d.pb)
    d.vals = O.gather(d.fields, d.enc, d.w)
    return d


def _case_centroid():
    d = _hex8()
    return Case(dict(conn=d.ca, pts=d.pa), lambda ctx, a, o: ctx.centroid(a.conn, a.pts), lambda ref: [d.cen], compare=_equal)


def _case_knn(k):
    d = _hex8()

    def call(ctx, a, o):
        a.keep = ctx.knn_build(a.src)                     # (released with ``a``: freeing it synchronises the stream)
        return a.keep.query(a.q, k, want_dist=True)

    def expect(ref):
        idx, dist = O.knn_ckdtree(d.cen, d.pb, k)
        return [idx, dist]

    return Case(dict(src=d.cen, q=d.pb), call, expect, compare=[_equal, _close12])


def _case_locate_hex8():
    d = _hex8()

    def call(ctx, a, o):
        enc, w, nf = ctx.locate_hex8(a.nn, a.conn, a.nodes, a.pts)
        return enc, w, nf, ctx.gather(a.fields, enc, w)

    return Case(dict(nn=d.nn, conn=d.conn_r, nodes=d.pa, pts=d.pb, fields=d.fields), call,
                lambda ref: [d.enc, d.w, d.nf, d.vals], compare=_equal)


def _case_interpolate_hex8(want_operator):
    d = _hex8()

    def call(ctx, a, o):
        return ctx.interpolate_hex8(a.nodes, a.conn, a.pts, a.fields, nelem_to_search=20, want_operator=want_operator, out=o.out)

    return Case(dict(nodes=d.pa, conn=d.ca, pts=d.pb, fields=d.fields), call,
                lambda ref: [d.vals, d.enc, d.w, d.nf] if want_operator else [d.vals, d.nf],
                outs=dict(out=((len(d.pb), 2), np.float64)), compare=_equal)


def _case_source_twice():
    d = _hex8()

    def call(ctx, a, o):
        a.keep = ctx.source(a.nodes, a.conn)
        v1, nf1 = a.keep.interpolate(a.pts, a.fields, out=o.out1)
        v2, nf2 = a.keep.interpolate(a.pts, a.fields, out=o.out2)
        return v1, nf1, v2, nf2

    shape = ((len(d.pb), 2), np.float64)
    return Case(dict(nodes=d.pa, conn=d.ca, pts=d.pb, fields=d.fields), call, lambda ref: [d.vals, d.nf, d.vals, d.nf],
                outs=dict(out1=shape, out2=shape), compare=_equal)


def _gll(dim):
    order = 2 if dim == 3 else 4
    gp = synth.gll_mesh(6, order, seed=4, jitter=0.25, dim=dim)
    rng = np.random.default_rng(order + dim)
    fields = np.stack([synth.field_linear(gp), synth.field_smooth(gp.reshape(-1, dim)).reshape(gp.shape[:2])])
    return order, gp, rng, np.ascontiguousarray(fields), min(20, gp.shape[0])


def _case_locate_gll(dim):
    order, gp, rng, fields, k = _gll(dim)
    pts = rng.uniform(-0.03, 1.03, size=(3000, dim))
    nn = O.knn_ckdtree(gp.mean(axis=1), pts, k)[0]

    def call(ctx, a, o):
        elem, co, miss = ctx.locate_gll(order, a.nn, a.gp, a.pts, tolerance=1.05)
        return elem, co, miss, ctx.gather_elem(a.fields, elem, co)

    def expect(ref):
        elem, co, miss = O.locate_gll(order, nn, gp, pts, tolerance=1.05)
        return [elem, co, miss, O.gather_elem(fields, elem, co)]

    return Case(dict(nn=nn, gp=gp, pts=pts, fields=fields), call, expect, compare=_equal)


def _case_locate_gll_bbox(dim):
    order, gp, rng, fields, k = _gll(dim)
    pts = rng.uniform(0.02, 0.98, size=(3000, dim))
    nn = O.knn_ckdtree(gp.mean(axis=1), pts, k)[0]
    return Case(dict(nn=nn, gp=gp, pts=pts), lambda ctx, a, o: ctx.locate_gll_bbox(order, a.nn, a.gp, a.pts),
                lambda ref: list(O.locate_gll_v1(order, nn, gp, pts)), compare=_equal)


def _case_interpolate_gll(dim):
    order, gp, rng, fields, k = _gll(dim)
    pts = rng.uniform(-0.03, 1.03, size=(3000, dim))

    def call(ctx, a, o):
        return ctx.interpolate_gll(order, a.gp, a.pts, a.fields, nelem_to_search=k, tolerance=1.05, want_operator=True, out=o.out)

    def expect(ref):
        nn = O.knn_ckdtree(gp.mean(axis=1), pts, k)[0]
        elem, co, miss = O.locate_gll(order, nn, gp, pts, tolerance=1.05)
        return [O.gather_elem(fields, elem, co), elem, co, miss]

    return Case(dict(gp=gp, pts=pts, fields=fields), call, expect, outs=dict(out=((3000, 2), np.float64)), compare=_equal)


def _case_sample_columns():
    from test_regular_grid_gpu import K, _chunk

    order = 2
    c, f = _chunk(order, True)
    gp = c["points"]
    lat, lon, depth = np.linspace(-8.77, 9.13, 17), np.linspace(-9.31, 8.29, 15), np.linspace(3217.0, 410_111.0, 5)
    lat_t, lon_t, r = api.column_tables(lat, lon, depth)

    def call(ctx, a, o):
        return ctx.sample_columns_gll(order, a.gp, a.f, a.lat_t, a.lon_t, a.r, nelem_to_search=K, want_points=True, out=o.out)

    def expect(ref):                        # tests/test_regular_grid_gpu.py::test_values_equal_the_oracle
        pts = ref[2].reshape(-1, 3)
        cen = gp[:, 0].copy()
        for p in range(1, gp.shape[1]):
            cen = cen + gp[:, p]
        cen = cen / gp.shape[1]
        nn, _ = O.knn_ckdtree(cen, pts, K)
        elem, co, miss = O.locate_gll(order, nn, gp, pts, tolerance=1.05)
        want = O.gather_elem(f, elem, co).T.copy()
        want[:, elem < 0] = np.nan
        assert 0 < miss < len(elem)
        return [want.reshape(3, len(depth), -1), miss, None]

    return Case(dict(gp=gp, f=f, lat_t=lat_t, lon_t=lon_t, r=r), call, expect,
                outs=dict(out=((3, len(depth), len(lat) * len(lon)), np.float64)))


def _case_sample_grid():
    pts, grid, fill = G.chunk_points(4099), G.grid_values(3), -12345.5

    def call(ctx, a, o):
        return ctx.sample_grid(a.pts, a.grid, a.depth, a.lat, a.lon, fill_value=fill, out=o.out, want_latlondepth=True)

    def expect(ref):                        # the statement on the device's own coordinates, as tests/test_grid_import_gpu.py
        lld = ref[2]
        want, nmiss, inside = G.sample(grid, G.DEPTH, G.LAT, G.LON, lld[:, 2], lld[:, 0], lld[:, 1], "fill", fill, False, None)
        assert 0.2 * len(pts) < nmiss < 0.8 * len(pts)
        return [want, nmiss, None]

    return Case(dict(pts=pts, grid=grid, depth=G.DEPTH, lat=G.LAT, lon=G.LON), call, expect,
                outs=dict(out=((3, len(pts)), np.float64)))


def _case_transpose_nodes():
    rng = np.random.default_rng(21)
    n, p, nsrc = 5003, 8, 1000
    ids, w, v = rng.integers(0, nsrc, (n, p)), rng.uniform(0.0, 1.0, (n, p)), T.wide(rng, (n, 3))

    def call(ctx, a, o):
        a.keep = ctx.transpose_nodes(a.ids, a.w, nsrc)
        return a.keep.apply(a.v, out=o.out)

    return Case(dict(ids=ids, w=w, v=v), call, lambda ref: [T.transpose_nodes(ids, w, v, nsrc)],
                outs=dict(out=((3, nsrc), np.float64)))


def _case_transpose_elem():
    rng = np.random.default_rng(22)
    n, p, nelem = 5003, 27, 125
    elem, co, v = rng.integers(-1, nelem, n), rng.uniform(-0.2, 1.0, (n, p)), T.wide(rng, (n, 3))

    def call(ctx, a, o):
        a.keep = ctx.transpose_elem(a.elem, a.co, nelem)
        return a.keep.apply(a.v, out=o.out)

    return Case(dict(elem=elem, co=co, v=v), call, lambda ref: [T.transpose_elem(elem, co, v, nelem)],
                outs=dict(out=((3, nelem, p), np.float64)))


def _tables(order):
    _, w, D = api.gll_quadrature(order)
    return w, D


def _case_gll_mass():
    gp = synth.gll_mesh(9, 2, seed=3)

    def expect(ref):
        mass, det = M.mass(gp, 2, *_tables(2))
        return [mass, M.n_bad(det), det]

    return Case(dict(gp=gp), lambda ctx, a, o: ctx.gll_mass(2, a.gp, want_det=True), expect)


def _case_weighted_sum():
    rng = np.random.default_rng(97)
    mass, f = rng.uniform(0.5, 1.5, size=4097), T.wide(rng, (3, 4097))
    return Case(dict(mass=mass, f=f), lambda ctx, a, o: ctx.weighted_sum(a.mass, a.f), lambda ref: [M.weighted_sum(mass, f)])


def _case_divide_rows():
    rng = np.random.default_rng(98)
    num, den = T.wide(rng, (2, 125, 27)), rng.uniform(0.5, 1.5, size=(125, 27))
    return Case(dict(num=num, den=den), lambda ctx, a, o: ctx.divide_rows(a.num, a.den, out=o.out), lambda ref: [num / den],
                outs=dict(out=(num.shape, np.float64)))


def _case_diffusion_apply():
    gp = synth.gll_mesh(9, 2, seed=3)
    u = T.wide(np.random.default_rng(231), (2,) + gp.shape[:2])

    def call(ctx, a, o):
        a.keep = ctx.diffusion(2, a.gp, kappa_h=0.7)
        return a.keep.apply(a.u, out=o.out)

    return Case(dict(gp=gp, u=u), call, lambda ref: [DC.apply(gp, 2, *_tables(2), u, kh=0.7)], outs=dict(out=(u.shape, np.float64)))


def _case_smooth():
    from test_diffusion_gpu import _check_against_direct, _cube, _fields

    n, steps, rtol = 5, 2, 1e-10
    gp = _cube(n, 2)
    f = np.ascontiguousarray(_fields(gp, 2)[:2])
    sigma = 1.0 / (n - 1)

    def call(ctx, a, o):
        a.keep = ctx.diffusion(2, a.gp, kappa_h=sigma * sigma)
        return a.keep.smooth(a.f, steps=steps, rtol=rtol)

    def within_the_bound(got, want):       # the direct solve, within the bound tests/test_diffusion_gpu.py states
        _check_against_direct(got, gp, 2, f, steps, rtol, "smooth on a caller's stream", kh=sigma * sigma)
        return True

    return Case(dict(gp=gp, f=f), call, lambda ref: [f], compare=within_the_bound)


def _case_gradient():
    gp = synth.gll_mesh(6, 2, seed=5)
    u = T.wide(np.random.default_rng(232), (2,) + gp.shape[:2])

    def call(ctx, a, o):
        return ctx.gll_gradient(2, a.gp, a.u, grad=True, radial=True, lateral=True, norm=True)

    return Case(dict(gp=gp, u=u), call, lambda ref: list(GC.gradient(gp, 2, _tables(2)[1], u)))


def _case_tensor_apply():
    values = T.wide(np.random.default_rng(233), (2, 125, 27))

    def call(ctx, a, o):
        return ctx.gll_tensor_apply(2, 4, 3, a.values, out=o.out)

    return Case(dict(values=values), call, lambda ref: [OC.tensor_apply(OC.table(2, 4), 3, values)],
                outs=dict(out=((2, 125, 125), np.float64)))


def _case_element_deviation():
    a_ = synth.gll_mesh(6, 2, seed=5)
    b_ = a_ + np.random.default_rng(234).normal(size=a_.shape) * 1e-3
    return Case(dict(a=a_, b=b_), lambda ctx, a, o: ctx.element_deviation(a.a, a.b), lambda ref: list(OC.element_deviation(a_, b_)))


def _shell_points(n, seed):
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 3))
    return pts * (rng.uniform(2.8e6, 6.6e6, n) / np.linalg.norm(pts, axis=1))[:, None]


def _case_radial_bins():
    pts, edges = _shell_points(3 * 4096 + 5, 31), np.linspace(3.0e6, 6.4e6, 8)

    def call(ctx, a, o):
        return ctx.radial_bins(a.pts, a.edges, want_radius=True)

    return Case(dict(pts=pts, edges=edges), call, lambda ref: list(RC.bins(pts, edges)))


def _case_binned_sum():
    from test_radial_gpu import _shuffled

    n, nbins = 3 * 4096 + 5, 7
    mass, fields, bins = _shuffled(n, nbins, 2, 32)
    bins = np.where((bins < 0) | (bins >= nbins), -1, bins).astype(np.int32)

    def call(ctx, a, o):
        return ctx.binned_weighted_sum(a.mass, a.bins, nbins, a.fields, want_count=True)

    return Case(dict(mass=mass, fields=fields, bins=bins), call,
                lambda ref: [RC.binned_weighted_sum(mass, fields, bins, nbins, False), RC.bin_counts(bins, nbins)])


def _case_radial_model():
    from test_radial_gpu import RADII3, _table3

    pts = synth.earth_chunk(2, nlat=5, nlon=6, radii=RADII3, nrad=(1, 2, 1))["points"]
    R, V = _table3()
    vin = np.random.default_rng(11).uniform(3.0, 5.0, (2,) + pts.shape[:2])

    def call(ctx, a, o):
        return ctx.radial_model_apply(a.pts, a.R, a.V, mode=1, values_in=a.vin, out=o.out)

    return Case(dict(pts=pts, R=R, V=V, vin=vin), call, lambda ref: [RC.model_apply(pts, R, V, 1, vin).reshape(vin.shape)],
                outs=dict(out=(vin.shape, np.float64)))


def _case_point_taper():
    from test_precondition_gpu import _centres_in

    pts = np.ascontiguousarray(synth.gll_mesh(7, 2, seed=4)[:3 * (256 // 27) - 1])
    c, ri, ro = _centres_in(pts, POINT_TAPER_BATCH + 1, seed=20 + POINT_TAPER_BATCH + 1)
    vals = np.random.default_rng(7).normal(size=(2,) + pts.shape[:2])

    def call(ctx, a, o):
        return ctx.point_taper(a.pts, a.c, a.ri, a.ro, values_in=a.vals, out=o.out, want_weight=True)

    def expect(ref):
        out, w, count = PC.taper_apply(pts, c, ri, ro, vals.reshape(2, -1))
        return [out.reshape(vals.shape), count, w.reshape(pts.shape[:2])]

    return Case(dict(pts=pts, c=c, ri=ri, ro=ro, vals=vals), call, expect, outs=dict(out=(vals.shape, np.float64)))


def _case_order_statistics():
    v = np.random.default_rng(41).normal(size=(3, 4097)) * np.array([[1.0], [1e-3], [1e6]])
    q = np.array([0.0, 0.5, 0.999, 1.0])

    def call(ctx, a, o):
        return ctx.order_statistics(a.v, ctx.asdevice(a.q, np.float64), absolute=True, method="higher")

    return Case(dict(v=v, q=q), call, lambda ref: list(PC.order_statistics(v, q, absolute=True, method="higher")))


def _case_clamp():
    v = np.random.default_rng(42).normal(size=(3, 4097)) * np.array([[1.0], [1e-3], [1e6]])
    v[1, ::5] = -0.0
    upper = np.array([0.5, 1e-4, 2.0])

    def call(ctx, a, o):
        return ctx.clamp(a.v, upper=a.upper, symmetric=True, out=o.out)

    return Case(dict(v=v, upper=upper), call, lambda ref: list(PC.clamp(v, upper=upper, symmetric=True)),
                outs=dict(out=(v.shape, np.float64)))


def _case_unique(ordered):
    from test_api_gpu import _first_occurrence_form

    pts = synth.gll_mesh(9, 4, seed=3).reshape(-1, 3)
    pts = np.ascontiguousarray(pts[np.random.default_rng(0).permutation(len(pts))])

    def call(ctx, a, o):
        return ctx.unique_points(a.pts, unique_out=o.uniq, inverse_out=o.inv, ordered=ordered)

    def expect(ref):
        if not ordered:
            return list(_first_occurrence_form(pts))
        u, inv = np.unique(pts, axis=0, return_inverse=True)
        return [u, inv.reshape(-1)]

    return Case(dict(pts=pts), call, expect, outs=dict(uniq=(pts.shape, np.float64), inv=((len(pts),), np.int64)), compare=_equal)


def _case_scatter_elements():
    rng = np.random.default_rng(51)
    ncomp, nelem, P, nsel, nu = 2, 300, 27, 171, 2000
    values, inverse = rng.normal(size=(nu, ncomp)), rng.integers(0, nu, nsel * P)
    ids = np.sort(rng.choice(nelem, nsel, replace=False))
    before = rng.normal(size=(ncomp, nelem, P))

    def expect(ref):
        want = before.copy()
        want[:, ids] = values[inverse].reshape(nsel, P, ncomp).transpose(2, 0, 1)
        return [want]

    return Case(dict(values=values, inverse=inverse, ids=ids, out=before),
                lambda ctx, a, o: ctx.scatter_elements(a.values, a.inverse, a.ids, a.out), expect, inout=("out",))


def _case_fluid_solid(P):
    rng = np.random.default_rng(P)
    E, C, vs = 501, 3, 1
    assert (C * P) % 64 != 0
    values, previous = rng.uniform(1.0, 2.0, size=(E, C, P)), rng.uniform(5.0, 6.0, size=(E, C, P))
    solid = rng.random(E) > 0.3
    hit = rng.choice(E, 60, replace=False)
    values[hit[:30], vs, rng.integers(0, P, 30)] = 0.0
    values[hit[30:], vs, rng.integers(0, P, 30)] = -0.0             # -0.0 == 0.0: restored as well
    assert solid[hit[30:]].any()

    def expect(ref):                        # reference interpolator.py:829-841 on copies
        want = values.copy()
        want[~solid] = previous[~solid]
        restored = 0
        for elem in np.unique(np.where(want[:, vs, :] == 0.0)[0]):
            if solid[elem]:
                want[elem, :, :] = previous[elem, :, :]
                restored += 1
        return [restored, want]

    return Case(dict(values=values, previous=previous),
                lambda ctx, a, o: (ctx.fluid_solid_fix(a.values, a.previous, solid, vs), "values"), expect, inout=("values",))


def _case_first_occurrence():
    d = _hex8()
    return Case(dict(conn=d.ca), lambda ctx, a, o: ctx.first_occurrence(a.conn, len(d.pa)),
                lambda ref: [np.unique(d.ca, return_index=True)[1]], compare=_equal)


def _sphere():
    n = 3 * 4096 + 5
    rng = np.random.default_rng(11)
    pts = rng.uniform(-6.4e6, 6.4e6, size=(n, 3))
    pts[::1000] = 0.0
    return pts, rng.uniform(0.5, 1.0, size=n)


def _case_map_to_sphere():
    from test_sphere import map_to_sphere_numpy

    pts, z = _sphere()
    return Case(dict(pts=pts, z=z), lambda ctx, a, o: ctx.map_to_sphere(a.pts, a.z, out=o.out),
                lambda ref: [map_to_sphere_numpy(pts, z)], outs=dict(out=(pts.shape, np.float64)), compare=_equal)


def _case_sphere_ratio():
    pts, z = _sphere()
    return Case(dict(pts=pts, z=z), lambda ctx, a, o: ctx.sphere_ratio(a.pts, a.z),
                lambda ref: [(np.sqrt(np.sum(pts ** 2, axis=1)) / 6371000.0) / z], compare=_equal)


def _case_scale_points():
    pts, z = _sphere()
    return Case(dict(pts=pts, f=z), lambda ctx, a, o: ctx.scale_points(a.pts, a.f, out=o.out),
                lambda ref: [(z * pts.T).T], outs=dict(out=(pts.shape, np.float64)), compare=_equal)


CASES = {
    "centroid": _case_centroid,
    "knn_k8": lambda: _case_knn(8),
    "knn_k64": lambda: _case_knn(64),
    "locate_hex8_gather": _case_locate_hex8,
    "interpolate_hex8": lambda: _case_interpolate_hex8(False),
    "interpolate_hex8_operator": lambda: _case_interpolate_hex8(True),
    "source_interpolate_twice": _case_source_twice,
    "locate_gll_gather_elem_3d": lambda: _case_locate_gll(3),
    "locate_gll_gather_elem_2d": lambda: _case_locate_gll(2),
    "locate_gll_bbox_3d": lambda: _case_locate_gll_bbox(3),
    "locate_gll_bbox_2d": lambda: _case_locate_gll_bbox(2),
    "interpolate_gll_3d": lambda: _case_interpolate_gll(3),
    "interpolate_gll_2d": lambda: _case_interpolate_gll(2),
    "sample_columns_gll": _case_sample_columns,
    "sample_grid": _case_sample_grid,
    "transpose_nodes_apply": _case_transpose_nodes,
    "transpose_elem_apply": _case_transpose_elem,
    "gll_mass": _case_gll_mass,
    "weighted_sum": _case_weighted_sum,
    "divide_rows": _case_divide_rows,
    "diffusion_apply": _case_diffusion_apply,
    "smooth_two_steps": _case_smooth,
    "gll_gradient": _case_gradient,
    "gll_tensor_apply": _case_tensor_apply,
    "element_deviation": _case_element_deviation,
    "radial_bins": _case_radial_bins,
    "binned_weighted_sum": _case_binned_sum,
    "radial_model_apply": _case_radial_model,
    "point_taper": _case_point_taper,
    "order_statistics": _case_order_statistics,
    "clamp": _case_clamp,
    "unique_points_ordered": lambda: _case_unique(True),
    "unique_points_any_order": lambda: _case_unique(False),
    "scatter_elements": _case_scatter_elements,
    "fluid_solid_fix_P125": lambda: _case_fluid_solid(125),
    "fluid_solid_fix_P27": lambda: _case_fluid_solid(27),
    "first_occurrence": _case_first_occurrence,
    "map_to_sphere": _case_map_to_sphere,
    "sphere_ratio": _case_sphere_ratio,
    "scale_points": _case_scale_points,
}


@pytest.fixture(scope="module")
def reference(ctx_ref):
    """name -> (the case, its results on the null-stream context with NumPy inputs, seconds of a warm call there)"""
    runs = {}
    for name, make in CASES.items():
        case = make()
        _run_reference(ctx_ref, case)                       # (the first call grows the scratch pool)
        results, seconds = _run_reference(ctx_ref, case)
        runs[name] = (case, results, seconds)
    return runs


def _spin_ms(torch, side, cycles):
    with torch.cuda.stream(side):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        torch.cuda._sleep(cycles)
        end.record()
    side.synchronize()
    return begin.elapsed_time(end)


@pytest.fixture(scope="module")
def spin(torch, side, reference):
    """(cycles, the spin in ms as measured on ``side``, the slowest call's name, its ms)"""
    slowest = max(reference, key=lambda name: reference[name][2])
    slowest_ms = reference[slowest][2] * 1e3
    _spin_ms(torch, side, 1_000_000)
    per_cycle = _spin_ms(torch, side, 20_000_000) / 20_000_000
    cycles = int(math.ceil(max(SPIN_FACTOR * slowest_ms, SPIN_FLOOR_MS) / per_cycle))
    measured = min(_spin_ms(torch, side, cycles) for _ in range(3))
    return cycles, measured, slowest, slowest_ms


def test_the_spin_outlasts_the_slowest_call(spin, side):
    cycles, measured, slowest, slowest_ms = spin
    print(f"spin: {cycles} cycles = {measured:.2f} ms on the side stream; slowest call: {slowest}, {slowest_ms:.2f} ms")
    assert side.cuda_stream != 0
    assert measured >= 2.0 * slowest_ms, (measured, slowest, slowest_ms)
    assert measured < SPIN_LIMIT_MS, measured


@pytest.mark.parametrize("name", list(CASES))
def test_late_producer_early_consumer(torch, side, ctx_side, reference, spin, name):
    case, ref, _ = reference[name]
    compare = case.compare or _bits
    _same_as(ref, case.expect(ref), compare, (name, "null stream against the CPU"))
    got = _run_on_side(torch, side, ctx_side, case, spin[0])
    _same_as(got, ref, _bits, (name, "caller's stream against the null stream"))
    _same_as(got, case.expect(ref), compare, (name, "caller's stream against the CPU"))


# ------------------------------------------------------------------------------------------- the host path, called twice
def test_interpolate_hex8_host_twice_between_work_on_the_stream(torch, side, ctx_side, spin):
    """Host arrays in and out: the early-consumer half.  The second call reuses the buffer cache, which the library
    synchronises before its uploads; torch work is queued on ``side`` before each call and the result is read after."""
    d = _hex8()
    for _ in range(2):
        with torch.cuda.stream(side):
            busy = torch.zeros(1 << 20, device="cuda")
            torch.cuda._sleep(spin[0])
            busy += 1.0
            vals, enc, w, nf = ctx_side.interpolate_hex8_host(d.pa, d.ca, d.pb, d.fields, nelem_to_search=20, want_operator=True)
            after = busy.clone()
        assert nf == d.nf and np.array_equal(vals, d.vals) and np.array_equal(enc, d.enc) and np.array_equal(w, d.w)
        side.synchronize()
        assert float(after.sum().item()) == float(1 << 20)


# ------------------------------------------------------------------------ two contexts, two streams, two host threads
def test_two_threads_on_their_own_contexts_and_streams(torch, ctx_ref):
    d = _hex8()
    order, gp, rng, gfields, k = _gll(3)
    inputs = []
    for t in range(2):
        rounds = []
        for r in range(3):
            lo = 1000 * (3 * t + r)
            pts = np.ascontiguousarray(d.pb[lo:lo + 4000])
            gpts = np.random.default_rng(100 + 3 * t + r).uniform(-0.03, 1.03, size=(2000, 3))
            cloud = np.ascontiguousarray(synth.gll_mesh(5, 2, seed=60 + 3 * t + r).reshape(-1, 3))
            rounds.append((pts, gpts, cloud))
        inputs.append(rounds)

    def work(ctx, rounds):
        out = []
        for pts, gpts, cloud in rounds:
            v, nf = ctx.interpolate_hex8(d.pa, d.ca, pts, d.fields)
            g, miss = ctx.interpolate_gll(order, gp, gpts, gfields, nelem_to_search=k)
            u, inv = ctx.unique_points(cloud, ordered=False)
            out.append((v.numpy(), nf, g.numpy(), miss, u.numpy(), inv.numpy()))
        return out

    serial = [work(ctx_ref, rounds) for rounds in inputs]
    barrier = threading.Barrier(2)
    results, errors = [None, None], [None, None]

    def run(t):
        try:
            stream = torch.cuda.Stream()
            with Context(0, stream=stream.cuda_stream) as ctx:
                barrier.wait(timeout=30)
                results[t] = work(ctx, inputs[t])
        except BaseException as exc:   # noqa: BLE001 -- reported by the assertion below
            errors[t] = exc

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads)
    assert errors == [None, None], errors
    for t in range(2):
        for got, want in zip(results[t], serial[t]):
            for g, w in zip(got, want):
                assert (g == w) if isinstance(w, int) else _bits(g, w), t


# ----------------------------------------------------------------------------------------------- the shard interpolators
def test_shard_interpolators_called_under_another_stream(torch, ctx_ref, spin):
    from multimesh_amd.distributed import HipShardGllInterpolator, HipShardInterpolator

    d = _hex8()
    order, gp, rng, gfields, k = _gll(3)
    gpts = rng.uniform(0.02, 0.98, size=(3000, 3))
    want, nf = ctx_ref.interpolate_hex8(d.pa, d.ca, d.pb, d.fields, nelem_to_search=20)
    gwant, gmiss = ctx_ref.interpolate_gll(order, gp, gpts, gfields, nelem_to_search=k)
    want, gwant = want.numpy(), gwant.numpy()
    stream_a, stream_b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(stream_a):
        hex8 = HipShardInterpolator(d.pa, d.ca, d.fields, nelem_to_search=20, device_index=0)
        gll = HipShardGllInterpolator(gp, order, gfields, nelem_to_search=k, device_index=0)
    assert hex8.stream == stream_a.cuda_stream == gll.stream
    for shard, points, expected, count in ((hex8, d.pb, want, nf), (gll, gpts, gwant, gmiss)):
        staging = torch.from_numpy(points).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream_b):                       # the points are still in production on B when A reads them
            pts = torch.zeros_like(staging)
            torch.cuda._sleep(spin[0])
            pts.copy_(staging, non_blocking=True)
            out, n = shard(pts)
            got = out.clone()
            out.fill_(SENTINEL)
        stream_b.synchronize()
        assert n == count and _bits(got.cpu().numpy(), expected)
        with torch.cuda.stream(stream_a):                       # the captured stream is the current one: nothing is added
            out, n = shard(staging)
            got = out.clone()
        stream_a.synchronize()
        assert n == count and _bits(got.cpu().numpy(), expected)


# -------------------------------------------------------------------------------------- argument checks on the device
def test_tensor_arguments_on_the_device(torch, side, ctx_side):
    pts, z = _sphere()
    want = (z * pts.T).T
    lib = helpers.load_lib()
    with torch.cuda.stream(side):
        p, f = torch.from_numpy(pts).cuda(), torch.from_numpy(z).cuda()
        out = torch.full(pts.shape, float(SENTINEL), dtype=torch.float64, device="cuda")
        got = ctx_side.scale_points(p, f, out=out)              # a tensor on the context's GPU is written in place
        assert got.ptr == out.data_ptr() and got._keepalive is out
        ctx_side.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
        # a CPU tensor as input is copied, not wrapped
        copied = ctx_side.scale_points(torch.from_numpy(pts), torch.from_numpy(z))
        assert np.array_equal(copied.numpy(), want)
        # a CPU tensor as out is refused before anything is launched; the library's status is as it was
        ctx_side.synchronize()
        status, message = lib.mm_last_status(), lib.mm_last_error()
        host_out = torch.full(pts.shape, float(SENTINEL), dtype=torch.float64)
        out.fill_(float(SENTINEL))
        with pytest.raises(ValueError, match="out must live on GPU 0"):
            ctx_side.scale_points(p, f, out=host_out)
        with pytest.raises(ValueError, match="out must live on GPU 0"):
            ctx_side.interpolate_hex8(_hex8().pa, _hex8().ca, p, _hex8().fields, out=host_out)   # (_out without a message)
        assert lib.mm_last_status() == status and lib.mm_last_error() == message
        assert (host_out.numpy() == SENTINEL).all()
    side.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
