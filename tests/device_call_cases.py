"""What :mod:`multimesh_amd.device` passes to the library, recorded without a GPU: a stand-in library that logs every
``mm_*`` call (allocations and copies are real, in host memory), and a driver that calls every public method of ``Context``,
``KnnIndex``, ``Source``, ``TransposedOperator`` and ``Diffusion`` once per branch of its argument marshalling.

    python tests/device_call_cases.py --write     # writes tests/golden/device_calls.json from the package beside tests/

The fixture pins what the layer passed before it was given one call path: it was written from that commit's package and
is compared, never regenerated from the code under test (tests/test_device_calls.py).

The record of a case is ``{"log": [...], "returns": ...}`` or ``{"log": [...], "raises": [class, message]}``.  A log entry
is ``[symbol, arg, ...]`` with every argument the library got but a leading context handle when it is the context's own.
A ``to_device`` is ``["upload", dtype and shape, crc, allocation]`` when it made one allocation and one copy of the whole
array into it (the case "to_device" shows them in full), else ``["upload", dtype and shape, crc]`` and its calls.  A
scalar is its value (a float its ``hex()``); a pointer is "null", ``[allocation, offset, bytes of the allocation]``
(allocations count from zero within the case), a name or ``[name, offset]`` for memory the case named (the context
handle "ctx", a handle the library made, a host array, the stream), "host" for other host memory, "out" for a ``byref``
and "out-array[n]" for a ctypes array.  Releases (``mm_device_free``, ``*_destroy``) are logged only for an explicit
``free()`` / ``close()``: when the collector runs the others is not part of the record."""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multimesh_amd import helpers as H  # noqa: E402
from multimesh_amd.device import Context, DeviceArray, Diffusion, KnnIndex, Source, TransposedOperator  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "device_calls.json")
CLASSES = (Context, KnnIndex, Source, TransposedOperator, Diffusion)
CTX_HANDLE = 0xC0DE00
LAST_ERROR = b"stand-in: the library refused the arguments"
_SCALARS = (H.i32, H.i64, H.usize)
_PAD = 64        # bytes between the end of an allocation and anything else: an end pointer belongs to one allocation only


def crc(array):
    return zlib.crc32(np.ascontiguousarray(array).tobytes())


class RecordingLibrary:
    """A plain object in the place of ``multi_mesh_hip.so``: every ``mm_*`` attribute appends to ``log`` and returns 0 (or
    what ``returns`` names for the symbol; -1 once for the symbol in ``fail``)."""

    def __init__(self):
        self.begin()

    def begin(self, fail=None, returns=None, nactive=()):
        self.log, self.allocations, self.named = [], [], [(CTX_HANDLE, 0, "ctx")]
        self.fail, self.returns, self.nactive = fail, dict(returns or {}), list(nactive)
        self.handles = 0
        self.log_frees = False

    def name(self, name, array_or_address):
        """Name host memory (an array) or a bare address so that a pointer to it is recorded as ``[name, offset]``."""
        if isinstance(array_or_address, np.ndarray):
            self.named.append((array_or_address.ctypes.data, array_or_address.nbytes, name))
        else:
            self.named.append((int(array_or_address), 0, name))
        return array_or_address

    def where(self, address):
        if not address:
            return "null"
        for number, (base, nbytes, _) in enumerate(self.allocations):
            if base <= address <= base + nbytes:
                return [number, address - base, nbytes]
        for base, nbytes, name in self.named:
            if base <= address <= base + nbytes:
                return [name, address - base] if address != base else name
        return "host"

    def _arg(self, ctype, v):
        if ctype in _SCALARS:
            return int(v)
        if ctype is H.f64:
            return float(v).hex()
        if v is None:
            return "null"
        if isinstance(v, C.c_void_p):
            return self.where(v.value)
        if isinstance(v, (int, np.integer)):
            return self.where(int(v))
        if isinstance(v, C.Array):
            return f"out-array[{len(v)}]"
        return "out"

    def __getattr__(self, symbol):
        if not symbol.startswith("mm_"):
            raise AttributeError(symbol)
        return lambda *args: self._call(symbol, args)

    def _call(self, symbol, args):
        restype, argtypes = H.SIGNATURES[symbol]
        if symbol == "mm_last_error":
            self.log.append([symbol])
            return LAST_ERROR
        if len(args) != len(argtypes):
            raise TypeError(f"{symbol} takes {len(argtypes)} arguments, got {len(args)}")
        release = symbol == "mm_device_free" or symbol.endswith("_destroy")
        if not release or self.log_frees:
            entry = [self._arg(t, v) for t, v in zip(argtypes, args)]
            self.log.append([symbol] + entry[entry[:1] == ["ctx"]:])       # (the context's own handle is left out)
        if release:
            return None if restype is None else 0
        if self.fail == symbol:
            self.fail = None
            return -1
        getattr(self, "_do_" + symbol, lambda *a: None)(*args)
        if argtypes and argtypes[-1] == C.POINTER(H.vp) and symbol != "mm_device_alloc":
            self.handles += 1
            value = 0xA0000 + 0x100 * self.handles
            self.name(f"handle{self.handles}", value)
            args[-1]._obj.value = value
        rv = self.returns.get(symbol, 0)
        return rv.pop(0) if isinstance(rv, list) else rv

    # ---- the symbols that do something -------------------------------------------------------
    def _do_mm_device_alloc(self, handle, nbytes, out):
        buffer = C.create_string_buffer(int(nbytes) + _PAD)
        self.allocations.append((C.addressof(buffer), int(nbytes), buffer))
        out._obj.value = C.addressof(buffer)

    def _do_mm_copy_h2d(self, handle, dst, src, nbytes):
        C.memmove(dst, src, nbytes)

    _do_mm_copy_d2h = _do_mm_copy_h2d

    def _do_mm_memset(self, handle, dst, value, nbytes):
        C.memset(dst, value, nbytes)

    def _do_mm_pcg_scalars(self, handle, state, ncomp, phase, rtol, nactive):
        if nactive:                                  # the number of systems still active, as the case scripts it
            C.c_int64.from_address(nactive).value = self.nactive.pop(0) if self.nactive else 0

    def _do_mm_interpolate_hex8_host(self, handle, nodes, nnodes, conn, nelem, points, n, fields, ncomp, k, out, enc, w):
        for address, width, value in ((out, ncomp, 1), (enc, 8, 2), (w, 8, 3)):      # (np.empty arrays: give them contents)
            if address:
                C.memset(address, value, 8 * n * width)

    def _do_mm_last_knn_kernels(self, handle, out):
        out._obj.value = 0b100000101

    def _do_mm_last_locate_stats(self, handle, out):
        out[0], out[1], out[2] = 11, 12, 13

    def _do_mm_last_timings(self, handle, out, n):
        for i in range(n):
            out[i] = 0.5 * (i + 1)


class Driver:
    def __init__(self):
        self.lib = RecordingLibrary()
        self.record = {}
        self.fold = True

    def context(self):
        """A context that was never opened, on the stand-in: the real ``empty``, ``to_device`` and ``asdevice`` run
        (``to_device`` behind a recorder of what is uploaded)."""
        ctx = object.__new__(Context)
        ctx.lib, ctx.handle, ctx.device = self.lib, CTX_HANDLE, 0

        def to_device(array, dtype=None):
            a = np.ascontiguousarray(array, dtype=dtype)
            log, start = self.lib.log, len(self.lib.log)
            log.append(["upload", f"{a.dtype}{list(a.shape)}", crc(a)])
            d = Context.to_device(ctx, array, dtype)
            number = len(self.lib.allocations) - 1
            plain = [["mm_device_alloc", a.nbytes, "out"], ["mm_copy_h2d", [number, 0, a.nbytes], "host", a.nbytes]]
            if self.fold and log[start + 1:] == plain[:2 if a.nbytes else 1]:
                log[start:] = [log[start] + [number]]        # one allocation, one copy of the whole array: one entry
            return d

        ctx.to_device = to_device
        return ctx

    def brief(self, x):
        if x is None:
            return None
        if isinstance(x, DeviceArray):
            return self.lib.where(x.ptr)
        return type(x).__name__

    def describe(self, x):
        if isinstance(x, DeviceArray):       # "device float64[2, 3] at <pointer>", then what is not the default
            out = [f"device {x.dtype}{list(x.shape)}", self.lib.where(x.ptr)]
            return out + ([] if x._owner and x._keepalive is None else [{"owner": x._owner, "keeps": self.brief(x._keepalive)}])
        if isinstance(x, np.ndarray):
            return [f"numpy {x.dtype}{list(x.shape)}", crc(x)]
        if isinstance(x, (tuple, list)):
            return [self.describe(v) for v in x]
        if isinstance(x, (set, frozenset)):
            return sorted(x)
        if isinstance(x, dict):
            return {str(k): self.describe(v) for k, v in x.items()}
        if isinstance(x, (KnnIndex, Source, TransposedOperator, Diffusion)):
            out = {"class": type(x).__name__}
            for name in ("handle", "nsrc", "ndim", "npoints", "out_shape", "nodes", "conn", "_keepalive", "order", "gp",
                         "nelem", "P", "dim", "kappa_h", "kappa_r", "_deriv", "_weights"):
                if hasattr(x, name):
                    v = getattr(x, name)
                    out[name] = self.lib.where(v) if name == "handle" else self.describe(v)
            return out
        if isinstance(x, (bool, str)) or x is None:
            return x
        if isinstance(x, (int, np.integer)):
            return int(x)
        if isinstance(x, (float, np.floating)):
            return float(x).hex()
        return type(x).__name__

    def case(self, name, fn, fail=None, returns=None, nactive=(), fold=True):
        """Run ``fn(ctx)`` from a clean log; ``fail``: the symbol that returns -1 once; ``fold=False``: uploads in full."""
        assert name not in self.record, name
        self.lib.begin(fail, returns, nactive)
        self.fold = fold
        entry = {}
        try:
            entry["returns"] = self.describe(fn(self.context()))
        except Exception as e:      # (whatever the layer raises is the record)
            entry["raises"] = [type(e).__name__, str(e)]
        entry["log"] = self.lib.log
        self.record[name] = entry

    def freed(self, thing, method="free"):
        """``thing.free()`` with the releases it makes in the log."""
        self.lib.log_frees = True
        try:
            getattr(thing, method)()
        finally:
            self.lib.log_frees = False
        return thing


# ---- inputs: small, sizes that differ from one another, contents that differ per array -----------------------------------
N, E, NC, K, M = 5, 3, 2, 4, 9          # points, elements, components, list width, hex8 nodes


def f(shape, start):
    shape = shape if isinstance(shape, tuple) else (shape,)
    return (np.arange(int(np.prod(shape)), dtype=np.float64) * 0.5 + start).reshape(shape)


def ints(shape, start, mod, dtype=np.int64):
    shape = shape if isinstance(shape, tuple) else (shape,)
    return ((np.arange(int(np.prod(shape))) * 3 + start) % mod).astype(dtype).reshape(shape)


def flags(n):
    """n flags all off, then all on: every flag both ways, every optional array given and not given."""
    return [(False,) * n, (True,) * n]


NODES, CONN, POINTS, FIELDS = f((M, 3), 1.0), ints((E, 8), 1, M), f((N, 3), 100.0), f((NC, M), 200.0)
NEAREST = ints((N, K), 2, E)
GP3, GP2 = f((E, 8, 3), 300.0), f((E, 9, 2), 400.0)          # order 1 in 3-D (P = 8), order 2 in 2-D (P = 9)
EN3, EN2 = f((NC, E, 8), 500.0), f((NC, E, 9), 600.0)        # element-nodal fields over them
IDS, WEIGHTS = ints((N, K), 1, M), f((N, K), 700.0)
ELEM, COEFFS = ints((N,), 1, E), f((N, 8), 800.0)
GROUPS = f((E, 8, 3), 900.0)                                 # node groups [G, P, 3]


def build_cases(d):
    c = d.case
    lib = d.lib

    # ---- memory, timers, settings ---------------------------------------------------------------------------------
    c("empty", lambda x: [x.empty((3, 2), np.float64), x.empty(4, np.int32), x.empty((0, 3), np.float64)])
    c("zeros", lambda x: [x.zeros((3, 2), np.int64), x.zeros((0,), np.float64)])
    c("to_device", lambda x: [x.to_device(POINTS), x.to_device(IDS, np.int32), x.to_device(np.zeros((0, 3)))], fold=False)
    c("asdevice", lambda x: [x.asdevice(POINTS, np.float64), x.asdevice([1, 2, 3], np.int64)])
    c("asdevice.wrapped", lambda x: (lambda a: [a, x.asdevice(a, np.float64) is a])(x.empty((2,), np.float64)))
    c("numpy", lambda x: [x.to_device(POINTS).numpy(), x.to_device(POINTS).rows(1, 3).numpy(),
                           x.to_device(POINTS).reshape(3, N).numpy(), x.empty((0, 2), np.float64).numpy()])
    c("array.free", lambda x: d.freed(x.empty((3,), np.float64)).ptr)
    c("synchronize", lambda x: x.synchronize())
    c("synchronize.fails", lambda x: x.synchronize(), fail="mm_synchronize")
    for on in (False, True, 2, 1):
        c(f"set_profiling.{on!r}", lambda x, on=on: x.set_profiling(on))
    for on in (False, True):
        c(f"set_lazy_lists.{on}", lambda x, on=on: x.set_lazy_lists(on))
    for mode in ("exact", "tol", H.MM_FP_TOL):
        c(f"set_fp_mode.{mode}", lambda x, mode=mode: x.set_fp_mode(mode))
    c("fp_mode.exact", lambda x: x.fp_mode())
    c("fp_mode.tol", lambda x: x.fp_mode(), returns={"mm_get_fp_mode": H.MM_FP_TOL})
    c("last_locate_stats", lambda x: x.last_locate_stats())
    c("last_knn_kernels", lambda x: x.last_knn_kernels())
    c("last_timings", lambda x: x.last_timings())

    def opened(x):
        lib.name("stream", 0x51234)                 # (Context() finds the stand-in through load_lib(): see drive())
        return [(lambda k: (k.handle == lib.named[-1][0], k.device, d.freed(k, "close").handle))(Context(1, s))
                for s in (None, 0x51234)]
    c("Context.open_close", opened)

    # ---- hex8 -----------------------------------------------------------------------------------------------------
    c("centroid", lambda x: x.centroid(CONN, NODES))
    c("knn_build", lambda x: x.knn_build(f((M, 2), 3.0)))
    c("knn_build.shape", lambda x: x.knn_build(f((M, 4), 3.0)))
    for want in (False, True):
        c(f"KnnIndex.query.dist={want}", lambda x, want=want: x.knn_build(NODES).query(POINTS, K, want_dist=want))
    c("KnnIndex.query.fails", lambda x: x.knn_build(NODES).query(POINTS, K), fail="mm_knn_query")
    c("KnnIndex.free", lambda x: d.freed(x.knn_build(NODES)))
    for given, exodus in flags(2):
        c(f"locate_hex8.given={given}.exodus={exodus}", lambda x, given=given, exodus=exodus: x.locate_hex8(
            NEAREST, CONN, NODES, POINTS, enc=x.zeros((N, 8), np.int64) if given else None,
            weights=x.zeros((N, 8), np.float64) if given else None, conn_is_exodus=exodus))
    c("locate_hex8.flat_list", lambda x: x.locate_hex8(ints((N,), 0, E), CONN, NODES, POINTS))
    for pm in (True, False):
        c(f"gather.point_major={pm}", lambda x, pm=pm: x.gather(FIELDS, IDS, WEIGHTS, point_major=pm))
    c("gather.one_component", lambda x: x.gather(FIELDS[0], IDS, WEIGHTS))
    c("gather.shape", lambda x: x.gather(FIELDS, IDS, WEIGHTS[:, :2]))
    for op, out in flags(2):
        c(f"interpolate_hex8.operator={op}.out={out}", lambda x, op=op, out=out: x.interpolate_hex8(
            NODES, CONN, POINTS, FIELDS, nelem_to_search=7, want_operator=op,
            out=x.empty((N, NC), np.float64) if out else None))
        c(f"Source.interpolate.operator={op}.out={out}", lambda x, op=op, out=out: x.source(NODES, CONN).interpolate(
            POINTS, FIELDS, nelem_to_search=6, want_operator=op, out=x.empty((N, NC), np.float64) if out else None))

        def host(x, op=op, out=out):
            arrays = [lib.name(n, a.copy()) for n, a in (("nodes", NODES), ("conn", CONN), ("points", POINTS),
                                                          ("fields", FIELDS))]
            return x.interpolate_hex8_host(*arrays, nelem_to_search=5, want_operator=op,
                                           out=lib.name("out", np.zeros((N, NC))) if out else None)
        c(f"interpolate_hex8_host.operator={op}.out={out}", host)
    c("source", lambda x: x.source(NODES, CONN))
    c("Source.free", lambda x: d.freed(x.source(NODES, CONN)))
    c("interpolate_hex8.fields", lambda x: x.interpolate_hex8(NODES, CONN, POINTS, FIELDS[:, :4]))

    # ---- GLL: locate, gather, the transposes ------------------------------------------------------------------------
    for snap in (False, True):
        c(f"locate_gll.snap={snap}", lambda x, snap=snap: x.locate_gll(1, NEAREST, GP3, POINTS, tolerance=1.25,
                                                                         snap_to_nearest=snap))
    c("locate_gll.2d", lambda x: x.locate_gll(2, NEAREST, GP2, f((N, 2), 5.0)))
    c("locate_gll.flat_list", lambda x: x.locate_gll(1, ints((N,), 0, E), GP3, POINTS))
    c("locate_gll.shape", lambda x: x.locate_gll(2, NEAREST, GP3, POINTS))
    c("locate_gll_bbox", lambda x: x.locate_gll_bbox(1, NEAREST, GP3, POINTS))
    c("locate_gll_bbox.fails", lambda x: x.locate_gll_bbox(1, NEAREST, GP3, POINTS), fail="mm_locate_gll_bbox")
    for pm in (True, False):
        c(f"gather_elem.point_major={pm}", lambda x, pm=pm: x.gather_elem(EN3, ELEM, COEFFS, point_major=pm))
    c("gather_elem.one_component", lambda x: x.gather_elem(EN3[0], ELEM, COEFFS))
    c("transpose_nodes", lambda x: x.transpose_nodes(IDS, WEIGHTS, M))
    c("transpose_elem", lambda x: x.transpose_elem(ELEM, COEFFS, E))
    c("transpose_elem.shape", lambda x: x.transpose_elem(ELEM, COEFFS[:3], E))
    for pm, out in flags(2):
        c(f"TransposedOperator.apply.point_major={pm}.out={out}", lambda x, pm=pm, out=out: x.transpose_nodes(
            IDS, WEIGHTS, M).apply(f((N, NC) if pm else (NC, N), 9.0), point_major=pm,
                                   out=x.empty((NC, M), np.float64) if out else None))
    for pm in (True, False):
        c(f"TransposedOperator.apply.flat.point_major={pm}", lambda x, pm=pm: x.transpose_elem(ELEM, COEFFS, E).apply(
            f((N,), 9.0), point_major=pm))
    c("TransposedOperator.apply.shape", lambda x: x.transpose_nodes(IDS, WEIGHTS, M).apply(f((N + 1, NC), 9.0)))
    c("TransposedOperator.apply.out_shape", lambda x: x.transpose_nodes(IDS, WEIGHTS, M).apply(
        f((N, NC), 9.0), out=x.empty((M, NC), np.float64)))
    c("TransposedOperator.free", lambda x: (lambda op: [d.freed(op), d.freed(op)])(x.transpose_elem(ELEM, COEFFS, E)))
    c("TransposedOperator.apply.freed", lambda x: d.freed(x.transpose_nodes(IDS, WEIGHTS, M)).apply(f((N, NC), 9.0)))
    for op, snap, out in flags(3):
        c(f"interpolate_gll.operator={op}.snap={snap}.out={out}", lambda x, op=op, snap=snap, out=out: x.interpolate_gll(
            1, GP3, POINTS, EN3, nelem_to_search=6, tolerance=1.5, snap_to_nearest=snap, want_operator=op,
            out=x.empty((N, NC), np.float64) if out else None))
    c("interpolate_gll.out_shape", lambda x: x.interpolate_gll(1, GP3, POINTS, EN3, out=x.empty((NC, N), np.float64)))

    # ---- mass, sums --------------------------------------------------------------------------------------------------
    for det in (False, True):
        c(f"gll_mass.det={det}", lambda x, det=det: x.gll_mass(2, GP2, want_det=det))
    c("gll_mass.3d", lambda x: x.gll_mass(1, GP3))
    c("gll_mass.shape", lambda x: x.gll_mass(2, GP3))
    mass = f((E, 9), 20.0)
    c("weighted_sum.none", lambda x: x.weighted_sum(mass))
    c("weighted_sum.one", lambda x: x.weighted_sum(mass, f((E, 9), 21.0)))
    c("weighted_sum.many", lambda x: x.weighted_sum(mass, EN2))
    c("weighted_sum.shape", lambda x: x.weighted_sum(mass, EN3))
    for out in (False, True):
        c(f"divide_rows.out={out}", lambda x, out=out: x.divide_rows(EN2, mass, out=x.empty(EN2.shape, np.float64)
                                                                     if out else None))
    c("divide_rows.in_place", lambda x: (lambda a: x.divide_rows(a, mass, out=a))(x.to_device(EN2)))
    c("divide_rows.shape", lambda x: x.divide_rows(EN3, mass))

    # ---- radial profiles ---------------------------------------------------------------------------------------------
    edges = f((4,), 1.0)
    for want in (False, True):
        c(f"radial_bins.radius={want}", lambda x, want=want: x.radial_bins(GROUPS, edges, want_radius=want))
    c("radial_bins.refused", lambda x: x.radial_bins(GROUPS, edges), fail="mm_radial_bins")
    c("radial_bins.count", lambda x: x.radial_bins(GROUPS, edges), returns={"mm_radial_bins": 3})
    c("radial_bins.points", lambda x: x.radial_bins(f((N, 2), 0.0), edges))
    bins = ints((E, 9), 0, 3, np.int32)
    for fields, square, count in flags(3):
        c(f"binned_weighted_sum.fields={fields}.square={square}.count={count}",
          lambda x, fields=fields, square=square, count=count: x.binned_weighted_sum(
              mass, bins, 3, fields=EN2 if fields else None, square=square, want_count=count))
    table_r, table_v = f((6,), 10.0), f((NC, 6), 30.0)
    c("radial_model_apply.groups", lambda x: x.radial_model_apply(GROUPS, table_r, table_v))
    c("radial_model_apply.points", lambda x: x.radial_model_apply(POINTS, table_r, table_v[0]))
    for out in (False, True):
        c(f"radial_model_apply.mode=2.out={out}", lambda x, out=out: x.radial_model_apply(
            GROUPS, table_r, table_v, mode=2, values_in=f((NC, E, 8), 40.0),
            out=x.empty((NC, E * 8), np.float64) if out else None))
    c("radial_model_apply.refused", lambda x: x.radial_model_apply(GROUPS, table_r, table_v), fail="mm_radial_model_apply")
    c("radial_model_apply.points_shape", lambda x: x.radial_model_apply(f((N, 2), 0.0), table_r, table_v))
    c("radial_model_apply.group_size", lambda x: x.radial_model_apply(f((2, 257, 3), 0.0), table_r, table_v))
    c("radial_model_apply.out_size", lambda x: x.radial_model_apply(GROUPS, table_r, table_v, out=x.empty((3,), np.float64)))

    # ---- preconditioning -----------------------------------------------------------------------------------------------
    centres, inner, outer = f((K, 3), 50.0), f((K,), 1.0), f((K,), 60.0)
    for values, out, weight in ((True, True, True), (True, False, False), (False, False, True), (False, False, False),
                                (False, True, True)):
        c(f"point_taper.values={values}.out={out}.weight={weight}", lambda x, values=values, out=out, weight=weight:
          x.point_taper(GROUPS, centres, inner, outer, values_in=f((NC, E, 8), 70.0) if values else None,
                        out=x.empty((NC, E, 8), np.float64) if out else None, want_weight=weight))
    c("point_taper.points", lambda x: x.point_taper(POINTS, centres, inner, outer, values_in=f((N,), 70.0)))
    c("point_taper.refused", lambda x: x.point_taper(POINTS, centres, inner, outer, want_weight=True), fail="mm_point_taper")
    c("point_taper.points_shape", lambda x: x.point_taper(f((N,), 0.0), centres, inner, outer, want_weight=True))
    c("point_taper.group_size", lambda x: x.point_taper(f((2, 257, 3), 0.0), centres, inner, outer, want_weight=True))
    q = np.array([0.25, 0.5, 1.0])
    for absolute, method in ((False, "lower"), (True, "higher")):
        c(f"order_statistics.absolute={absolute}.{method}", lambda x, absolute=absolute, method=method:
          x.order_statistics(EN3, q, absolute=absolute, method=method))
    c("order_statistics.flat", lambda x: x.order_statistics(f((7,), 1.0), 0.5))
    c("order_statistics.device_q", lambda x: x.order_statistics(EN3, x.to_device(q)))
    c("order_statistics.refused", lambda x: x.order_statistics(EN3, q), fail="mm_order_statistics")
    c("order_statistics.scalar", lambda x: x.order_statistics(x.empty((), np.float64), q))
    lower, upper = f((NC,), -5.0), f((NC,), 5.0)
    for lo, hi, count, out in flags(4):
        c(f"clamp.lower={lo}.upper={hi}.count={count}.out={out}", lambda x, lo=lo, hi=hi, count=count, out=out: x.clamp(
            EN3, lower=lower if lo else None, upper=upper if hi else None, want_count=count,
            out=x.empty(EN3.shape, np.float64) if out else None))
    c("clamp.symmetric", lambda x: x.clamp(f((7,), 1.0), upper=x.to_device(f((1,), 2.0)), symmetric=True))
    c("clamp.refused", lambda x: x.clamp(EN3, upper=upper), fail="mm_clamp")
    c("clamp.scalar", lambda x: x.clamp(x.empty((), np.float64), upper=upper))
    c("clamp.bounds", lambda x: x.clamp(EN3, upper=f((3,), 1.0)))

    # ---- boundaries ----------------------------------------------------------------------------------------------------
    corner_ids, faces, side = ints((E, 8), 0, M), ints((4,), 0, 6 * E), ints((4,), 0, 3, np.int32)
    c("boundary_faces", lambda x: x.boundary_faces(corner_ids, M), returns={"mm_boundary_faces": 4})
    c("boundary_faces.refused", lambda x: x.boundary_faces(corner_ids, M), fail="mm_boundary_faces")
    for up in (None, (0.0, 0.5, 1.0)):
        c(f"boundary_classify.up={up}", lambda x, up=up: x.boundary_classify(GP3, faces, up=up, cos_min=0.75))
    c("boundary_classify.refused", lambda x: x.boundary_classify(GP3, faces), fail="mm_boundary_classify")
    for given in (False, True):
        c(f"boundary_nodes.side={given}", lambda x, given=given: x.boundary_nodes(
            GP3, 1, faces, side=side if given else None, side_mask=5), returns={"mm_boundary_nodes": 8})
    c("boundary_nodes.refused", lambda x: x.boundary_nodes(GP3, 1, faces), fail="mm_boundary_nodes")
    c("boundary_nodes.side_shape", lambda x: x.boundary_nodes(GP3, 1, faces, side=side[:2]))
    c("cutoff_distance", lambda x: x.cutoff_distance(GROUPS, centres, 2.5), returns={"mm_cutoff_distance": 2})
    c("cutoff_distance.refused", lambda x: x.cutoff_distance(GROUPS, centres, 2.5), fail="mm_cutoff_distance")
    dist = f((E, 8), 1.0)
    for a, b, elem, out, weight in ((True,) * 5, (True, False, False, False, False), (False, False, True, False, True),
                                    (False,) * 5):
        c(f"distance_taper.a={a}.b={b}.elem={elem}.out={out}.weight={weight}",
          lambda x, a=a, b=b, elem=elem, out=out, weight=weight: x.distance_taper(
              dist, 0.5, 2.0, f((NC, E, 8), 3.0) if a else None, b=f((NC, E, 8), 4.0) if b else None,
              elem=ints((E, 8), 0, 3) - 1 if elem else None, out=x.empty((NC, E, 8), np.float64) if out else None,
              want_weight=weight))
    c("distance_taper.one_component", lambda x: x.distance_taper(dist, 0.5, 2.0, f((E, 8), 3.0)))
    c("distance_taper.refused", lambda x: x.distance_taper(dist, 0.5, 2.0, None, want_weight=True), fail="mm_distance_taper")
    c("distance_taper.b_alone", lambda x: x.distance_taper(dist, 0.5, 2.0, None, b=f((E, 8), 3.0)))

    # ---- scattered models ------------------------------------------------------------------------------------------------
    idx, kd = ints((N, K), 0, M), f((N, K), 0.0)
    for pm, nearest, count, out in flags(4):
        c(f"idw_gather.point_major={pm}.nearest={nearest}.count={count}.out={out}",
          lambda x, pm=pm, nearest=nearest, count=count, out=out: x.idw_gather(
              FIELDS, idx, kd, power=3, max_distance=2.5, fill_value=-1.5, point_major=pm, want_nearest=nearest,
              want_count=count, out=x.empty((N, NC) if pm else (NC, N), np.float64) if out else None))
    c("idw_gather.keep", lambda x: x.idw_gather(FIELDS[0], idx, kd, outside="keep", out=x.empty((1, N), np.float64)),
      returns={"mm_idw_gather": 2})
    c("idw_gather.keep_without_out", lambda x: x.idw_gather(FIELDS, idx, kd, outside="keep"))
    c("idw_gather.refused", lambda x: x.idw_gather(FIELDS, idx, kd), fail="mm_idw_gather")
    c("idw_gather.out_shape", lambda x: x.idw_gather(FIELDS, idx, kd, out=x.empty((N, NC), np.float64)))

    # ---- resolution --------------------------------------------------------------------------------------------------------
    for fast, slow, spacing in ((False, False, False), (True, False, True), (True, True, False), (False, False, True)):
        c(f"gll_resolution.fast={fast}.slow={slow}.spacing={spacing}", lambda x, fast=fast, slow=slow, spacing=spacing:
          x.gll_resolution(2, GP2, fast=EN2 if fast else None, slow=f((3, E, 9), 8.0) if slow else None,
                           want_node_spacing=spacing))
    c("gll_resolution.one_component", lambda x: x.gll_resolution(2, GP2, fast=EN2[0]))
    c("gll_resolution.refused", lambda x: x.gll_resolution(2, GP2), fail="mm_gll_resolution")
    c("gll_resolution.fast_shape", lambda x: x.gll_resolution(2, GP2, fast=EN3))
    for want in (False, True):
        c(f"arg_extreme.max={want}", lambda x, want=want: x.arg_extreme(EN3, want_max=want))
    c("arg_extreme.flat", lambda x: x.arg_extreme(f((7,), 1.0)))
    c("arg_extreme.refused", lambda x: x.arg_extreme(EN3), fail="mm_arg_extreme")
    c("arg_extreme.scalar", lambda x: x.arg_extreme(x.empty((), np.float64)))

    # ---- gradient, order change ------------------------------------------------------------------------------------------------
    for grad, radial, lateral, norm in ((True,) * 4, (True, False, False, False), (False, True, True, True), (False,) * 4):
        c(f"gll_gradient.{grad}.{radial}.{lateral}.{norm}", lambda x, g=(grad, radial, lateral, norm):
          x.gll_gradient(1, GP3, EN3, *g))
    c("gll_gradient.2d", lambda x: x.gll_gradient(2, GP2, EN2[0]))
    c("gll_gradient.fails", lambda x: x.gll_gradient(2, GP2, EN2), fail="mm_gll_gradient")
    for layout, shape in ((0, (NC, E, 9)), (1, (E, 9, NC)), (2, (E, NC, 9))):
        for transpose, extras in flags(2):
            c(f"gll_tensor_apply.layout={layout}.transpose={transpose}.extras={extras}",
              lambda x, layout=layout, shape=shape, transpose=transpose, extras=extras: x.gll_tensor_apply(
                  2, 1, 2, f(shape, 2.0), layout=layout, transpose=transpose,
                  scale_in=f((E, 9), 3.0) if extras else None, div_out=f((E, 4), 4.0) if extras else None,
                  out=x.empty(((NC, E, 4), (E, 4, NC), (E, NC, 4))[layout], np.float64) if extras else None))
    c("gll_tensor_apply.one_component", lambda x: x.gll_tensor_apply(1, 2, 3, f((E, 8), 2.0)))
    c("gll_tensor_apply.out_shape", lambda x: x.gll_tensor_apply(2, 1, 2, f((NC, E, 9), 2.0), out=x.empty((NC, E, 9), np.float64)))
    c("element_deviation", lambda x: x.element_deviation(GP3, f((E, 8, 3), 301.0)))

    # ---- grids ---------------------------------------------------------------------------------------------------------------
    lat_t, lon_t, rad = f((3, 2), 0.0), f((4, 2), 1.0), f((2,), 6.0e6)
    for paired, want, out in flags(3):
        c(f"sample_columns_gll.paired={paired}.points={want}.out={out}", lambda x, paired=paired, want=want, out=out:
          x.sample_columns_gll(1, GP3, EN3, lat_t, f((3, 2), 1.0) if paired else lon_t, rad, paired=paired,
                               nelem_to_search=9, tolerance=1.25, fill_value=-2.0, chunk_points=5 if want else None,
                               want_points=want, out=x.empty((NC, 2, 3 if paired else 12), np.float64) if out else None))
    depth, lat, lon = f((2,), 0.0), f((3,), -1.0), np.array([0.0, 90.0, 180.0, 360.0])
    cube = f((NC, 2, 3, 4), 5.0)
    for outside in ("fill", "clamp", "keep"):
        for periodic, want in flags(2):
            c(f"sample_grid.{outside}.periodic={periodic}.lld={want}", lambda x, outside=outside, periodic=periodic,
              want=want: x.sample_grid(GROUPS, cube, depth, lat, lon, outside=outside, fill_value=-3.0, lon_periodic=periodic,
                                       out=x.empty((NC, E, 8), np.float64) if outside == "keep" else None,
                                       want_latlondepth=want))
    c("sample_grid.one_component", lambda x: x.sample_grid(POINTS, cube[0], x.to_device(depth), lat, lon))
    c("sample_grid.keep_without_out", lambda x: x.sample_grid(POINTS, cube, depth, lat, lon, outside="keep"))
    c("sample_grid.axis", lambda x: x.sample_grid(POINTS, cube, depth, lat[::-1], lon))
    c("sample_grid.fails", lambda x: x.sample_grid(POINTS, cube, depth, lat, lon), fail="mm_sample_grid")
    for clamp, periodic, lld, given in flags(4):
        c(f"grid_operator.clamp={clamp}.periodic={periodic}.lld={lld}.out={given}",
          lambda x, clamp=clamp, periodic=periodic, lld=lld, given=given: x.grid_operator(
              POINTS, depth, lat, lon, clamp=clamp, lon_periodic=periodic, latlondepth=lld,
              ids_out=x.empty((N, 8), np.int64) if given else None,
              weights_out=x.empty((N, 8), np.float64) if given else None))
    c("grid_operator.out_shape", lambda x: x.grid_operator(POINTS, depth, lat, lon, ids_out=x.empty((N, 4), np.int64)))

    # ---- layers, the sphere, unique points ----------------------------------------------------------------------------------------
    c("scatter_elements", lambda x: x.scatter_elements(f((7, NC), 1.0), ints((2 * 8,), 0, 7), ints((2,), 1, E),
                                                        x.zeros((NC, E, 8), np.float64)))
    c("fluid_solid_fix", lambda x: x.fluid_solid_fix(x.to_device(f((E, NC, 8), 1.0)), f((E, NC, 8), 2.0),
                                                      np.array([True, False, True]), 1), returns={"mm_fluid_solid_fix": 2})
    c("first_occurrence", lambda x: x.first_occurrence(CONN, M))
    c("first_occurrence.refused", lambda x: x.first_occurrence(CONN, M), fail="mm_first_occurrence")
    c("first_occurrence.unreferenced", lambda x: x.first_occurrence(CONN, M), returns={"mm_first_occurrence": 2})
    rad_en, conn_en = f((E, 8), 6.0e6), ints((E, 8), 0, N)
    c("map_to_sphere.element_nodal", lambda x: x.map_to_sphere(GROUPS, rad_en, r_ref=6.0e6))
    c("map_to_sphere.connectivity", lambda x: x.map_to_sphere(POINTS, rad_en, connectivity=conn_en))
    c("map_to_sphere.first", lambda x: x.map_to_sphere(POINTS, rad_en, first=ints((N,), 0, 24)))
    c("map_to_sphere.out", lambda x: x.map_to_sphere(GROUPS, rad_en, out=x.empty((E * 8, 3), np.float64)))
    c("map_to_sphere.in_place", lambda x: (lambda p: x.map_to_sphere(p, rad_en, out=p))(x.to_device(GROUPS)))
    c("map_to_sphere.host_out", lambda x: x.map_to_sphere(GROUPS, rad_en, out=lib.name("out", np.ones(GROUPS.shape))))
    c("map_to_sphere.host_in_place", lambda x: (lambda p: x.map_to_sphere(p, rad_en, out=p))(lib.name("points", GROUPS + 1.0)))
    c("map_to_sphere.rad_size", lambda x: x.map_to_sphere(POINTS, rad_en))
    for layout in ("element_nodal", "connectivity", "first"):
        c(f"sphere_ratio.{layout}", lambda x, layout=layout: x.sphere_ratio(
            GROUPS if layout == "element_nodal" else POINTS, rad_en, r_ref=6.0e6,
            connectivity=conn_en if layout == "connectivity" else None,
            first=x.to_device(ints((N,), 0, 24)) if layout == "first" else None))
    for out in (False, True):
        c(f"scale_points.out={out}", lambda x, out=out: x.scale_points(GROUPS, f((E, 8), 2.0),
                                                                       out=x.empty(GROUPS.shape, np.float64) if out else None))
    c("scale_points.fails", lambda x: x.scale_points(GROUPS, f((E, 8), 2.0)), fail="mm_scale_points")
    for ordered, given in flags(2):
        c(f"unique_points.ordered={ordered}.out={given}", lambda x, ordered=ordered, given=given: x.unique_points(
            POINTS, unique_out=x.empty((N + 1, 3), np.float64) if given else None,
            inverse_out=x.empty((N + 2,), np.int64) if given else None, ordered=ordered),
          returns={"mm_unique_points": 4, "mm_unique_points_any_order": 3})
    for ordered in (True, False):
        c(f"unique_points.ordered={ordered}.fails", lambda x, ordered=ordered: x.unique_points(POINTS, ordered=ordered),
          fail="mm_unique_points" if ordered else "mm_unique_points_any_order")
    c("unique_points.empty", lambda x: x.unique_points(np.zeros((0, 3))))

    # ---- diffusion -----------------------------------------------------------------------------------------------------------------
    c("diffusion.scalar", lambda x: x.diffusion(2, GP2, kappa_h=2.5))
    c("diffusion.arrays", lambda x: x.diffusion(1, GP3, kappa_h=f((E, 8), 1.0), kappa_r=x.to_device(f((E, 8), 2.0))))
    c("diffusion.radial_in_2d", lambda x: x.diffusion(2, GP2, kappa_r=1.0))
    kappas = {"scalar": lambda x: dict(kappa_h=2.5), "radial": lambda x: dict(kappa_h=1.5, kappa_r=0.5),
              "arrays": lambda x: dict(kappa_h=f((E, 8), 1.0), kappa_r=f((E, 8), 2.0))}
    for name, kw in kappas.items():
        for out in ((False, True) if name == "arrays" else (False,)):
            c(f"Diffusion.apply.{name}.out={out}", lambda x, kw=kw, out=out: x.diffusion(1, GP3, **kw(x)).apply(
                EN3, out=x.empty(EN3.shape, np.float64) if out else None))
    c("Diffusion.apply.in_place", lambda x: (lambda u: x.diffusion(1, GP3).apply(u, out=u))(x.to_device(EN3)))
    c("Diffusion.apply.fails", lambda x: x.diffusion(1, GP3).apply(EN3), fail="mm_gll_diffusion_apply")
    c("Diffusion.roughness", lambda x: x.diffusion(1, GP3, kappa_h=2.0).roughness(EN3))
    any_order = {"mm_unique_points_any_order": 7}
    c("Diffusion.smooth.steps=0", lambda x: (lambda k: [k.smooth(EN3[0], steps=0), k.last_iterations])(x.diffusion(1, GP3)),
      returns=any_order)
    c("Diffusion.smooth.steps=1", lambda x: (lambda k: [k.smooth(EN3, steps=1, max_iter=1), k.last_iterations])(
        x.diffusion(1, GP3, kappa_h=1.5, kappa_r=0.5)), returns=any_order, nactive=[NC, 0])
    c("Diffusion.smooth.no_convergence", lambda x: x.diffusion(1, GP3).smooth(EN3, steps=1, max_iter=1),
      returns=any_order, nactive=[NC, NC])
    c("Diffusion.free", lambda x: (lambda k: [k.smooth(EN3, steps=0), d.freed(k), d.freed(k)])(x.diffusion(1, GP3)),
      returns=any_order)
    c("Diffusion.apply.freed", lambda x: d.freed(x.diffusion(1, GP3)).apply(EN3))

    # ---- the two functions of the api package that hold a library call of their own ---------------------------------------------
    from multimesh_amd import api
    c("api.query_gll_model", lambda x: api.query_gll_model(GP3, f((E, NC, 8), 1.0), POINTS, nelem_to_search=K, context=x))
    api_cases(d)
    c("Context.close", lambda x: d.freed(x, "close").handle)


def api_cases(d):
    from multimesh_amd import api
    grid = api.RegularGrid(np.array([0.0, 1000.0]), np.array([-10.0, 0.0, 10.0]), np.array([0.0, 10.0, 20.0, 30.0]),
                           {"VS": f((2, 3, 4), 1.0)})
    mesh = api.GllMesh(GP3, 1, {"VS": f((E, 8), 2.0), "VP": f((E, 8), 3.0)})
    for mass in (True, False):
        d.case(f"api.regular_grid_adjoint.mass={mass}", lambda x, mass=mass: (lambda g: [g.data_vars, g.nmissing])(
            api.regular_grid_adjoint(grid, mesh, ["VS", "VP"], mass=mass, context=x)))


def drive():
    d = Driver()
    cache = H.cache[:]
    H.cache[:] = [d.lib]            # (helpers.check reads the library's last error through load_lib())
    try:
        build_cases(d)
    finally:
        H.cache[:] = cache
    return d.record


def signatures():
    """name -> str(inspect.signature) of every public method of the five classes."""
    import inspect
    return {f"{cls.__name__}.{name}": str(inspect.signature(getattr(cls, name))) for cls in CLASSES
            for name in dir(cls) if not name.startswith("_") and callable(getattr(cls, name))}


def dump(record, path):
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in record.items()) + "\n}\n")


if __name__ == "__main__":
    if "--signatures" in sys.argv:
        for k, v in signatures().items():
            print(f'    "{k}": {v!r},')
    elif "--write" in sys.argv:
        dump(drive(), FIXTURE)
        print(f"wrote {FIXTURE}")
    else:
        rec = drive()
        for k, v in rec.items():
            if "raises" in v:
                print(k, v["raises"])
        print(len(rec), "cases;", sorted({e[0] for v in rec.values() for e in v["log"]}))
