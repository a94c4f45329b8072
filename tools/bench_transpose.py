#!/usr/bin/env python3
"""The operator transpose (mm_transpose_*) at the sizes the forward gather is measured at, beside the forward gather on
the SAME operator in the same run (it moves the same operator bytes once) and the host route it replaces.

  metric      10,077,696 hex8 targets -> 10,077,696 nodes (the operator shape of tools/bench_gather.py), rows of ~8
  cfg4_shard  one rank's 12.6 M targets of the 465^3 mesh -> the 10 M-node source: they cover an eighth of it, rows of ~64
  cfg5_gll    order-4 GLL, 43^3 source elements, the unique points of a 47^3-element target mesh (device pipeline)

Per operator: create ms (wall clock, the call synchronises), apply ms at C = 1 and C = 3 (stage timer, median of 10),
forward ms, apply / forward, counted bytes over time as a fraction of 8 TB/s.  Counted bytes, node form: 8 + 4 per
contribution read, 8 C gathered per contribution, 8 C written per destination; element form: the coefficient rows and 4 B
of permutation per target, 8 C of values per target, 8 C P written per element.  One JSON line per case, also written to
--out (default profiles/transpose_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimesh_amd import synth
from multimesh_amd.device import Context

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "transpose_bench.json"))
ap.add_argument("--n-src", type=int, default=216, help="nodes per side of the hex8 source mesh")
ap.add_argument("--gll-src", type=int, default=44)
ap.add_argument("--gll-tgt", type=int, default=48)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--cases", default="metric,cfg4_shard,cfg5_gll,host_route")
a = ap.parse_args()
cases = a.cases.split(",")
ctx = Context(0)
ctx.set_profiling(True)
lines = []


def timed(fn, stage="gather"):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(a.reps):
        fn()
        ms.append(ctx.last_timings()[stage])
    return float(np.median(ms)), float(np.min(ms))


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def bench_nodes(case, d_ids, d_w, n, nsrc, note):
    rng = np.random.default_rng(1)
    create_ms = []
    op = None
    for _ in range(3):
        if op is not None:
            op.free()
        ctx.synchronize()
        t0 = time.perf_counter()
        op = ctx.transpose_nodes(d_ids, d_w, nsrc)
        create_ms.append((time.perf_counter() - t0) * 1e3)
    rec = {"case": case, "form": "nodes", "targets": n, "P": 8, "destinations": nsrc, "note": note,
           "create_ms_first": round(create_ms[0], 3), "create_ms": round(min(create_ms[1:]), 3),
           "handle_bytes": 12 * n * 8 + 4 * (nsrc + 1)}
    for ncomp in (1, 3):
        d_v = ctx.to_device(rng.normal(size=(n, ncomp)))
        d_f = ctx.to_device(rng.normal(size=(ncomp, nsrc)))
        d_out = ctx.empty((ncomp, nsrc), np.float64)
        t_med, t_min = timed(lambda: op.apply(d_v, out=d_out))
        f_med, _ = timed(lambda: ctx.gather(d_f, d_ids, d_w))
        counted = n * 8 * (12 + 8 * ncomp) + 8 * ncomp * nsrc
        rec[f"C{ncomp}"] = {"apply_ms": round(t_med, 4), "apply_ms_min": round(t_min, 4), "forward_gather_ms": round(f_med, 4),
                            "apply_over_forward": round(t_med / f_med, 2), "counted_bytes": counted,
                            "GBps": round(counted / t_med / 1e6, 1), "frac_of_8TBps": round(counted / t_med / 1e6 / 8000, 3)}
    emit(rec)
    return op


pa = ca = None
if {"metric", "cfg4_shard", "host_route"} & set(cases):
    pa, ca = synth.hex_mesh(a.n_src, seed=1)
    conn = synth.reorder_hex8(ca)
    nsrc = len(pa)

if "metric" in cases or "host_route" in cases:
    n = nsrc
    rng = np.random.default_rng(0)
    # operator rows as the locate stage produces them: target t sits in an element next to node t
    elem = np.minimum(np.arange(n, dtype=np.int64) * len(ca) // n, len(ca) - 1)
    ids = np.ascontiguousarray(conn[elem])
    d_ids, d_w = ctx.to_device(ids), ctx.to_device(rng.uniform(size=(n, 8)))
    if "metric" in cases:
        bench_nodes("metric", d_ids, d_w, n, nsrc, "targets in source-element order, uniform weights").free()
    if "host_route" in cases:
        # what a user does today: operator rows to the host, np.add.at there (single-threaded) -- on a SUBSAMPLE of the
        # first 1,000,000 targets of the metric operator, not the whole of it
        m = min(1_000_000, n)
        v = np.random.default_rng(2).normal(size=m)
        t0 = time.perf_counter()
        ids_h, w_h = d_ids.rows(0, m).numpy(), d_w.rows(0, m).numpy()
        t_down = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        out = np.zeros(nsrc)
        np.add.at(out, ids_h, w_h * v[:, None])
        t_add = (time.perf_counter() - t0) * 1e3
        op = ctx.transpose_nodes(d_ids.rows(0, m), d_w.rows(0, m), nsrc)
        d_v = ctx.to_device(v)
        same = bool(np.array_equal(op.apply(d_v).numpy()[0].view(np.uint64), out.view(np.uint64)))
        t_dev, _ = timed(lambda: op.apply(d_v))
        op.free()
        emit({"case": "host_route_subsample", "note": "SUBSAMPLE: the first 1,000,000 targets of the metric operator",
              "targets": m, "download_ms": round(t_down, 2), "np_add_at_ms": round(t_add, 2),
              "device_apply_ms": round(t_dev, 4), "bit_equal": same})
    d_ids = d_w = ids = None

if "cfg4_shard" in cases:
    n = 465 ** 3 // 8
    rng = np.random.default_rng(3)
    covered = len(ca) // 8          # a contiguous shard of the target mesh lies in an eighth of the source
    elem = np.minimum(np.arange(n, dtype=np.int64) * covered // n, covered - 1)
    d_ids, d_w = ctx.to_device(np.ascontiguousarray(conn[elem])), ctx.to_device(rng.uniform(size=(n, 8)))
    bench_nodes("cfg4_shard", d_ids, d_w, n, nsrc,
                "12.6 M targets inside the first eighth of the source elements: rows of ~64, seven eighths of the nodes unnamed").free()
    d_ids = d_w = None

if "cfg5_gll" in cases:
    src = synth.gll_mesh(a.gll_src, 4, seed=1)
    d_u, _ = ctx.unique_points(ctx.to_device(synth.gll_mesh(a.gll_tgt, 4, seed=7).reshape(-1, 3)))
    n, nelem, P = d_u.shape[0], src.shape[0], src.shape[1]
    d_src = ctx.to_device(src)
    _, d_elem, d_co, missing = ctx.interpolate_gll(4, d_src, d_u, ctx.zeros((1, nelem, P), np.float64), nelem_to_search=20,
                                                   want_operator=True)
    rng = np.random.default_rng(4)
    create_ms, op = [], None
    for _ in range(3):
        if op is not None:
            op.free()
        ctx.synchronize()
        t0 = time.perf_counter()
        op = ctx.transpose_elem(d_elem, d_co, nelem)
        create_ms.append((time.perf_counter() - t0) * 1e3)
    rec = {"case": "cfg5_gll", "form": "elem", "targets": n, "P": P, "destinations": nelem, "missing": missing,
           "create_ms_first": round(create_ms[0], 3), "create_ms": round(min(create_ms[1:]), 3),
           "handle_bytes": 4 * n + 4 * (nelem + 1)}
    for ncomp in (1, 3):
        d_v = ctx.to_device(rng.normal(size=(n, ncomp)))
        d_f = ctx.to_device(rng.normal(size=(ncomp, nelem, P)))
        d_out = ctx.empty((ncomp, nelem, P), np.float64)
        t_med, t_min = timed(lambda: op.apply(d_v, out=d_out))
        f_med, _ = timed(lambda: ctx.gather_elem(d_f, d_elem, d_co))
        counted = n * (8 * P + 4 + 8 * ncomp) + 8 * ncomp * nelem * P
        rec[f"C{ncomp}"] = {"apply_ms": round(t_med, 4), "apply_ms_min": round(t_min, 4), "forward_gather_elem_ms": round(f_med, 4),
                            "apply_over_forward": round(t_med / f_med, 2), "counted_bytes": counted,
                            "GBps": round(counted / t_med / 1e6, 1), "frac_of_8TBps": round(counted / t_med / 1e6 / 8000, 3)}
    emit(rec)
    op.free()

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    for rec in lines:
        fh.write(json.dumps(rec) + "\n")
