"""The grid import as an operator and its transpose (mm_grid_operator, mm_transpose_*, mm_gather), on the workload of
tools/bench_grid_import.py: the 125 M nodes of a 1 M-element order-4 Earth chunk against a 312 x 400 x 400 cube.

  (a) mm_grid_operator beside mm_sample_grid with one component, on the same resident points: both read 24 B per point, the
      operator writes 128 B per point where the sampler writes 8;
  (b) the transpose: mm_transpose_create_nodes once, then mm_transpose_apply with 1 and 4 components;
  (c) GridOperator.apply's device part (mm_gather through the kept operator) beside a fresh mm_sample_grid, 1 and 4 components.

Wall clock around whole calls (each ends in a stream synchronisation), median of --steps after --warmup.  Prints one JSON line
per case and writes them to --out.
Usage: python tools/bench_grid_adjoint.py [--steps N] [--warmup W] [--nel 100] [--out profiles/grid_adjoint_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402


def timed(fn, steps, warmup, sync):
    """Median and minimum wall-clock ms of fn() followed by a stream synchronisation (mm_gather and mm_transpose_apply do
    not synchronise themselves)"""
    for _ in range(warmup):
        fn()
    sync()
    ms = []
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nlat", type=int, default=400)
    ap.add_argument("--nlon", type=int, default=400)
    ap.add_argument("--ndepth", type=int, default=312)
    ap.add_argument("--nel", type=int, default=100, help="elements per side (lat, lon, radius): nel^3 elements")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_adjoint_bench.json"))
    args = ap.parse_args()
    lines = []

    def emit(record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    pts_h = synth.earth_chunk(4, nlat=args.nel, nlon=args.nel, lat=(-40.0, 40.0), lon=(-40.0, 40.0),
                              radii=(4_371_000.0, 5_371_000.0, 6_371_000.0),
                              nrad=(args.nel // 2, args.nel - args.nel // 2))["points"].reshape(-1, 3)
    n = len(pts_h)
    lat = np.linspace(-40.5, 40.5, args.nlat)
    lon = np.linspace(-40.5, 40.5, args.nlon)
    depth = np.linspace(-1_000.0, 2_001_000.0, args.ndepth)
    nsrc = args.ndepth * args.nlat * args.nlon
    rng = np.random.default_rng(0)
    full = (args.nel, args.ndepth, args.nlat, args.nlon) == (100, 312, 400, 400)
    base = {"workload": "full" if full else "reduced", "elements": args.nel ** 3, "order": 4, "points": n,
            "grid": [args.ndepth, args.nlat, args.nlon]}

    ctx = Context(0)
    pts = ctx.to_device(pts_h)
    del pts_h
    d_d, la_d, lo_d = ctx.to_device(depth), ctx.to_device(lat), ctx.to_device(lon)
    cube4 = ctx.to_device(rng.normal(size=(4, nsrc)))
    ids, w = ctx.empty((n, 8), np.int64), ctx.empty((n, 8), np.float64)
    out4 = ctx.empty((4, n), np.float64)
    res = {}

    # (a)
    def operator():
        res["outside"] = ctx.grid_operator(pts, d_d, la_d, lo_d, ids_out=ids, weights_out=w)[2]

    def sample(ncomp):
        return lambda: ctx.sample_grid(pts, cube4.rows(0, ncomp).reshape(ncomp, args.ndepth, args.nlat, args.nlon), d_d, la_d, lo_d,
                                       out=out4.rows(0, ncomp))

    ms_op, min_op = timed(operator, args.steps, args.warmup, ctx.synchronize)
    ms_s = {c: timed(sample(c), args.steps, args.warmup, ctx.synchronize) for c in (1, 4)}
    emit({"case": "a_grid_operator", "ms_median": round(ms_op, 3), "ms_min": round(min_op, 3), "counted_bytes_per_point": 152,
          "counted_TB_per_s": round(152 * n / ms_op / 1e9, 3), "noutside": res["outside"], **base})
    emit({"case": "a_sample_grid_1comp", "ms_median": round(ms_s[1][0], 3), "ms_min": round(ms_s[1][1], 3),
          "counted_bytes_per_point": 32, "counted_TB_per_s": round(32 * n / ms_s[1][0] / 1e9, 3), **base})
    emit({"case": "a_ratio_operator_over_sample_grid", "ratio": round(ms_op / ms_s[1][0], 3), **base})

    # (c) before the transpose takes its memory
    for ncomp in (1, 4):
        ms_g, min_g = timed(lambda: ctx.gather(cube4.rows(0, ncomp), ids, w, point_major=False).free(), args.steps, args.warmup, ctx.synchronize)
        emit({"case": "c_gather_through_operator", "ncomp": ncomp, "ms_median": round(ms_g, 3), "ms_min": round(min_g, 3),
              "fresh_sample_grid_ms": round(ms_s[ncomp][0], 3), "ratio_to_sample_grid": round(ms_g / ms_s[ncomp][0], 3), **base})

    # (b)
    t = time.perf_counter()
    op = ctx.transpose_nodes(ids, w, nsrc)
    ctx.synchronize()
    create_ms = (time.perf_counter() - t) * 1e3
    emit({"case": "b_transpose_create", "ms": round(create_ms, 3), "contributions": 8 * n, **base})
    back = ctx.empty((4, nsrc), np.float64)
    values = ctx.to_device(rng.normal(size=(4, n)))
    for ncomp in (1, 4):
        ms_t, min_t = timed(lambda: op.apply(values.rows(0, ncomp), point_major=False, out=back.rows(0, ncomp)), args.steps, args.warmup, ctx.synchronize)
        emit({"case": "b_transpose_apply", "ncomp": ncomp, "ms_median": round(ms_t, 3), "ms_min": round(min_t, 3), **base})
    op.free()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
