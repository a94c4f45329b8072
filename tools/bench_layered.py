"""A layered column model onto the nodes of an order-4 Earth mesh (mm_layered_model_apply), against the regular-grid import
on the same points in the same run:

  (a) layered.layered_model_apply with the mesh's points and the model's tables resident on the device: a global
      180 x 360 map (closed: 361 columns) with nb = 9 interfaces, lateral "bilinear" and "cell", pick "node", 1 and 4 components;
  (b) the yardstick: Context.sample_grid on the same points with a 9 x 180 x 361 cube and the same component count;
  (c) the ratio (a) / (b).

The mesh is synth.earth_chunk (order 4, ~1 M elements, 125 M nodes) over the uppermost 80 km.  Both are timed by the wall
clock around whole calls that end in a stream synchronisation, median of --steps after --warmup; the bytes/s count 24 B read
and 8 B written per component and node (the tables' columns and the cube's corners are not counted).
Prints one JSON line per case and writes them to --out.
Usage: python tools/bench_layered.py [--steps N] [--warmup W] [--nel 100] [--out profiles/layered_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import layered, synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nlat", type=int, default=180)
    ap.add_argument("--nlon", type=int, default=360)
    ap.add_argument("--nb", type=int, default=9)
    ap.add_argument("--nel", type=int, default=100, help="elements per side (lat, lon, radius): nel^3 elements")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layered_bench.json"))
    args = ap.parse_args()
    lines = []

    def emit(record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    t = time.perf_counter()
    pts_h = synth.earth_chunk(4, nlat=args.nel, nlon=args.nel, lat=(-40.0, 40.0), lon=(-40.0, 40.0),
                              radii=(6_291_000.0, 6_341_000.0, 6_371_000.0),
                              nrad=(args.nel // 2, args.nel - args.nel // 2))["points"].reshape(-1, 3)
    build_s = time.perf_counter() - t
    n = len(pts_h)
    nlayer = args.nb - 1
    rng = np.random.default_rng(0)
    lat = np.linspace(-90.0 + 90.0 / args.nlat, 90.0 - 90.0 / args.nlat, args.nlat)
    lon = -180.0 + 180.0 / args.nlon + 360.0 / args.nlon * np.arange(args.nlon)
    top = rng.uniform(-3000.0, 3000.0, (args.nlat, args.nlon))
    thickness = rng.uniform(2000.0, 14000.0, (nlayer, args.nlat, args.nlon))
    thickness[1, : args.nlat // 2] = 0.0                                   # a layer pinched out over half the map
    model = layered.LayeredModel.from_thickness(lat, lon, top, thickness,
                                                {f"p{c}": rng.uniform(2000.0, 8000.0, (nlayer,) + top.shape) for c in range(4)})
    assert model.periodic and model.appended
    depth = np.linspace(-3000.0, 80_000.0, args.nb)
    cube4 = rng.normal(size=(4, args.nb, args.nlat, args.nlon + 1))
    cube4[..., -1] = cube4[..., 0]
    base = {"elements": args.nel ** 3, "order": 4, "points": n, "map": [args.nlat, args.nlon + 1], "nb": args.nb}

    ctx = Context(0)
    pts = ctx.to_device(pts_h)
    la_d, lo_d, d_d = ctx.to_device(model.lat), ctx.to_device(model.lon), ctx.to_device(depth)
    ratios = {}
    for ncomp in (1, 4):
        names, bounds_h, values_h = model.packed(model.parameters[:ncomp])
        bounds, values = ctx.to_device(bounds_h), ctx.to_device(values_h)
        cube = ctx.to_device(np.ascontiguousarray(cube4[:ncomp]))
        out = ctx.empty((ncomp, n), np.float64)
        count = ctx.zeros((1,), np.int64)
        res = {}

        def sampler():
            res["miss"] = ctx.sample_grid(pts, cube, d_d, la_d, lo_d, lon_periodic=True, out=out)[1]

        ms_b, min_b = timed(sampler, args.steps, args.warmup)
        counted = (24 + 8 * ncomp) * n
        emit({"case": "b_sample_grid_same_points", "ncomp": ncomp, "ms_median": round(ms_b, 3), "ms_min": round(min_b, 3),
              "counted_bytes_per_point": 24 + 8 * ncomp, "counted_TB_per_s": round(counted / ms_b / 1e9, 3),
              "nmissing": res["miss"], **base})
        for lateral in ("bilinear", "cell"):
            def apply():
                layered.layered_model_apply(ctx, pts, la_d, lo_d, bounds, values, lon_periodic=True, lateral=lateral, out=out,
                                            noutside=count)
                ctx.synchronize()

            ms_a, min_a = timed(apply, args.steps, args.warmup)
            ratios[(lateral, ncomp)] = ms_a / ms_b
            emit({"case": "a_layered_model_apply", "lateral": lateral, "pick": "node", "ncomp": ncomp, "ms_median": round(ms_a, 3),
                  "ms_min": round(min_a, 3), "points_per_s": round(n / ms_a * 1e3), "counted_bytes_per_point": 24 + 8 * ncomp,
                  "counted_TB_per_s": round(counted / ms_a / 1e9, 3), "ratio_to_sample_grid": round(ms_a / ms_b, 4),
                  "noutside_per_call": int(count.numpy()[0]) // (args.steps + args.warmup), **base})
            count = ctx.zeros((1,), np.int64)
        for a in (bounds, values, cube, out):
            a.free()
    emit({"summary": "layered model", **{f"ratio_{lateral}_{ncomp}comp": round(r, 4) for (lateral, ncomp), r in ratios.items()},
          "mesh_build_s": round(build_s, 1), **base})
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
