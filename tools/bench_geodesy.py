"""The geographic view on the element-nodal points of an order-4 elliptical Earth mesh (mm_geographic_points), against the
sphere map and the rotation on the same points in the same run:

  (y) the yardsticks: Context.map_to_sphere out of place (24 B read + 8 B radius + 24 B written per point) and
      frames.rotate_points out of place (48 B per point) -- two kernels of the same launch shape that are HBM-bound;
  (a) direction 0 out of place and in place, counted at 48 B per point;
  (b) direction 0 out of place with radius_d and height_out_d, at 64 B per point;
  (c) direction 1 out of place and in place, at 48 B per point;
  and for each the ratio of its time to each yardstick's, and of its byte rate to theirs.

A ratio of times near the ratio of counted bytes says the kernel streams at the yardstick's rate: HBM-bound.  A larger one
is what the 10 quotients and 6 square roots of direction 0 (5 and 3 of direction 1) cost beyond the traffic.

The mesh is synth.earth_chunk (order 4, ~1 M elements, 125 M nodes, ellipticity of WGS84).  Everything is resident; each
case is timed by the wall clock around a call that ends in a stream synchronisation, median of --steps after --warmup.  The
spread of a case is (max - min) / median of its steps.  Prints one JSON line per case and writes them to --out.
Usage: python tools/bench_geodesy.py [--steps N] [--warmup W] [--nel 100] [--out profiles/geodesy_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import frames, geodesy, synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nel", type=int, default=100, help="elements per side (lat, lon, radius): nel^3 elements")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesy_bench.json"))
    args = ap.parse_args()
    lines = []

    def emit(record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    t = time.perf_counter()
    chunk = synth.earth_chunk(4, nlat=args.nel, nlon=args.nel, lat=(-40.0, 40.0), lon=(-40.0, 40.0),
                              radii=(6_291_000.0, 6_341_000.0, 6_371_000.0), nrad=(args.nel // 2, args.nel - args.nel // 2),
                              ellipticity=geodesy.WGS84_F)
    build_s = time.perf_counter() - t
    E, P = chunk["points"].shape[:2]
    n = E * P
    base = {"elements": E, "order": 4, "points": n}
    R = frames.Rotation.to_north_pole(35.0, -120.0).matrix
    ell = geodesy.Ellipsoid.from_mean_radius().constants()

    ctx = Context(0)
    pts = ctx.to_device(chunk["points"])
    rad = ctx.to_device(chunk["z_node_1D"])
    other = ctx.empty((E, P, 3), np.float64)
    radius = ctx.to_device(chunk["z_node_1D"] * 6371000.0)
    heights = ctx.empty((E, P), np.float64)
    del chunk
    yard = {}

    def run(case, fn, bytes_per_point):
        def call():
            fn()
            ctx.synchronize()

        ms, lo, hi = timed(call, args.steps, args.warmup)
        rate = bytes_per_point * n / ms / 1e9
        record = {"case": case, "ms_median": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                  "spread": round((hi - lo) / ms, 4), "counted_bytes_per_point": bytes_per_point, "TB_per_s": round(rate, 3)}
        for name, (yms, yrate) in yard.items():
            record[f"time_over_{name}"] = round(ms / yms, 4)
            record[f"rate_over_{name}"] = round(rate / yrate, 4)
        emit({**record, **base})
        return ms, rate

    first = run("y_map_to_sphere_out_of_place", lambda: ctx.map_to_sphere(pts, rad, out=other), 56)
    second = run("y_rotate_points_out_of_place", lambda: frames.rotate_points(ctx, pts, R, out=other), 48)
    yard["map_to_sphere"], yard["rotate_points"] = first, second
    go = geodesy.geographic_points_on_device
    ms_0, _ = run("a_to_geographic_out_of_place", lambda: go(ctx, pts, ell, out=other), 48)
    # in place on the copy, again and again: every step moves a point by the 20 km between the two latitudes at the most, so
    # the values stay at Earth scale over the steps of a run (the kernel has no branch that depends on them)
    run("a_to_geographic_in_place", lambda: go(ctx, other, ell, out=other), 48)
    ms_0r, _ = run("b_to_geographic_radius_and_height", lambda: go(ctx, pts, ell, out=other, radius=radius, height_out=heights), 64)
    pseudo = ctx.empty((E, P, 3), np.float64)
    go(ctx, pts, ell, out=pseudo)
    ms_1, _ = run("c_from_geographic_out_of_place", lambda: go(ctx, pseudo, ell, geodesy.TO_CARTESIAN, out=other), 48)
    run("c_from_geographic_in_place", lambda: go(ctx, other, ell, geodesy.TO_CARTESIAN, out=other), 48)
    again, _ = run("y_rotate_points_again", lambda: frames.rotate_points(ctx, pts, R, out=other), 48)
    emit({"summary": "geodesy", "ms_map_to_sphere": round(first[0], 4), "ms_rotate_points": round(second[0], 4),
          "ms_rotate_points_again": round(again, 4), "ms_to_geographic": round(ms_0, 4),
          "ms_to_geographic_radius_height": round(ms_0r, 4), "ms_from_geographic": round(ms_1, 4),
          "to_geographic_over_rotate_points": round(ms_0 / second[0], 3), "from_geographic_over_rotate_points": round(ms_1 / second[0], 3),
          "mesh_build_s": round(build_s, 1), "steps": args.steps, "warmup": args.warmup, **base})
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
