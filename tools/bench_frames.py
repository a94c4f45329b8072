"""Rotations and the local basis on the element-nodal points of an order-4 Earth mesh (mm_rotate_points,
mm_rotate_vectors, mm_local_components), against the sphere map on the same points in the same run:

  (y) the yardstick: Context.map_to_sphere on the points, out of place (24 B read + 8 B radius + 24 B written per point);
  (a) frames.rotate_points out of place and in place, counted at 48 B per point;
  (b) frames.rotate_vectors_on_device on field planes [3][E][P], out of place, at 48 B per node;
  (c) frames.local_components_on_device on the same planes and the mesh's points, at 72 B per node;
  and for each the ratio of its byte rate to the yardstick's.

The mesh is synth.earth_chunk (order 4, ~1 M elements, 125 M nodes).  Everything is resident; each case is timed by the wall
clock around a call that ends in a stream synchronisation, median of --steps after --warmup.  The spread of a case is
(max - min) / median of its steps.  Prints one JSON line per case and writes them to --out.
Usage: python tools/bench_frames.py [--steps N] [--warmup W] [--nel 100] [--out profiles/frames_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import frames, synth  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    args = ap.parse_args()
    lines = []

    def emit(record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    t = time.perf_counter()
    chunk = synth.earth_chunk(4, nlat=args.nel, nlon=args.nel, lat=(-40.0, 40.0), lon=(-40.0, 40.0),
                              radii=(6_291_000.0, 6_341_000.0, 6_371_000.0), nrad=(args.nel // 2, args.nel - args.nel // 2))
    build_s = time.perf_counter() - t
    E, P = chunk["points"].shape[:2]
    n = E * P
    base = {"elements": E, "order": 4, "points": n}
    R = frames.Rotation.to_north_pole(35.0, -120.0).matrix

    ctx = Context(0)
    pts = ctx.to_device(chunk["points"])
    rad = ctx.to_device(chunk["z_node_1D"])
    other = ctx.empty((E, P, 3), np.float64)
    del chunk

    def run(case, fn, bytes_per_point, yardstick=None):
        def call():
            fn()
            ctx.synchronize()

        ms, lo, hi = timed(call, args.steps, args.warmup)
        rate = bytes_per_point * n / ms / 1e9
        record = {"case": case, "ms_median": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                  "spread": round((hi - lo) / ms, 4), "counted_bytes_per_point": bytes_per_point, "TB_per_s": round(rate, 3)}
        if yardstick is not None:
            record["rate_over_map_to_sphere"] = round(rate / yardstick, 4)
        emit({**record, **base})
        return rate

    yard = run("y_map_to_sphere_out_of_place", lambda: ctx.map_to_sphere(pts, rad, out=other), 56)
    run("a_rotate_points_out_of_place", lambda: frames.rotate_points(ctx, pts, R, out=other), 48, yard)
    # in place on the copy: there and back, so that the values stay at Earth scale however many steps run
    flip = [False]

    def in_place():
        frames.rotate_points(ctx, other, R, transpose=flip[0], out=other)
        flip[0] = not flip[0]

    run("a_rotate_points_in_place", in_place, 48, yard)
    fields = other.reshape(3, E, P)                  # three planes [E][P]: whatever the copy holds
    out = ctx.empty((3, E, P), np.float64)
    layout = lambda a: (a, P, E * P, (0, 1, 2))
    run("b_rotate_vectors_planes", lambda: frames.rotate_vectors_on_device(ctx, R, E, P, layout(fields), layout(out)), 48, yard)
    run("c_local_components_planes", lambda: frames.local_components_on_device(ctx, pts, E, P, layout(fields), layout(out)), 72, yard)
    run("y_map_to_sphere_again", lambda: ctx.map_to_sphere(pts, rad, out=other), 56, yard)
    emit({"summary": "frames", "mesh_build_s": round(build_s, 1), "steps": args.steps, "warmup": args.warmup, **base})
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
