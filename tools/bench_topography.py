"""The radial stretching of the nodes of an order-4 Earth mesh by an interface map (mm_radial_stretch), against the sphere map
and the layered import on the same points in the same run:

  (a) topography.stretch_points with the mesh's points and the map resident on the device: a global 180 x 360 map (closed: 361
      columns) with 5 anchors; directions "apply" and "flatten", lateral "bilinear" and "cell", in place and out of place;
  (b) the yardsticks: Context.map_to_sphere (out of place) and layered.layered_model_apply (bilinear, pick "node", 1 component,
      a 9-interface model on the same map) on the same points;
  (c) the ratios (a) / (b) to both.

The mesh is synth.earth_chunk (order 4, ~1 M elements, 125 M nodes) over the uppermost 80 km.  In-place calls move the points;
so that every step sees the same kind of input, an in-place "apply" is followed by an untimed in-place "flatten" (and the
other way round), which brings the points back within rounding in bilinear mode; in cell mode the map is piecewise constant,
and a node within rounding of the border between two map nodes' cells may read the other column on the way back: the summary
reports how far each mode's round trips carried the points, and the mesh's own points are uploaded again after each.  All are timed by the wall clock around whole calls that end
in a stream synchronisation, median of --steps after --warmup; the bytes/s count 24 B read and 24 B written per node (the
map's columns are not counted).
Prints one JSON line per case and writes them to --out.
Usage: python tools/bench_topography.py [--steps N] [--warmup W] [--nel 100] [--out profiles/topography_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import layered, synth, topography  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402


def timed(fn, steps, warmup, after=None):
    ms = []
    for step in range(warmup + steps):
        t = time.perf_counter()
        fn()
        if step >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
        if after:
            after()
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nlat", type=int, default=180)
    ap.add_argument("--nlon", type=int, default=360)
    ap.add_argument("--na", type=int, default=5)
    ap.add_argument("--nel", type=int, default=100, help="elements per side (lat, lon, radius): nel^3 elements")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topography_bench.json"))
    args = ap.parse_args()
    lines = []

    def emit(record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    t = time.perf_counter()
    chunk = synth.earth_chunk(4, nlat=args.nel, nlon=args.nel, lat=(-40.0, 40.0), lon=(-40.0, 40.0),
                              radii=(6_291_000.0, 6_341_000.0, 6_371_000.0), nrad=(args.nel // 2, args.nel - args.nel // 2))
    pts_h, z_h = chunk["points"].reshape(-1, 3), chunk["z_node_1D"].reshape(-1)
    build_s = time.perf_counter() - t
    n = len(pts_h)
    rng = np.random.default_rng(0)
    lat = np.linspace(-90.0 + 90.0 / args.nlat, 90.0 - 90.0 / args.nlat, args.nlat)
    lon = -180.0 + 180.0 / args.nlon + 360.0 / args.nlon * np.arange(args.nlon)
    anchors = np.linspace(6_371_000.0, 6_271_000.0, args.na)                  # 25 km apart at na = 5: three lie in the mesh
    shifts = rng.uniform(-4000.0, 4000.0, (args.na,) + (args.nlat, args.nlon))
    shifts[-1] = 0.0
    imap = topography.InterfaceMap(lat, lon, anchors, shifts)
    assert imap.periodic and imap.appended
    nb = 9
    top = rng.uniform(-3000.0, 3000.0, (args.nlat, args.nlon))
    thickness = rng.uniform(2000.0, 14000.0, (nb - 1, args.nlat, args.nlon))
    thickness[1, : args.nlat // 2] = 0.0
    model = layered.LayeredModel.from_thickness(lat, lon, top, thickness, {"p0": rng.uniform(2000.0, 8000.0, (nb - 1,) + top.shape)})
    base = {"elements": args.nel ** 3, "order": 4, "points": n, "map": [args.nlat, args.nlon + 1], "na": args.na}

    ctx = Context(0)
    pts = ctx.to_device(pts_h)
    out = ctx.empty((n, 3), np.float64)
    resident = imap.on_device(ctx)
    count = ctx.zeros((1,), np.int64)

    # ---- the yardsticks
    z = ctx.to_device(z_h)

    def sphere():
        ctx.map_to_sphere(pts, z, out=out)
        ctx.synchronize()

    ms_s, min_s = timed(sphere, args.steps, args.warmup)
    emit({"case": "b_map_to_sphere_same_points", "ms_median": round(ms_s, 3), "ms_min": round(min_s, 3),
          "counted_bytes_per_point": 56, "counted_TB_per_s": round(56 * n / ms_s / 1e9, 3), **base})
    z.free()
    _, bounds_h, values_h = model.packed()
    la_d, lo_d, bounds, values = (ctx.to_device(a) for a in (model.lat, model.lon, bounds_h, values_h))
    field = ctx.empty((1, n), np.float64)

    def layers():
        layered.layered_model_apply(ctx, pts, la_d, lo_d, bounds, values, lon_periodic=True, lateral="bilinear", out=field,
                                    noutside=count)
        ctx.synchronize()

    ms_l, min_l = timed(layers, args.steps, args.warmup)
    emit({"case": "b_layered_model_apply_bilinear_1comp", "nb": nb, "ms_median": round(ms_l, 3), "ms_min": round(min_l, 3),
          "counted_bytes_per_point": 32, "counted_TB_per_s": round(32 * n / ms_l / 1e9, 3), **base})
    for a in (bounds, values, field):
        a.free()

    # ---- the stretching
    ratios, drift = {}, {}
    other = {"apply": "flatten", "flatten": "apply"}
    for direction in ("apply", "flatten"):
        for lateral in ("bilinear", "cell"):
            for in_place in (False, True):
                count = ctx.zeros((1,), np.int64)

                def stretch(direction=direction):
                    topography.stretch_points(ctx, pts, resident, direction=direction, lateral=lateral,
                                              out=pts if in_place else out, noutside=count)
                    ctx.synchronize()

                def undo():
                    topography.stretch_points(ctx, pts, resident, direction=other[direction], lateral=lateral, out=pts)
                    ctx.synchronize()

                ms, mn = timed(stretch, args.steps, args.warmup, after=undo if in_place else None)
                key = f"{direction}_{lateral}_{'in_place' if in_place else 'out_of_place'}"
                ratios[key] = (ms / ms_s, ms / ms_l)
                emit({"case": "a_radial_stretch", "direction": direction, "lateral": lateral, "in_place": in_place,
                      "ms_median": round(ms, 3), "ms_min": round(mn, 3), "points_per_s": round(n / ms * 1e3),
                      "counted_bytes_per_point": 48, "counted_TB_per_s": round(48 * n / ms / 1e9, 3),
                      "ratio_to_map_to_sphere": round(ms / ms_s, 4), "ratio_to_layered_1comp": round(ms / ms_l, 4),
                      "noutside_per_call": int(count.numpy()[0]) // (args.steps + args.warmup), **base})
                if in_place:      # how far the round trips carried the points, then the mesh's own points again
                    drift[f"{direction}_{lateral}"] = float(np.abs(pts.numpy() - pts_h).max())
                    pts.free()
                    pts = ctx.to_device(pts_h)
    emit({"summary": "topography", "ms_map_to_sphere": round(ms_s, 3), "ms_layered_1comp": round(ms_l, 3),
          **{f"ratio_to_sphere_{k}": round(v[0], 4) for k, v in ratios.items()},
          **{f"ratio_to_layered_{k}": round(v[1], 4) for k, v in ratios.items()},
          **{f"drift_m_after_round_trips_{k}": v for k, v in drift.items()}, "mesh_build_s": round(build_s, 1), **base})
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
