"""The inside flag and the signed distance to a region's outline (mm_region_distance) on the nodes of an order-4 Earth mesh,
against two yardsticks on the same points in the same run:

  (a) regions.region_distance_call with the points, the edge table and the outputs resident on the device: a wiggly circle that
      covers about half the chunk laterally, with 64, 1 024 and 16 384 edges, cutoff 300 km, signed distance and flags both;
  (b) the yardsticks: Context.radial_bins (the coordinate stream) and Context.point_taper with 1 024 centres (a unit with the same
      per-element cull structure) on the same points;
  (c) the ratios (a) / (b) to both, and the ratio of the 16 384-edge time to the 1 024-edge time: near 16 means the culls do not
      work.

The mesh is synth.earth_chunk (order 4, ~1 M elements, 125 M nodes).  All are timed by the wall clock around whole calls that
end in a stream synchronisation, median of --steps after --warmup.  Building a Region is host work (NumPy: the edge table, the
anchor search over 24 candidates, anchor_inside) and is reported per case as region_build_host_s; it is not part of the times.
Prints one JSON line per case and writes them to --out.
Usage: python tools/bench_regions.py [--steps N] [--warmup W] [--nel 100] [--out profiles/regions_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import regions, synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402

R = 6371000.0


def timed(fn, steps, warmup):
    ms = []
    for step in range(warmup + steps):
        t = time.perf_counter()
        fn()
        if step >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def wiggly_circle(nedges, radius_deg=28.0, wiggle=0.15, lobes=9):
    phi = 2.0 * np.pi * np.arange(nedges) / nedges
    rad = radius_deg * (1.0 + wiggle * np.sin(lobes * phi))
    return np.stack([rad * np.sin(phi), rad * np.cos(phi)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nel", type=int, default=100, help="elements per side (lat, lon, radius): nel^3 elements")
    ap.add_argument("--cutoff-km", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.json"))
    args = ap.parse_args()
    lines = []

    def emit(record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    t = time.perf_counter()
    chunk = synth.earth_chunk(4, nlat=args.nel, nlon=args.nel, lat=(-40.0, 40.0), lon=(-40.0, 40.0),
                              radii=(6_291_000.0, 6_341_000.0, 6_371_000.0), nrad=(args.nel // 2, args.nel - args.nel // 2))
    gp = chunk["points"]
    build_s = time.perf_counter() - t
    nelem, P = gp.shape[:2]
    n = nelem * P
    base = {"elements": nelem, "order": 4, "points": n}
    unit_cutoff = 2.0 * np.sin(args.cutoff_km * 1e3 / (2.0 * R))

    ctx = Context(0)
    pts = ctx.to_device(gp)
    signed, flags = ctx.empty((nelem, P), np.float64), ctx.empty((nelem, P), np.int32)

    # ---- the yardsticks
    edges_r = np.linspace(6_291_000.0, 6_371_000.0, 33)

    def bins():
        ctx.radial_bins(pts, edges_r)[0].free()

    ms_b, min_b = timed(bins, args.steps, args.warmup)
    emit({"case": "b_radial_bins_same_points", "ms_median": round(ms_b, 3), "ms_min": round(min_b, 3), **base})
    rng = np.random.default_rng(0)
    centres = regions.unit_vectors(np.stack([rng.uniform(-40.0, 40.0, 1024), rng.uniform(-40.0, 40.0, 1024)], axis=1)) * R
    cd, ri, ro = ctx.to_device(centres), ctx.to_device(np.full(1024, 5.0e4)), ctx.to_device(np.full(1024, 3.0e5))

    def taper():
        ctx.point_taper(pts, cd, ri, ro, want_weight=True)[2].free()

    ms_t, min_t = timed(taper, args.steps, args.warmup)
    emit({"case": "b_point_taper_1024_centres", "ms_median": round(ms_t, 3), "ms_min": round(min_t, 3), **base})

    # ---- the regions
    ms_of = {}
    for nedges in (64, 1024, 16384):
        t = time.perf_counter()
        region = regions.Region(wiggly_circle(nedges))
        region_s = time.perf_counter() - t                       # host: the edge table, the anchor search, anchor_inside
        e, a = ctx.to_device(region.edges), ctx.to_device(region.anchor)
        got = {}

        def run():
            res, got["ninside"] = regions.region_distance_call(ctx, pts, e, a, region.anchor_inside, unit_cutoff, R, signed_out=signed,
                                                               inside_out=flags, want_info=True)
            got["info"] = res["info"].numpy().tolist()

        ms, mn = timed(run, args.steps, args.warmup)
        ms_of[nedges] = ms
        emit({"case": "a_region_distance", "edges": nedges, "cutoff_km": args.cutoff_km, "ms_median": round(ms, 3), "ms_min": round(mn, 3),
              "points_per_s": round(n / ms * 1e3), "ratio_to_radial_bins": round(ms / ms_b, 3), "ratio_to_point_taper": round(ms / ms_t, 3),
              "inside_fraction": round(got["ninside"] / n, 4), "hit_fraction": round(got["info"][0] / n, 4), "region_build_host_s": round(region_s, 3), **base})
        e.free(), a.free()
    emit({"summary": "regions", "ms_radial_bins": round(ms_b, 3), "ms_point_taper_1024": round(ms_t, 3),
          **{f"ms_{k}_edges": round(v, 3) for k, v in ms_of.items()},
          "ratio_16384_to_1024_edges": round(ms_of[16384] / ms_of[1024], 3), "mesh_build_s": round(build_s, 1), **base})
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
