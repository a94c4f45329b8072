"""A regular lat/lon/depth cube onto the nodes of an order-4 Earth mesh (mm_sample_grid), against the host path it replaces:

  (a) Context.sample_grid with the mesh's points resident on the device;
  (b) what a caller without (a) does: xyz -> lat/lon/depth in NumPy, scipy.interpolate.RegularGridInterpolator, and the
      upload of the values -- run on every 50th point and reported per point;
  (c) the ratio (a) / (b), per point.

The mesh is synth.earth_chunk (order 4, ~1 M elements, 125 M nodes), the cube 312 x 400 x 400 around it, 1 and 4
components.  (a) is timed by the wall clock around whole calls (each ends in a stream synchronisation), median of --steps
after --warmup; its bytes/s count 24 B read and 8 B written per component and point (the cube's corners are not counted).
Also recorded: the largest |lat_device - lat_numpy| and |lon_device - lon_numpy| in degrees over 10^6 random points.
Prints one JSON line per case and writes them to --out.
Usage: python tools/bench_grid_import.py [--steps N] [--warmup W] [--nel 100] [--out profiles/grid_import_bench.json]"""
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

R_EARTH = 6371000.0


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def host_latlondepth(p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = np.sqrt((x * x + y * y) + z * z)
    return 90.0 - np.rad2deg(np.arccos(z / r)), np.rad2deg(np.arctan2(y, x)), R_EARTH - r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nlat", type=int, default=400)
    ap.add_argument("--nlon", type=int, default=400)
    ap.add_argument("--ndepth", type=int, default=312)
    ap.add_argument("--nel", type=int, default=100, help="elements per side (lat, lon, radius): nel^3 elements")
    ap.add_argument("--subsample", type=int, default=50, help="the host path runs on every n-th point")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_import_bench.json"))
    args = ap.parse_args()
    lines = []

    def emit(record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    t = time.perf_counter()
    pts_h = synth.earth_chunk(4, nlat=args.nel, nlon=args.nel, lat=(-40.0, 40.0), lon=(-40.0, 40.0),
                              radii=(4_371_000.0, 5_371_000.0, 6_371_000.0),
                              nrad=(args.nel // 2, args.nel - args.nel // 2))["points"].reshape(-1, 3)
    build_s = time.perf_counter() - t
    n = len(pts_h)
    lat = np.linspace(-40.5, 40.5, args.nlat)
    lon = np.linspace(-40.5, 40.5, args.nlon)
    depth = np.linspace(-1_000.0, 2_001_000.0, args.ndepth)
    rng = np.random.default_rng(0)
    cube4 = rng.normal(size=(4, args.ndepth, args.nlat, args.nlon))
    base = {"elements": args.nel ** 3, "order": 4, "points": n, "grid": [args.ndepth, args.nlat, args.nlon]}

    ctx = Context(0)
    pts = ctx.to_device(pts_h)
    d_d, la_d, lo_d = ctx.to_device(depth), ctx.to_device(lat), ctx.to_device(lon)
    sub = np.ascontiguousarray(pts_h[::args.subsample])
    ratios = {}
    for ncomp in (1, 4):
        cube_h = np.ascontiguousarray(cube4[:ncomp])
        cube = ctx.to_device(cube_h)
        out = ctx.empty((ncomp, n), np.float64)
        res = {}

        def case_a():
            res["miss"] = ctx.sample_grid(pts, cube, d_d, la_d, lo_d, out=out)[1]

        ms_a, min_a = timed(case_a, args.steps, args.warmup)
        counted = (24 + 8 * ncomp) * n
        emit({"case": "a_sample_grid_resident_points", "ncomp": ncomp, "ms_median": round(ms_a, 3), "ms_min": round(min_a, 3),
              "points_per_s": round(n / ms_a * 1e3), "counted_bytes_per_point": 24 + 8 * ncomp,
              "counted_TB_per_s": round(counted / ms_a / 1e9, 3), "nmissing": res["miss"], **base})

        from scipy.interpolate import RegularGridInterpolator

        def case_b():
            la, lo, de = host_latlondepth(sub)
            at = np.stack([de, la, lo], axis=1)
            vals = np.stack([RegularGridInterpolator((depth, lat, lon), cube_h[c], bounds_error=False)(at)
                             for c in range(ncomp)])
            res["host"] = vals
            ctx.to_device(vals).free()

        ms_b, min_b = timed(case_b, max(1, min(args.steps, 2)), 0)
        per_point_a, per_point_b = ms_a / n, ms_b / len(sub)
        dev = out.numpy()[:, ::args.subsample]
        agree = float(np.nanmax(np.abs(dev - res["host"]))) if len(sub) else 0.0
        emit({"case": "b_host_scipy_plus_upload", "ncomp": ncomp, "points_timed": len(sub), "ms_median": round(ms_b, 2),
              "ns_per_point": round(per_point_b * 1e6, 2), "full_mesh_ms_extrapolated": round(per_point_b * n, 1),
              "max_abs_difference_to_a": agree, **base})
        ratios[ncomp] = per_point_a / per_point_b
        emit({"case": "c_ratio_a_over_b_per_point", "ncomp": ncomp, "ratio": round(ratios[ncomp], 6), **base})
        cube.free()
        out.free()

    v = rng.normal(size=(1_000_000, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    v *= rng.uniform(3.5e6, 6.4e6, size=(len(v), 1))
    lld = ctx.sample_grid(v, np.zeros((0, args.ndepth, args.nlat, args.nlon)), d_d, la_d, lo_d, want_latlondepth=True)[2].numpy()
    la, lo, de = host_latlondepth(v)
    emit({"case": "coordinates_device_vs_numpy", "points": len(v), "max_abs_lat_deg": float(np.abs(lld[:, 0] - la).max()),
          "max_abs_lon_deg": float(np.abs(lld[:, 1] - lo).max()), "depth_bit_equal": bool(np.array_equal(lld[:, 2], de))})
    emit({"summary": "grid import", "a_over_b_1comp": round(ratios[1], 6), "a_over_b_4comp": round(ratios[4], 6),
          "mesh_build_s": round(build_s, 1), **base})
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
