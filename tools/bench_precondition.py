"""Times mm_point_taper, mm_order_statistics and mm_clamp on a 1 M-element order-4 chunk with 4 components, each beside an
existing call of this library on the same arrays in the same run, and writes profiles/precondition_bench.json.

  taper   0, 100 and 5000 centres under a patch of the surface (well under 1 % of the elements are hit; the share is
          recorded); yardstick: mm_radial_bins over the same points, a pure coordinate stream
  select  m = 1 and m = 4 on smooth and on all-equal data; yardstick: one mm_weighted_sum pass over the same values times
          the eight passes the select makes

    python tools/bench_precondition.py [--side 100] [--reps 5] [--out profiles/precondition_bench.json]
"""
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

PASSES = 8


def chunk(side, order=4, edge=10_000.0):
    """f64[side^3, (order+1)^3, 3]: a regular block of elements under the surface z = 6371 km, node p = i + m j + m^2 k"""
    g = (synth.gll_nodes_1d(order) + 1.0) * 0.5 * edge
    m = order + 1
    pts = np.empty((side, side, side, m, m, m, 3))
    e = np.arange(side) * edge
    pts[..., 0] = (e[None, None, :, None, None, None] + g[None, None, None, None, None, :]) - 0.5 * side * edge
    pts[..., 1] = (e[None, :, None, None, None, None] + g[None, None, None, None, :, None]) - 0.5 * side * edge
    pts[..., 2] = (e[:, None, None, None, None, None] + g[None, None, None, :, None, None]) + (6_371_000.0 - side * edge)
    return pts.reshape(side ** 3, m ** 3, 3)


def timed(ctx, fn, reps):
    fn()
    ctx.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precondition_bench.json"))
    args = ap.parse_args()
    side, edge, ncomp = args.side, 10_000.0, 4
    rng = np.random.default_rng(0)
    ctx = Context(0)
    pts_h = chunk(side, edge=edge)
    nelem, P = pts_h.shape[:2]
    n = nelem * P
    print(f"{nelem} elements, {n} nodes", flush=True)
    pts = ctx.to_device(pts_h)
    x = pts_h[..., 0].reshape(-1) / (side * edge)
    z = (pts_h[..., 2].reshape(-1) - 6_371_000.0) / (side * edge)
    del pts_h
    smooth = np.stack([np.sin((3.0 + c) * x) * np.exp(2.0 * z) * (1.0 + c) for c in range(ncomp)])
    values = ctx.to_device(smooth)
    del smooth, x, z
    equal = ctx.to_device(np.full((ncomp, n), 2.5))
    print("arrays are on the device", flush=True)
    result = {"nelem": nelem, "order": 4, "nodes": n, "ncomp": ncomp, "reps": args.reps, "taper": [], "select": [], "clamp": {}}

    edges = np.linspace(6_371_000.0 - 1.8 * side * edge, 6_371_000.0 + side * edge, 65)
    t_bins = timed(ctx, lambda: ctx.radial_bins(pts, edges), args.reps)
    result["yardstick_radial_bins_ms"] = t_bins
    patch = 0.3 * side * edge
    for K in (0, 100, 5000):
        c = np.stack([rng.uniform(-0.5 * patch, 0.5 * patch, K), rng.uniform(-0.5 * patch, 0.5 * patch, K),
                      6_371_000.0 - rng.uniform(0.0, 2.0 * edge, K)], axis=1).reshape(K, 3)
        ri, ro = np.full(K, 0.2 * edge), np.full(K, 0.6 * edge)
        cd, rid, rod = ctx.to_device(c), ctx.to_device(ri), ctx.to_device(ro)
        t_w = timed(ctx, lambda: ctx.point_taper(pts, cd, rid, rod, want_weight=True), args.reps)
        t_in = timed(ctx, lambda: ctx.point_taper(pts, cd, rid, rod, values_in=values, out=values), args.reps)
        _, ncut, w = ctx.point_taper(pts, cd, rid, rod, want_weight=True)
        hit = int((w.numpy().min(axis=1) < 1.0).sum())
        del w
        result["taper"].append({"K": K, "weights_only_ms": t_w, "in_place_4_components_ms": t_in, "ncut_nodes": ncut,
                                "elements_cut": hit, "elements_cut_share": hit / nelem,
                                "weights_only_over_radial_bins": t_w / t_bins, "in_place_over_radial_bins": t_in / t_bins})
        print(result["taper"][-1], flush=True)

    flat = [values.rows(c, c + 1).reshape(n) for c in range(ncomp)]
    t_sum = timed(ctx, lambda: [ctx.weighted_sum(f) for f in flat], args.reps)
    result["yardstick_weighted_sum_pass_ms"] = t_sum
    for name, data in (("smooth", values), ("all_equal", equal)):
        for m in (1, 4):
            q = ctx.to_device(np.array([0.999, 0.5, 0.99, 0.9][:m]))
            t = timed(ctx, lambda: ctx.order_statistics(data, q, absolute=True, method="higher"), args.reps)
            result["select"].append({"data": name, "m": m, "ms": t, "passes": PASSES,
                                     "over_passes_times_weighted_sum": t / (PASSES * t_sum)})
            print(result["select"][-1], flush=True)
    bound = ctx.order_statistics(values, [0.999], absolute=True, method="higher")[0].reshape(ncomp)
    t = timed(ctx, lambda: ctx.clamp(values, upper=bound, symmetric=True, out=values), args.reps)
    result["clamp"] = {"in_place_4_components_ms": t, "over_weighted_sum_pass": t / t_sum}
    print(result["clamp"], flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
