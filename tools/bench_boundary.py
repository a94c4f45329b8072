"""Times the boundary entry points on a 1 M-element order-4 chunk, each beside an existing call of this library on the same
arrays in the same run, and writes profiles/boundary_bench.json.

  faces     mm_boundary_faces over the 8 M corner ids (after mm_unique_points_any_order, timed on its own), mm_boundary_classify
            and mm_boundary_nodes
  distance  mm_cutoff_distance of all 125 M nodes to the nodes of the side and bottom faces, cutoff = 1, 3 and 10 element
            widths; yardstick: mm_radial_bins over the same points, a pure coordinate stream
  knn       the middle cutoff through mm_knn_build + mm_knn_query(k = 1), the alternative that was not chosen, on every
            tenth element (the query's outputs for all nodes would be 2 GB); mm_cutoff_distance on the same subset beside it
  taper     mm_distance_taper in place on 4 components; yardstick: mm_clamp in place on the same values

    python tools/bench_boundary.py [--side 100] [--reps 5] [--out profiles/boundary_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_precondition import chunk, timed  # noqa: E402
from multimesh_amd.boundary import corner_nodes  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402


def write(result, path):
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_bench.json"))
    args = ap.parse_args()
    side, edge, ncomp, order = args.side, 10_000.0, 4, 4
    ctx = Context(0)
    pts_h = chunk(side, order=order, edge=edge)
    nelem, P = pts_h.shape[:2]
    n = nelem * P
    print(f"{nelem} elements, {n} nodes", flush=True)
    pts = ctx.to_device(pts_h)
    corners = ctx.to_device(pts_h[:, corner_nodes(order)])
    subset = ctx.to_device(pts_h[::10])
    del pts_h
    result = {"nelem": nelem, "order": order, "nodes": n, "ncomp": ncomp, "reps": args.reps, "distance": []}

    flat = corners.reshape(nelem * 8, 3)
    result["unique_corner_points_ms"] = timed(ctx, lambda: ctx.unique_points(flat, ordered=False), args.reps)
    uniq, inv = ctx.unique_points(flat, ordered=False)
    ids, nnodes = inv.reshape(nelem, 8), uniq.shape[0]
    result["boundary_faces_ms"] = timed(ctx, lambda: ctx.boundary_faces(ids, nnodes), args.reps)
    faces, nonmanifold = ctx.boundary_faces(ids, nnodes)
    result["boundary_classify_ms"] = timed(ctx, lambda: ctx.boundary_classify(corners, faces), args.reps)
    sides = ctx.boundary_classify(corners, faces)
    result["boundary_nodes_ms"] = timed(ctx, lambda: ctx.boundary_nodes(pts, order, faces, sides, 0b101), args.reps)
    nodes = ctx.boundary_nodes(pts, order, faces, sides, 0b101)
    result.update({"corner_classes": nnodes, "boundary_faces": faces.shape[0], "nonmanifold": nonmanifold,
                   "faces_per_side": np.bincount(sides.numpy(), minlength=3).tolist(), "boundary_nodes": nodes.shape[0]})
    print({k: v for k, v in result.items() if k != "distance"}, flush=True)

    edges = np.linspace(6_371_000.0 - 1.8 * side * edge, 6_371_000.0 + side * edge, 65)
    t_bins = timed(ctx, lambda: ctx.radial_bins(pts, edges), args.reps)
    result["yardstick_radial_bins_ms"] = t_bins
    for widths in (1, 3, 10):
        cutoff = widths * edge
        t = timed(ctx, lambda: ctx.cutoff_distance(pts, nodes, cutoff), args.reps)
        dist, nnear = ctx.cutoff_distance(pts, nodes, cutoff)
        result["distance"].append({"cutoff_element_widths": widths, "ms": t, "nodes_within_cutoff": nnear,
                                   "share_within_cutoff": nnear / n, "over_radial_bins": t / t_bins})
        print(result["distance"][-1], flush=True)
        if widths != 3:
            del dist
        else:
            dist3 = dist
    write(result, args.out)

    values = ctx.to_device(np.random.default_rng(0).normal(size=(ncomp, 1)) * np.ones((1, n)))
    bound = ctx.to_device(np.full(ncomp, 0.5))
    t_clamp = timed(ctx, lambda: ctx.clamp(values, upper=bound, symmetric=True, out=values), args.reps)
    t_taper = timed(ctx, lambda: ctx.distance_taper(dist3, 0.5 * edge, 3.0 * edge, values, out=values), args.reps)
    result["taper"] = {"in_place_4_components_ms": t_taper, "yardstick_clamp_in_place_ms": t_clamp, "over_clamp": t_taper / t_clamp}
    print(result["taper"], flush=True)
    del values, dist3
    write(result, args.out)

    cutoff = 3 * edge
    t_cut = timed(ctx, lambda: ctx.cutoff_distance(subset, nodes, cutoff), args.reps)
    t_build = timed(ctx, lambda: ctx.knn_build(nodes).free(), args.reps)
    index = ctx.knn_build(nodes)
    sub_flat = subset.reshape(subset.size // 3, 3)
    t_query = timed(ctx, lambda: index.query(sub_flat, 1, want_dist=True), max(1, args.reps // 2))
    result["knn"] = {"cutoff_element_widths": 3, "points": subset.size // 3, "cutoff_distance_ms": t_cut, "knn_build_ms": t_build,
                     "knn_query_k1_ms": t_query, "knn_over_cutoff_distance": (t_build + t_query) / t_cut}
    print(result["knn"], flush=True)
    write(result, args.out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
