"""Times the surface distance on bench_boundary.py's workload -- the 1 M-element order-4 chunk, 125 M nodes, its side and bottom
faces -- beside the node distance of the same faces in the same run, and writes profiles/surface_distance_bench.json.

  emit      mm_boundary_triangles of the side and bottom faces (mm_boundary_nodes beside it)
  distance  mm_surface_distance at cutoffs of 1, 3 and 10 element widths and unbounded, and mm_cutoff_distance to the same
            faces' nodes at 1, 3 and 10 widths; yardstick: mm_radial_bins over the same points, a pure coordinate stream

Every distance is first timed on every tenth element (12.5 M points).  It is timed on all nodes as well when ten times that
figure stays under --full-limit-ms; otherwise the entry says "all_nodes_ms": null and the subset figure stands.  The
unbounded case starts on every hundredth element and moves up to every tenth under the same rule (with --side 100 the elements
0, 100, ... all lie on the face x = 0: that figure only gates the next call and says nothing about the interior).  Best of --reps calls after
one warm-up call, host clock around the call and a stream synchronise (the calls read their count back, so they end drained).

    python tools/bench_surface_distance.py [--side 100] [--reps 3] [--full-limit-ms 4000] [--out profiles/surface_distance_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_boundary import write  # noqa: E402
from bench_precondition import chunk, timed  # noqa: E402
from multimesh_amd import surface  # noqa: E402
from multimesh_amd.boundary import Boundary, corner_nodes  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--full-limit-ms", type=float, default=4000.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_distance_bench.json"))
    args = ap.parse_args()
    side, edge, order = args.side, 10_000.0, 4
    ctx = Context(0)
    pts_h = chunk(side, order=order, edge=edge)
    nelem, P = pts_h.shape[:2]
    n = nelem * P
    print(f"{nelem} elements, {n} nodes", flush=True)
    pts = ctx.to_device(pts_h)
    corners = ctx.to_device(pts_h[:, corner_nodes(order)])
    tenth, hundredth = ctx.to_device(pts_h[::10]), ctx.to_device(pts_h[::100])
    del pts_h
    uniq, inv = ctx.unique_points(corners.reshape(nelem * 8, 3), ordered=False)
    faces, _ = ctx.boundary_faces(inv.reshape(nelem, 8), uniq.shape[0])
    sides = ctx.boundary_classify(corners, faces)
    bnd = Boundary(ctx, pts, order, faces, sides, 0)
    result = {"nelem": nelem, "order": order, "nodes": n, "reps": args.reps, "full_limit_ms": args.full_limit_ms,
              "subset_points": tenth.size // 3, "surface_distance": [], "node_distance": []}
    result["boundary_nodes_ms"] = timed(ctx, lambda: bnd._nodes(0b101), args.reps)
    result["boundary_triangles_ms"] = timed(ctx, lambda: surface._triangles(bnd, 0b101), args.reps)
    nodes, tri = bnd._nodes(0b101), surface._triangles(bnd, 0b101)
    result.update({"boundary_faces": faces.shape[0], "boundary_nodes": nodes.shape[0], "triangles": tri.shape[0]})
    edges = np.linspace(6_371_000.0 - 1.8 * side * edge, 6_371_000.0 + side * edge, 65)
    result["yardstick_radial_bins_ms"] = t_bins = timed(ctx, lambda: ctx.radial_bins(pts, edges), args.reps)
    print({k: v for k, v in result.items() if not isinstance(v, list)}, flush=True)

    def both(call):
        """(ms on every tenth element, ms on all nodes or None, the count of the last call)"""
        t_sub = timed(ctx, lambda: call(tenth), args.reps)
        t_all = timed(ctx, lambda: call(pts), args.reps) if 10.0 * t_sub <= args.full_limit_ms else None
        return t_sub, t_all

    for widths in (1, 3, 10):
        cutoff = widths * edge
        for name, call in (("surface_distance", lambda p: surface._distance(ctx, p, tri, cutoff)),
                           ("node_distance", lambda p: ctx.cutoff_distance(p, nodes, cutoff))):
            t_sub, t_all = both(call)
            result[name].append({"cutoff_element_widths": widths, "every_tenth_element_ms": t_sub, "all_nodes_ms": t_all,
                                 "all_nodes_over_radial_bins": None if t_all is None else t_all / t_bins})
            print(name, result[name][-1], flush=True)
        s, m = result["surface_distance"][-1], result["node_distance"][-1]
        s["over_node_distance_every_tenth"] = s["every_tenth_element_ms"] / m["every_tenth_element_ms"]
        s["over_node_distance_all_nodes"] = (s["all_nodes_ms"] / m["all_nodes_ms"]
                                             if s["all_nodes_ms"] is not None and m["all_nodes_ms"] is not None else None)
        write(result, args.out)

    t_100 = timed(ctx, lambda: surface._distance(ctx, hundredth, tri, np.inf), 1)
    t_10 = timed(ctx, lambda: surface._distance(ctx, tenth, tri, np.inf), 1) if 10.0 * t_100 <= 10.0 * args.full_limit_ms else None
    result["surface_distance"].append({"cutoff_element_widths": None, "every_hundredth_element_ms": t_100,
                                       "every_tenth_element_ms": t_10, "all_nodes_ms": None,
                                       "note": "unbounded; one call after one warm-up; not timed on all nodes"})
    print("surface_distance", result["surface_distance"][-1], flush=True)
    write(result, args.out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
