"""mm_map_to_sphere (make_spherical's map, reference interpolator.py:1125-1144) at two sizes, timed with device
events after warm-up:

* node layout: the 216^3 hex8 mesh of the metric (10.1 M nodes, 10 M elements x 8), z_node_1D element-nodal and
  read at each node's first occurrence (mm_first_occurrence, timed on its own);
* element-nodal layout: 1 M order-4 elements, 125 M points (a Salvus mesh's MODEL/coordinates).

Counted bytes per point: 24 read + 8 of radius + 24 written = 56, plus 8 for the first-occurrence index in the node
layout.  Prints one JSON line per case.  Usage: python tools/bench_sphere.py [--reps N]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimesh_amd import synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402

PEAK_GBPS = 8000.0


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return float(np.median(ms)), float(np.min(ms))


def report(case, npoints, bytes_per_point, ms, ms_min, **extra):
    counted = npoints * bytes_per_point
    line = {"case": case, "points": npoints, "ms_median": round(ms, 4), "ms_min": round(ms_min, 4),
            "counted_bytes": counted, "GBps": round(counted / ms / 1e6, 1),
            "frac_of_8TBps": round(counted / ms / 1e6 / PEAK_GBPS, 3)}
    line.update(extra)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    ctx = Context(0, stream=stream.cuda_stream)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)

    # ---- node layout: 10 M nodes of the metric mesh, moved into the mantle
    pts_h, conn_h = synth.hex_mesh(216, seed=1)
    pts = torch.from_numpy(pts_h).to(dev) * 1.0e6 + torch.tensor([3.0e6, 1.0e6, 2.0e6], device=dev, dtype=torch.float64)
    conn = torch.from_numpy(conn_h).to(dev)
    del pts_h, conn_h
    z = torch.rand(conn.shape, generator=gen, device=dev, dtype=torch.float64) * 0.5 + 0.5
    out = torch.empty_like(pts)
    n = pts.shape[0]
    first = ctx.first_occurrence(conn, n)
    ms, ms_min = timed(lambda: ctx.first_occurrence(conn, n), args.reps)
    report("first_occurrence", conn.numel(), 8, ms, ms_min, nodes=n,
           note="counted: the connectivity read once (the node-side init / finish passes are not counted)")
    ms, ms_min = timed(lambda: ctx.map_to_sphere(pts, z, out=out, first=first), args.reps)
    report("map_node_layout", n, 64, ms, ms_min, note="24 read + 8 first index + 8 radius (gathered) + 24 written")
    del pts, conn, z, out, first
    torch.cuda.empty_cache()

    # ---- element-nodal layout: 1 M order-4 elements = 125 M points
    E, P = 1_000_000, 125
    pts = torch.rand((E, P, 3), generator=gen, device=dev, dtype=torch.float64) * 2.0e6 + 3.0e6
    z = torch.rand((E, P), generator=gen, device=dev, dtype=torch.float64) * 0.5 + 0.5
    out = torch.empty_like(pts)
    ms, ms_min = timed(lambda: ctx.map_to_sphere(pts, z, out=out), args.reps)
    report("map_element_nodal", E * P, 56, ms, ms_min, note="out of place: 24 read + 8 radius + 24 written")
    ms, ms_min = timed(lambda: ctx.map_to_sphere(pts, z, out=pts), args.reps)
    report("map_element_nodal_in_place", E * P, 56, ms, ms_min)
    torch.cuda.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
