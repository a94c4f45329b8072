"""mm_gll_mass at two sizes, timed with device events after warm-up, beside mm_map_to_sphere on the same number of
points in the same process (the repository's measured streaming kernel, profiles/sphere_map_bench.json: the yardstick):

* gll_mesh(44, 4), cfg5's source: 79,507 order-4 elements, 9.9 M nodes (238 MB of coordinates: inside the Infinity Cache);
* 1 M order-4 elements, 125 M nodes (3 GB of coordinates: HBM).

Counted bytes per node: 24 read + 8 written = 32 for the mass; 24 + 8 + 24 = 56 for the sphere map.  Writes
profiles/mass_bench.json (ms, bytes, TB/s, and the ratio of the two byte rates) and prints it.
Usage: python tools/bench_mass.py [--reps N] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402

MASS_BYTES, SPHERE_BYTES = 32, 56


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


def case(ctx, lib, name, pts, z, reps):
    """pts f64[E, 125, 3] on the device.  The mass through the ABI on resident tables and outputs (no allocation and
    no table upload inside the timed window; the call's own synchronise and count readback are part of it)."""
    E, P, _ = pts.shape
    n = E * P
    deriv, weights = ctx.to_device(synth.gll_derivative_matrix(4)), ctx.to_device(synth.gll_weights_1d(4))
    mass = torch.empty((E, P), device=pts.device, dtype=torch.float64)
    bad = []

    def run_mass():
        bad.append(lib.mm_gll_mass(ctx.handle, 4, 3, pts.data_ptr(), E, deriv.ptr, weights.ptr, mass.data_ptr(), None))

    ms, ms_min = timed(run_mass, reps)
    assert all(b >= 0 for b in bad), bad
    out = torch.empty_like(pts)
    s_ms, s_min = timed(lambda: ctx.map_to_sphere(pts, z, out=out), reps)
    rate, s_rate = n * MASS_BYTES / ms / 1e9, n * SPHERE_BYTES / s_ms / 1e9
    return {"case": name, "elements": E, "nodes": n, "n_bad": int(bad[-1]),
            "mass_ms_median": round(ms, 4), "mass_ms_min": round(ms_min, 4), "mass_counted_bytes": n * MASS_BYTES,
            "mass_TBps": round(rate, 3),
            "sphere_ms_median": round(s_ms, 4), "sphere_ms_min": round(s_min, 4), "sphere_counted_bytes": n * SPHERE_BYTES,
            "sphere_TBps": round(s_rate, 3), "mass_over_sphere_rate": round(rate / s_rate, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mass_bench.json"))
    args = ap.parse_args()
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    results = []

    pts = torch.from_numpy(synth.gll_mesh(44, 4, seed=1)).to(dev)
    z = torch.rand(pts.shape[:2], generator=gen, device=dev, dtype=torch.float64) * 0.5 + 0.5
    results.append(case(ctx, ctx.lib, "gll_mesh(44, 4)", pts, z, args.reps))
    del pts, z
    torch.cuda.empty_cache()

    # 1 M elements: 100^3 cells of a regular grid, every element's nodes placed by the tensor GLL points (right-handed)
    g = torch.from_numpy((synth.gll_nodes_1d(4) + 1.0) / 2.0).to(dev)
    cell = torch.arange(100, device=dev, dtype=torch.float64)
    ax = ((cell[:, None] + g[None, :]) * 1.0e4 + 3.0e6)                            # [100, 5]: metres, away from the origin
    pts = torch.empty((100, 100, 100, 5, 5, 5, 3), device=dev, dtype=torch.float64)   # [ex, ey, ez, k, j, i, c]
    pts[..., 0] = ax[:, None, None, None, None, :]
    pts[..., 1] = ax[None, :, None, None, :, None]
    pts[..., 2] = ax[None, None, :, :, None, None]
    pts = pts.reshape(1_000_000, 125, 3)
    z = torch.rand(pts.shape[:2], generator=gen, device=dev, dtype=torch.float64) * 0.5 + 0.5
    results.append(case(ctx, ctx.lib, "1M order-4 elements", pts, z, args.reps))
    torch.cuda.synchronize()
    ctx.close()

    doc = {"what": "mm_gll_mass beside mm_map_to_sphere on the same points, device events, median of --reps after warm-up",
           "bytes_per_node": {"mass": MASS_BYTES, "sphere": SPHERE_BYTES}, "reps": args.reps, "cases": results}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
