"""mm_gll_resolution and mm_arg_extreme on the 1 M-element order-4 chunk (125 M nodes, 3 GB of coordinates: HBM), timed with
device events after warm-up, beside mm_gll_mass on the same arrays in the same process (the yardstick: it reads the same
24 B per node and writes 8 B per node where the sizes-only call writes 24 B per element) and beside NumPy on every 50th
element, per node:

* sizes only;
* sizes with 2 fast and 2 slow components (24 + 32 B read per node);
* mm_arg_extreme over the 1 M values of the step row.

Writes profiles/resolution_bench.json (ms, counted bytes, TB/s, the ratio to the mass kernel, NumPy's ns per node) and
prints it.  Usage: python tools/bench_resolution.py [--reps N] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resolution_cases as RC  # noqa: E402
from multimesh_amd import synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402

ORDER, P = 4, 125


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


def chunk(dev, side=100):
    """side^3 elements: cells of a regular grid, every element's nodes placed by the tensor GLL points (right-handed)"""
    g = torch.from_numpy((synth.gll_nodes_1d(ORDER) + 1.0) / 2.0).to(dev)
    cell = torch.arange(side, device=dev, dtype=torch.float64)
    ax = ((cell[:, None] + g[None, :]) * 1.0e4 + 3.0e6)
    pts = torch.empty((side, side, side, 5, 5, 5, 3), device=dev, dtype=torch.float64)   # [ex, ey, ez, k, j, i, c]
    pts[..., 0] = ax[:, None, None, None, None, :]
    pts[..., 1] = ax[None, :, None, None, :, None]
    pts[..., 2] = ax[None, None, :, :, None, None]
    return pts.reshape(side ** 3, P, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--side", type=int, default=100, help="elements per side of the chunk (100: the 1 M-element case)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resolution_bench.json"))
    args = ap.parse_args()
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    pts = chunk(dev, args.side)
    E = pts.shape[0]
    n = E * P
    fast = torch.rand((2, E, P), generator=gen, device=dev, dtype=torch.float64) * 5.0e3 + 8.0e3
    slow = torch.rand((2, E, P), generator=gen, device=dev, dtype=torch.float64) * 3.0e3 + 4.0e3
    out = torch.empty((5, E), device=dev, dtype=torch.float64)
    info = torch.empty((2,), device=dev, dtype=torch.int64)
    rc = []

    def sizes():
        rc.append(lib.mm_gll_resolution(ctx.handle, ORDER, 3, pts.data_ptr(), E, None, 0, None, 0, None, out.data_ptr(),
                                        info.data_ptr()))

    def model():
        rc.append(lib.mm_gll_resolution(ctx.handle, ORDER, 3, pts.data_ptr(), E, fast.data_ptr(), 2, slow.data_ptr(), 2, None,
                                        out.data_ptr(), info.data_ptr()))

    value = torch.empty((1,), device=dev, dtype=torch.float64)
    index, nvalid = torch.empty((1,), device=dev, dtype=torch.int64), torch.empty((1,), device=dev, dtype=torch.int64)

    def extreme():
        rc.append(lib.mm_arg_extreme(ctx.handle, out[3].data_ptr(), 1, E, 0, value.data_ptr(), index.data_ptr(),
                                     nvalid.data_ptr()))

    deriv, weights = ctx.to_device(synth.gll_derivative_matrix(ORDER)), ctx.to_device(synth.gll_weights_1d(ORDER))
    mass = torch.empty((E, P), device=dev, dtype=torch.float64)

    def run_mass():
        rc.append(lib.mm_gll_mass(ctx.handle, ORDER, 3, pts.data_ptr(), E, deriv.ptr, weights.ptr, mass.data_ptr(), None))

    results = {}
    for name, fn, nbytes in (("mass", run_mass, n * 32), ("sizes", sizes, n * 24 + E * 24),
                             ("sizes_2fast_2slow", model, n * 56 + E * 40), ("mass_again", run_mass, n * 32),
                             ("arg_extreme_step_row", extreme, E * 8 * 2)):
        ms, ms_min = timed(fn, args.reps)
        results[name] = {"ms_median": round(ms, 4), "ms_min": round(ms_min, 4), "counted_bytes": nbytes,
                         "TBps": round(nbytes / ms / 1e9, 3)}
    assert all(r >= 0 for r in rc), rc
    # the results at this size against the statement, on every 50th element; and NumPy's own time there
    sel = slice(0, E, 50)
    gp_h, f_h, s_h = pts[sel].cpu().numpy(), fast[:, sel].cpu().numpy(), slow[:, sel].cpu().numpy()
    t0 = time.perf_counter()
    ref, ref_info, _ = RC.resolution(gp_h, ORDER, f_h, s_h)
    numpy_s = time.perf_counter() - t0
    same = RC.same_bits(out[:, sel].cpu().numpy(), ref)
    got_index, got_value = int(index.cpu()[0]), float(value.cpu()[0])
    step = out[3].cpu().numpy()
    torch.cuda.synchronize()
    ctx.close()
    doc = {"what": "mm_gll_resolution and mm_arg_extreme beside mm_gll_mass on the same order-4 chunk, device events, median "
                   "of --reps after warm-up; NumPy's statement on every 50th element",
           "elements": E, "nodes": n, "reps": args.reps, "cases": results,
           "sizes_over_mass_time": round(results["sizes"]["ms_median"] / results["mass"]["ms_median"], 3),
           "numpy_elements": int(gp_h.shape[0]), "numpy_ns_per_node": round(numpy_s * 1e9 / (gp_h.shape[0] * P), 2),
           "gpu_model_ns_per_node": round(results["sizes_2fast_2slow"]["ms_median"] * 1e6 / n, 5),
           "same_bits_as_numpy_on_the_sample": bool(same), "invalid": [int(v) for v in info.cpu()],
           "arg_extreme_matches_numpy": bool(got_index == int(np.argmin(step)) and got_value == float(step.min()))}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
