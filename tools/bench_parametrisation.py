"""mm_convert_parameters and mm_convert_kernels on the 125 M nodes of 1 M order-4 elements, timed with device events after
warm-up, beside mm_clamp in place on 4 components of the same arrays in the same process (the streaming yardstick of
tools/bench_precondition.py: 16 bytes per value):

* vti_velocity -> iso_velocity: four steps, 6 components in and 3 out;
* iso_velocity -> vti_velocity: the copy, 3 in and 6 out;
* the kernel transform of the first: the model (6) and the kernels (3) in, 6 out;

each on field planes [C][E][P] and on MODEL/data-style rows [E][C][P].  Counted bytes per node: 8 * (C_in + C_out).  Writes
profiles/parametrisation_bench.json (ms, bytes, TB/s, and the ratio of each byte rate to the clamp's) and prints it.
Usage: python tools/bench_parametrisation.py [--reps N] [--elements E] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import parametrisation as P  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402

NODES_PER_ELEMENT = 125
VTI, ISO = "vti_velocity", "iso_velocity"


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


def layout(ctx, tensor, rows):
    """(DeviceArray, group_stride, comp_stride, cols) of a tensor [C, E, P] (planes) or [E, C, P] (rows)."""
    d = ctx.asdevice(tensor, np.float64)
    if rows:
        E, C, Pn = tensor.shape
        return (d, C * Pn, Pn, range(C))
    C, E, Pn = tensor.shape
    return (d, Pn, E * Pn, range(C))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--elements", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parametrisation_bench.json"))
    args = ap.parse_args()
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    E, Pn = args.elements, NODES_PER_ELEMENT
    n = E * Pn

    def rand(lo, hi):
        return torch.rand((E, Pn), generator=gen, device=dev, dtype=torch.float64) * (hi - lo) + lo

    vp, rho = rand(2000.0, 9000.0), rand(1000.0, 6000.0)
    vs = vp * rand(0.4, 0.6)
    vti = torch.stack([vp * rand(0.95, 1.05), vp * rand(0.95, 1.05), vs * rand(0.95, 1.05), vs * rand(0.95, 1.05),
                       rand(0.8, 1.1), rho])                                        # [6, E, P]
    iso = torch.stack([vp, vs, rho])
    kin = torch.randn((3, E, Pn), generator=gen, device=dev, dtype=torch.float64)
    del vp, vs, rho
    results = []
    for rows in (False, True):
        def arranged(t):
            return t.permute(1, 0, 2).contiguous() if rows else t

        m6, m3, k3 = arranged(vti), arranged(iso), arranged(kin)
        o3, o6 = torch.empty_like(m3), torch.empty_like(m6)
        name = "rows [E][C][P]" if rows else "planes [C][E][P]"
        nbad = ctx.zeros((1,), np.int64)
        runs = {
            "vti_velocity->iso_velocity": (9, lambda: P.convert_on_device(ctx, VTI, ISO, E, Pn, layout(ctx, m6, rows),
                                                                          layout(ctx, o3, rows), nbad=nbad)),
            "iso_velocity->vti_velocity": (9, lambda: P.convert_on_device(ctx, ISO, VTI, E, Pn, layout(ctx, m3, rows),
                                                                          layout(ctx, o6, rows), nbad=nbad)),
            "kernels vti_velocity->iso_velocity": (15, lambda: P.convert_on_device(
                ctx, VTI, ISO, E, Pn, layout(ctx, m6, rows), layout(ctx, o6, rows), kernels=layout(ctx, k3, rows), nbad=nbad)),
        }
        # the yardstick: mm_clamp in place on 4 components of the same array (its first 4 n values), bounds that clip nothing
        four = ctx.asdevice(m6, np.float64).reshape(6 * n).rows(0, 4 * n).reshape(4, n)
        upper = ctx.to_device(np.full(4, np.inf))
        c_ms, c_min = timed(lambda: ctx.clamp(four, upper=upper, out=four, want_count=False), args.reps)
        c_rate = 4 * n * 16 / c_ms / 1e9
        results.append({"layout": name, "case": "mm_clamp in place, 4 components", "ms_median": round(c_ms, 4),
                        "ms_min": round(c_min, 4), "counted_bytes": 4 * n * 16, "TBps": round(c_rate, 3)})
        for case, (words, fn) in runs.items():
            ms, ms_min = timed(fn, args.reps)
            rate = n * 8 * words / ms / 1e9
            results.append({"layout": name, "case": case, "ms_median": round(ms, 4), "ms_min": round(ms_min, 4),
                            "counted_bytes": n * 8 * words, "TBps": round(rate, 3), "rate_over_clamp": round(rate / c_rate, 3)})
        assert int(nbad.numpy()[0]) == 0
        del m6, m3, k3, o3, o6, four
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    ctx.close()
    doc = {"what": "mm_convert_parameters / mm_convert_kernels beside mm_clamp in place on the same arrays, device events, "
                   "median of --reps after warm-up", "elements": E, "nodes": n, "reps": args.reps, "cases": results}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
