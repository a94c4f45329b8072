"""mm_gll_gradient, timed with device events after warm-up, beside the two kernels it sits between.

One call on 1 M order-4 elements (125 M nodes, the mesh of tools/bench_mass.py and tools/bench_diffusion.py), all in one
run: mm_gll_mass (32 bytes per node), mm_gll_diffusion_apply isotropic at C = 1 and 3 (24 + 16 C), and mm_gll_gradient with
grad_d alone at C = 1 and 3 and with all four outputs at C = 1 -- each gradient timing with its counted bytes, 24 + 8 C
read plus 8 per written plane per node.  The gradient does a subset of the apply's arithmetic and LDS traffic and writes
24 B per node and component where the apply writes 8: the expectation is a time at or below the apply's at equal C.

Writes profiles/gradient_bench.json and prints it.  Usage: python tools/bench_gradient.py [--reps N] [--out PATH]"""
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

MASS_BYTES = 32


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


def row(ms, ms_min, nbytes, **what):
    return {**what, "ms_median": round(ms, 4), "ms_min": round(ms_min, 4), "counted_bytes": nbytes,
            "TBps": round(nbytes / ms / 1e9, 3)}


def cases(ctx, reps):
    lib, dev = ctx.lib, torch.device("cuda", 0)
    g = torch.from_numpy((synth.gll_nodes_1d(4) + 1.0) / 2.0).to(dev)
    cell = torch.arange(100, device=dev, dtype=torch.float64)
    ax = ((cell[:, None] + g[None, :]) * 1.0e4 + 3.0e6)                            # metres, away from the origin
    pts = torch.empty((100, 100, 100, 5, 5, 5, 3), device=dev, dtype=torch.float64)   # [ex, ey, ez, k, j, i, c]
    pts[..., 0] = ax[:, None, None, None, None, :]
    pts[..., 1] = ax[None, :, None, None, :, None]
    pts[..., 2] = ax[None, None, :, :, None, None]
    pts = pts.reshape(1_000_000, 125, 3)
    E, P, _ = pts.shape
    n = E * P
    deriv, weights = ctx.to_device(synth.gll_derivative_matrix(4)), ctx.to_device(synth.gll_weights_1d(4))
    mass = torch.empty((E, P), device=dev, dtype=torch.float64)
    ms, ms_min = timed(lambda: lib.mm_gll_mass(ctx.handle, 4, 3, pts.data_ptr(), E, deriv.ptr, weights.ptr,
                                               mass.data_ptr(), None), reps)
    out = {"elements": E, "nodes": n, "mass": row(ms, ms_min, n * MASS_BYTES), "apply": [], "gradient": []}
    del mass
    gen = torch.Generator(device=dev).manual_seed(0)
    for ncomp in (1, 3):
        u = torch.rand((ncomp, E, P), generator=gen, device=dev, dtype=torch.float64)
        y = torch.empty_like(u)

        def apply():
            rc = lib.mm_gll_diffusion_apply(ctx.handle, 4, 3, pts.data_ptr(), E, deriv.ptr, weights.ptr, u.data_ptr(),
                                            ncomp, 2.0, None, 0, 0.0, None, y.data_ptr())
            assert rc == 0, rc
        ms, ms_min = timed(apply, reps)
        out["apply"].append(row(ms, ms_min, n * (24 + 16 * ncomp), ncomp=ncomp, anisotropic=False))
        del y
        torch.cuda.empty_cache()
        grad = torch.empty((ncomp, 3, E, P), device=dev, dtype=torch.float64)
        for outputs in (("grad",), ("grad", "radial", "lateral", "norm")) if ncomp == 1 else (("grad",),):
            parts = [torch.empty_like(u) for _ in outputs[1:]]                      # radial, lateral, norm
            ptrs = [grad.data_ptr()] + [t.data_ptr() for t in parts] + [None] * (3 - len(parts))

            def gradient():
                rc = lib.mm_gll_gradient(ctx.handle, 4, 3, pts.data_ptr(), E, deriv.ptr, u.data_ptr(), ncomp, *ptrs)
                assert rc == 0, rc
            ms, ms_min = timed(gradient, reps)
            planes = ncomp * (3 + len(parts))
            out["gradient"].append(row(ms, ms_min, n * (24 + 8 * ncomp + 8 * planes), ncomp=ncomp, outputs=list(outputs),
                                       planes_written=planes))
            del parts
        del u, grad
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradient_bench.json"))
    args = ap.parse_args()
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    doc = {"what": "mm_gll_gradient beside mm_gll_mass and mm_gll_diffusion_apply (isotropic) in one run: device events, "
                   "median of --reps after warm-up",
           "bytes_per_node": {"mass": MASS_BYTES, "apply": "24 + 16 C", "gradient": "24 + 8 C + 8 per written plane"},
           "reps": args.reps}
    doc["one_million_elements"] = cases(ctx, args.reps)
    torch.cuda.synchronize()
    ctx.close()
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
