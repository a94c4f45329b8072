"""mm_harmonic_model_transpose on the 125 M nodes of a 1 M-element order-4 chunk of a spherical shell (the chunk of
tools/bench_harmonics.py), timed with device events after warm-up: lmax 20 and 40, 1 and 4 components, 21 knots, no weights,
the default scratch limit.  mm_harmonic_model_apply (mode 0) is timed with the same points, table, degree and number of
components in the same run: it is the yardstick, and the ratio of the two times is what this tool reports.

Counted fp64 operations per node of the transpose: (8 * ncomp + 5 * ceil(ncomp / 2)) per (l, k) term -- a product and a sum
for each of the four factors (cosine, sine) x (Lo, Hi) per component, and the Legendre recurrence (5, as counted for the
forward kernel) once per pass of two components.
Writes profiles/harmonic_adjoint_bench.json and prints it.
Usage: python tools/bench_harmonic_adjoint.py [--reps N] [--side S] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import harmonic_adjoint as A  # noqa: E402
from multimesh_amd import harmonics as H  # noqa: E402
from multimesh_amd import synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402

KNOTS = 21


def timed(fn, reps, warmup=1):
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


def operations_per_node(lmax, ncomp):
    return (8 * ncomp + 5 * ((ncomp + 1) // 2)) * ((lmax + 1) * (lmax + 2) // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--side", type=int, default=100, help="elements per side of the chunk (100: 1 M elements)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harmonic_adjoint_bench.json"))
    args = ap.parse_args()
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    lib = A.bind(H.bind(ctx.lib))
    dev = torch.device("cuda", 0)

    # ---- the chunk of tools/bench_harmonics.py: side^3 order-4 elements of a shell, [shell, lat, lon] with the shell slowest
    s = args.side
    g = torch.from_numpy((synth.gll_nodes_1d(4) + 1.0) / 2.0).to(dev)
    cell = torch.arange(s, device=dev, dtype=torch.float64)
    unit = (cell[:, None] + g[None, :]) / s
    rad = 3.5e6 + unit * (6.371e6 - 3.5e6)
    lat = torch.deg2rad(-20.0 + unit * 40.0)
    lon = torch.deg2rad(-20.0 + unit * 40.0)
    shape = (s, s, s, 5, 5, 5)
    R = rad[:, None, None, :, None, None].expand(shape)
    LA = lat[None, :, None, None, :, None].expand(shape)
    LO = lon[None, None, :, None, None, :].expand(shape)
    pts = torch.stack([R * torch.cos(LA) * torch.cos(LO), R * torch.cos(LA) * torch.sin(LO), R * torch.sin(LA)], dim=-1)
    pts = pts.reshape(s ** 3, 125, 3).contiguous()
    del R, LA, LO
    E, n = s ** 3, s ** 3 * 125
    values = torch.empty((4, n), device=dev, dtype=torch.float64)
    values.copy_(torch.cos(torch.arange(4 * n, device=dev, dtype=torch.float64)).reshape(4, n))
    table = ctx.to_device(np.linspace(3.48e6, 6.3466e6, KNOTS))
    rng = np.random.default_rng(0)
    count = torch.zeros(1, device=dev, dtype=torch.int64)
    results = []
    for lmax in (20, 40):
        nlm = H.coefficient_count(lmax)
        for ncomp in (1, 4):
            coef = ctx.to_device(0.01 * rng.standard_normal((ncomp, KNOTS, 2, nlm)))
            grad = ctx.empty((ncomp, KNOTS, 2, nlm), np.float64)
            check = []
            fwd = timed(lambda: check.append(lib.mm_harmonic_model_apply(ctx.handle, pts.data_ptr(), E, 125, table.ptr, KNOTS, lmax,
                                                                         coef.ptr, ncomp, 0, 0, None, values.data_ptr(),
                                                                         count.data_ptr())), args.reps)
            # (the forward call has just written `values`: the transpose reads a model's field, and every run the same one)
            adj = timed(lambda: check.append(lib.mm_harmonic_model_transpose(ctx.handle, pts.data_ptr(), E, 125, table.ptr, KNOTS,
                                                                             lmax, None, values.data_ptr(), ncomp, 0, grad.ptr,
                                                                             count.data_ptr(), 0)), args.reps)
            assert not any(check), check
            ops = n * operations_per_node(lmax, ncomp)
            results.append({"what": f"mm_harmonic_model_transpose, lmax {lmax}, {ncomp} comp", "lmax": lmax, "ncomp": ncomp,
                            "ms_median": round(adj[0], 3), "ms_min": round(adj[1], 3),
                            "forward_ms_median": round(fwd[0], 3), "forward_ms_min": round(fwd[1], 3),
                            "time_over_harmonic_model_apply": round(adj[0] / fwd[0], 2),
                            "counted_fp64_operations": ops, "Tops_per_s": round(ops / adj[0] / 1e9, 3),
                            "ns_per_node": round(adj[0] * 1e6 / n, 4)})
            print(json.dumps(results[-1]), flush=True)
    torch.cuda.synchronize()
    ctx.close()

    doc = {"what": "mm_harmonic_model_transpose beside mm_harmonic_model_apply (mode 0) on the same points, table, degree and "
                   "components in the same run; device events, median of --reps after warm-up; the default scratch limit",
           "elements": E, "nodes": n, "knots": KNOTS, "reps": args.reps, "cases": results}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
