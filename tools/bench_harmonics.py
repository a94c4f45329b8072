"""mm_harmonic_model_apply on the 125 M nodes of a 1 M-element order-4 chunk of a spherical shell, timed with device events
after warm-up: lmax 20 and 40, 1 and 4 components, 21 knots, mode 0.  mm_radial_model_apply (mode 0, a table of 21 rows) is
timed on the same points in the same run as the streaming yardstick: it reads the same coordinates and writes the same
outputs, with a handful of operations per node.

Counted fp64 operations per node: (8 * ncomp + 5) per (l, k) term, (lmax + 1)(lmax + 2) / 2 terms.  Per term the Legendre
recurrence a * (ct * P1 - b * P2) is 4 operations and is counted as 5 with its share of the per-order work (P_kk, C_k, S_k,
the order's term), and each component adds a product and a sum for the cosine and the sine coefficient at both knot rows:
2 * 2 * 2 = 8.  Products and sums are separate instructions (no fused multiply-add), each counted as one.
Counted bytes per node (both kernels): 24 read + 8 written per component.
Writes profiles/harmonics_bench.json and prints it.  Usage: python tools/bench_harmonics.py [--reps N] [--side S] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import harmonics as H  # noqa: E402
from multimesh_amd import synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402

KNOTS = 21


def timed(fn, reps, warmup=2):
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
    return (8 * ncomp + 5) * ((lmax + 1) * (lmax + 2) // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--side", type=int, default=100, help="elements per side of the chunk (100: 1 M elements)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harmonics_bench.json"))
    args = ap.parse_args()
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    lib = H.bind(ctx.lib)
    dev = torch.device("cuda", 0)

    # ---- the chunk of tools/bench_radial.py: side^3 order-4 elements of a shell, [shell, lat, lon] with the shell slowest
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
    out = torch.empty((4, n), device=dev, dtype=torch.float64)
    knots = np.linspace(3.48e6, 6.3466e6, KNOTS)
    table = ctx.to_device(knots)
    rng = np.random.default_rng(0)
    results = []

    yardstick = {}
    for ncomp in (1, 4):
        vals = ctx.to_device(np.cos(np.arange(ncomp * KNOTS, dtype=np.float64)).reshape(ncomp, -1) + 4.0)
        check = []
        t = timed(lambda: check.append(lib.mm_radial_model_apply(ctx.handle, pts.data_ptr(), E, 125, table.ptr, vals.ptr, KNOTS,
                                                                 ncomp, 0, None, out.data_ptr())), args.reps)
        assert not any(check), check
        nbytes = n * (24 + 8 * ncomp)
        yardstick[ncomp] = t[0]
        results.append({"what": f"mm_radial_model_apply, mode 0, {ncomp} comp (the streaming yardstick)", "ncomp": ncomp,
                        "ms_median": round(t[0], 4), "ms_min": round(t[1], 4), "counted_bytes": nbytes,
                        "TBps": round(nbytes / t[0] / 1e9, 3)})

    count = torch.zeros(1, device=dev, dtype=torch.int64)
    for lmax in (20, 40):
        nlm = H.coefficient_count(lmax)
        for ncomp in (1, 4):
            coef = ctx.to_device(0.01 * rng.standard_normal((ncomp, KNOTS, 2, nlm)))
            check = []
            t = timed(lambda: check.append(lib.mm_harmonic_model_apply(ctx.handle, pts.data_ptr(), E, 125, table.ptr, KNOTS, lmax,
                                                                       coef.ptr, ncomp, 0, 0, None, out.data_ptr(),
                                                                       count.data_ptr())), args.reps)
            assert not any(check), check
            ops = n * operations_per_node(lmax, ncomp)
            nbytes = n * (24 + 8 * ncomp)
            results.append({"what": f"mm_harmonic_model_apply, lmax {lmax}, {ncomp} comp", "lmax": lmax, "ncomp": ncomp,
                            "ms_median": round(t[0], 3), "ms_min": round(t[1], 3),
                            "counted_fp64_operations": ops, "Tops_per_s": round(ops / t[0] / 1e9, 3),
                            "ns_per_node": round(t[0] * 1e6 / n, 4), "counted_bytes": nbytes,
                            "time_over_radial_model_apply": round(t[0] / yardstick[ncomp], 1)})
    torch.cuda.synchronize()
    outside = int(count.item())
    ctx.close()

    doc = {"what": "mm_harmonic_model_apply beside mm_radial_model_apply on the same points, device events, median of --reps "
                   "after warm-up; counted fp64 operations (8 * ncomp + 5) per (l, k) term and node",
           "elements": E, "nodes": n, "knots": KNOTS, "reps": args.reps, "nodes_outside_the_table_per_call": outside // max(
               1, 4 * (args.reps + 2)), "cases": results}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
