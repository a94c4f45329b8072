"""mm_gll_tensor_apply, timed with device events after warm-up, beside the search route it replaces.

On 1 M elements in 3-D (the mesh of tools/bench_gradient.py): 2 -> 4 and 4 -> 2 with 1 and 4 components in layout 0, each
with its counted bytes, 8 (P_in + P_out) per element and component, and the bytes/s they make.  Beside that, in the same
run, the search route on the same job: api.interpolate_gll_to_gll's device path -- Context.interpolate_gll of the order-2
model onto the order-4 nodes, the points already on the device -- and the ratio of the two times.  The yardsticks a
reading is held against are the project's own measured streaming kernels: mm_gll_mass (3.97 TB/s) and the sphere map
(4.97 TB/s).

Writes profiles/order_bench.json and prints it.  Usage: python tools/bench_order.py [--reps N] [--out PATH]"""
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

SIDE = 100                                                                            # elements per side: 1 M elements


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


def counted_bytes(nelem, ncomp, order_in, order_out, dim=3):
    return 8 * ((order_in + 1) ** dim + (order_out + 1) ** dim) * nelem * ncomp


def mesh_points(order, dev):
    """[E, P, 3] of SIDE^3 cubic elements of 10 km, away from the origin."""
    g = torch.from_numpy((synth.gll_nodes_1d(order) + 1.0) / 2.0).to(dev)
    m = order + 1
    cell = torch.arange(SIDE, device=dev, dtype=torch.float64)
    ax = ((cell[:, None] + g[None, :]) * 1.0e4 + 3.0e6)
    pts = torch.empty((SIDE, SIDE, SIDE, m, m, m, 3), device=dev, dtype=torch.float64)   # [ex, ey, ez, k, j, i, c]
    pts[..., 0] = ax[:, None, None, None, None, :]
    pts[..., 1] = ax[None, :, None, None, :, None]
    pts[..., 2] = ax[None, None, :, :, None, None]
    return pts.reshape(SIDE ** 3, m ** 3, 3)


def cases(ctx, reps):
    lib, dev = ctx.lib, torch.device("cuda", 0)
    E = SIDE ** 3
    gen = torch.Generator(device=dev).manual_seed(0)
    out = {"elements": E, "tensor_apply": []}
    up_ms = None
    for order_in, order_out in ((2, 4), (4, 2)):
        table = ctx.to_device(synth.gll_order_table(order_in, order_out))
        pin, pout = (order_in + 1) ** 3, (order_out + 1) ** 3
        for ncomp in (1, 4):
            u = torch.rand((ncomp, E, pin), generator=gen, device=dev, dtype=torch.float64)
            y = torch.empty((ncomp, E, pout), device=dev, dtype=torch.float64)

            def apply():
                rc = lib.mm_gll_tensor_apply(ctx.handle, 3, order_in, order_out, table.ptr, 0, u.data_ptr(), y.data_ptr(),
                                             E, ncomp, None, None)
                assert rc == 0, rc
            ms, ms_min = timed(apply, reps)
            nbytes = counted_bytes(E, ncomp, order_in, order_out)
            out["tensor_apply"].append({"order_in": order_in, "order_out": order_out, "ncomp": ncomp, "layout": 0,
                                        "ms_median": round(ms, 4), "ms_min": round(ms_min, 4), "counted_bytes": nbytes,
                                        "TBps": round(nbytes / ms / 1e9, 3)})
            if (order_in, order_out, ncomp) == (2, 4, 1):
                up_ms = ms
            del u, y
            torch.cuda.empty_cache()
    # the search route on the 2 -> 4 job, one component: every order-4 node located in the order-2 mesh
    src, tgt = mesh_points(2, dev), mesh_points(4, dev).reshape(-1, 3)
    field = torch.rand((1, E, 27), generator=gen, device=dev, dtype=torch.float64)
    vals = torch.empty((tgt.shape[0], 1), device=dev, dtype=torch.float64)
    missing = []

    def search():
        missing.append(ctx.interpolate_gll(2, src, tgt, field, out=vals)[1])
    ms, ms_min = timed(search, max(3, reps // 4), warmup=1)
    out["search_route"] = {"what": "Context.interpolate_gll, order-2 model onto the order-4 nodes, points on the device",
                           "targets": int(tgt.shape[0]), "ncomp": 1, "ms_median": round(ms, 3), "ms_min": round(ms_min, 3),
                           "targets_not_located": int(max(missing))}
    out["search_over_tensor_apply"] = round(ms / up_ms, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_bench.json"))
    args = ap.parse_args()
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    doc = {"what": "mm_gll_tensor_apply (3-D, layout 0) and the search route on the same 2 -> 4 job in one run: device "
                   "events, median of --reps after warm-up",
           "bytes_per_element_and_component": "8 (P_in + P_out)",
           "yardsticks_TBps": {"mm_gll_mass": 3.97, "sphere_map": 4.97},
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
