"""The scattered import on the 125 M nodes of a 1 M-element order-4 chunk against a 10 M-point cloud, k = 8 and 20, C = 1
and 4.  Three things, in runs that alternate (a) and (b):

* (a) mm_idw_gather alone, on the rows of one mm_knn_query;
* (b) the yardstick: mm_gather with P = k on the same idx and with dist as weights -- the same 16 k + C (8 k + 8) bytes per
  target, the rows read by 8 lanes per target in contiguous pieces;
* (c) the whole interpolate_scattered (host points in, host values out, chunked) beside mm_knn_query alone.

On every 50th point the host baseline runs too: scipy.spatial.cKDTree plus the NumPy statement (tests/scattered_cases.py),
in points per second, and the sample's bits are compared with the device's.

Device events on the null stream; every run is recorded, with the median and the run-to-run spread (max - min over the
median) of (a), (b) and their ratio.  Writes profiles/scattered_bench.json and prints it.
Usage: python tools/bench_scattered.py [--side N] [--cloud N] [--runs N] [--out PATH]"""
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
import scattered_cases as SC  # noqa: E402
from multimesh_amd import scattered, synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402

ORDER, P = 4, 125


def chunk(dev, side):
    """side^3 order-4 elements on a regular grid of unit cells: f64[side^3 * 125, 3]"""
    g = torch.from_numpy((synth.gll_nodes_1d(ORDER) + 1.0) / 2.0).to(dev)
    ax = torch.arange(side, device=dev, dtype=torch.float64)[:, None] + g[None, :]
    pts = torch.empty((side, side, side, 5, 5, 5, 3), device=dev, dtype=torch.float64)
    pts[..., 0] = ax[:, None, None, None, None, :]
    pts[..., 1] = ax[None, :, None, None, :, None]
    pts[..., 2] = ax[None, None, :, :, None, None]
    return pts.reshape(side ** 3 * P, 3)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    med = float(np.median(ms))
    return {"runs_ms": [round(float(m), 4) for m in ms], "median_ms": round(med, 4),
            "spread": round(float((max(ms) - min(ms)) / med), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100, help="elements per side of the chunk (100: 1 M elements, 125 M nodes)")
    ap.add_argument("--cloud", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scattered_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    src = rng.random((args.cloud, 3)) * args.side
    vals = rng.standard_normal((4, args.cloud))
    result = {"elements": args.side ** 3, "nodes": args.side ** 3 * P, "cloud": args.cloud, "runs": args.runs, "cases": []}
    with Context(0) as ctx:
        tgt = chunk(dev, args.side)
        n = tgt.shape[0]
        cloud = scattered.PointCloud(src, vals.T, ["A", "B", "C", "D"])
        index = cloud.index(ctx)
        fields = ctx.to_device(vals)
        sample = np.arange(0, n, 50)
        tgt_sample = tgt[torch.from_numpy(sample).to(dev)].cpu().numpy()
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        tree = cKDTree(src)
        tree_s = time.perf_counter() - t0
        for k in (8, 20):
            query_ms = [event_ms(lambda: index.query(tgt, k, want_dist=True)) for _ in range(args.runs + 1)][1:]
            idx, dist = index.query(tgt, k, want_dist=True)
            t0 = time.perf_counter()
            hd, hi = tree.query(tgt_sample, k)
            host_query_s = time.perf_counter() - t0
            for ncomp in (1, 4):
                f = fields.rows(0, ncomp)
                out_a, out_b = ctx.empty((ncomp, n), np.float64), ctx.empty((ncomp, n), np.float64)

                def run_a():
                    ctx.lib.mm_idw_gather(ctx.handle, f.ptr, args.cloud, ncomp, idx.ptr, dist.ptr, n, k, 2, np.inf, 0, 0.0,
                                          out_a.ptr, 0, None, None)

                def run_b():
                    ctx.lib.mm_gather(ctx.handle, f.ptr, args.cloud, ncomp, idx.ptr, dist.ptr, n, k, out_b.ptr, 0)

                run_a(), run_b()
                a_ms, b_ms = [], []
                for _ in range(args.runs):
                    a_ms.append(event_ms(run_a))
                    b_ms.append(event_ms(run_b))
                # (c) the public call: host points in, host values out
                tgt_h = tgt.cpu().numpy()
                t0 = time.perf_counter()
                got, nout = scattered.interpolate_scattered(cloud, tgt_h, ["A", "B", "C", "D"][:ncomp], k=k, context=ctx)
                whole_s = time.perf_counter() - t0
                # the host baseline on the sample, and its bits against the device's
                t0 = time.perf_counter()
                ref = SC.idw(vals[:ncomp], hi, hd, args.cloud, power=2)[0]
                host_s = host_query_s + time.perf_counter() - t0
                si, sd = index.query(tgt_sample, k, want_dist=True)       # (a target's row depends on the target alone)
                dev_sample = SC.idw(vals[:ncomp], si.numpy(), sd.numpy(), args.cloud, power=2)[0]
                nbytes = n * (16 * k + ncomp * (8 * k + 8))
                a, b = summary(a_ms), summary(b_ms)
                result["cases"].append({
                    "k": k, "ncomp": ncomp, "bytes": nbytes, "idw_gather": a, "gather_yardstick": b,
                    "idw_over_gather": round(a["median_ms"] / b["median_ms"], 4),
                    "idw_TBps": round(nbytes / a["median_ms"] / 1e9, 3),
                    "knn_query": summary(query_ms), "interpolate_scattered_s": round(whole_s, 3),
                    "interpolate_scattered_over_query": round(whole_s * 1e3 / float(np.median(query_ms)), 2),
                    "noutside": int(nout),
                    "host_points_per_s": round(len(sample) / host_s), "host_tree_build_s": round(tree_s, 2),
                    "sample_bits_agree": bool(SC.same_bits(got[sample].T, dev_sample)),
                    "host_rows_agree": bool(SC.same_bits(ref, dev_sample))})
                out_a.free(), out_b.free()
            idx.free(), dist.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
