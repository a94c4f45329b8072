"""mm_radial_bins, mm_binned_weighted_sum and mm_radial_model_apply, timed with device events after warm-up, beside
mm_weighted_sum on the same arrays in the same process (the yardstick: one pass of 16 B per value and component, no bins):

* a 1 M-element order-4 chunk of a spherical shell (125 M values), elements ordered shell by shell, so that a chunk of
  4096 values (about 33 elements) spans a few bins: 1 and 4 components, 64 and 512 bins;
* a shuffled cloud of 16 M values with random bins: every chunk spans all bins (ceil(nbins / 8) windows per chunk).

Counted bytes per value: bins 24 read + 4 written; binned sum 8 (mass) + 4 (bin) + 8 per component, the mass and the bins
read again for every component; model apply 24 + 8 written per component (mode 0), + 8 read per component (mode 2).
Also times NumPy's bincount(weights=...) on every 50th value, with the download it needs.
Writes profiles/radial_bench.json and prints it.  Usage: python tools/bench_radial.py [--reps N] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import synth  # noqa: E402
from multimesh_amd.device import Context  # noqa: E402


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


def row(name, ms, nbytes, **extra):
    d = {"what": name, "ms_median": round(ms[0], 4), "ms_min": round(ms[1], 4), "counted_bytes": int(nbytes),
         "TBps": round(nbytes / ms[0] / 1e9, 3)}
    d.update(extra)
    return d


def sums(ctx, lib, mass, fields, bins, n, reps, label):
    """The binned sum for 1 and 4 components and 64 / 512 bins beside mm_weighted_sum; bins: {nbins: int32 tensor}."""
    rows = []
    for ncomp in (1, 4):
        out1 = torch.empty(ncomp, device=mass.device, dtype=torch.float64)
        check = []
        plain = timed(lambda: check.append(lib.mm_weighted_sum(ctx.handle, mass.data_ptr(), fields.data_ptr(), n, ncomp,
                                                              out1.data_ptr())), reps)
        assert not any(check), check
        rows.append(row(f"{label}: mm_weighted_sum, {ncomp} comp", plain, n * 16 * ncomp, ncomp=ncomp))
        for nbins, b in bins.items():
            out = torch.empty((ncomp, nbins), device=mass.device, dtype=torch.float64)
            check = []
            t = timed(lambda: check.append(lib.mm_binned_weighted_sum(ctx.handle, mass.data_ptr(), fields.data_ptr(),
                                                                      b.data_ptr(), n, ncomp, nbins, 0, out.data_ptr(),
                                                                      None)), reps)
            assert not any(check), check
            rows.append(row(f"{label}: mm_binned_weighted_sum, {ncomp} comp, {nbins} bins", t, n * 20 * ncomp, ncomp=ncomp,
                            nbins=nbins, time_over_weighted_sum=round(t[0] / plain[0], 3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--side", type=int, default=100, help="elements per side of the chunk (100: 1 M elements)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radial_bench.json"))
    args = ap.parse_args()
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    results = []

    # ---- the chunk: side^3 order-4 elements of a shell, [shell, lat, lon] with the shell slowest
    s = args.side
    g = torch.from_numpy((synth.gll_nodes_1d(4) + 1.0) / 2.0).to(dev)
    cell = torch.arange(s, device=dev, dtype=torch.float64)
    unit = (cell[:, None] + g[None, :]) / s                                          # [side, 5] in [0, 1]
    rad = 3.5e6 + unit * (6.371e6 - 3.5e6)
    lat = torch.deg2rad(-20.0 + unit * 40.0)
    lon = torch.deg2rad(-20.0 + unit * 40.0)
    shape = (s, s, s, 5, 5, 5)
    R = rad[:, None, None, :, None, None].expand(shape)
    LA = lat[None, :, None, None, :, None].expand(shape)
    LO = lon[None, None, :, None, None, :].expand(shape)
    pts = torch.stack([R * torch.cos(LA) * torch.cos(LO), R * torch.cos(LA) * torch.sin(LO), R * torch.sin(LA)], dim=-1)
    pts = pts.reshape(s ** 3, 125, 3).contiguous()
    E, n = s ** 3, s ** 3 * 125
    deriv, weights = ctx.to_device(synth.gll_derivative_matrix(4)), ctx.to_device(synth.gll_weights_1d(4))
    mass_t = torch.empty(n, device=dev, dtype=torch.float64)
    n_bad = lib.mm_gll_mass(ctx.handle, 4, 3, pts.data_ptr(), E, deriv.ptr, weights.ptr, mass_t.data_ptr(), None)
    assert n_bad in (0, n), n_bad                       # (a left-handed chunk has |det J| as its mass all the same)
    fields = torch.randn((4, n), generator=gen, device=dev, dtype=torch.float64) + 4.0
    bins, edges = {}, {}
    for nbins in (64, 512):
        e = ctx.to_device(np.linspace(3.5e6 - 1.0, 6.371e6 + 1.0, nbins + 1))
        b = torch.empty(n, device=dev, dtype=torch.int32)
        outside = []
        t = timed(lambda: outside.append(lib.mm_radial_bins(ctx.handle, pts.data_ptr(), n, e.ptr, nbins, b.data_ptr(), None)),
                  args.reps)
        assert outside[-1] == 0, outside[-1]
        results.append(row(f"chunk: mm_radial_bins, {nbins} bins", t, n * 28, nbins=nbins))
        bins[nbins], edges[nbins] = b, e
    results += sums(ctx, lib, mass_t, fields, bins, n, args.reps, "chunk")

    # NumPy on every 50th value: the download and the bincount
    t0 = time.perf_counter()
    m_h, f_h, b_h = mass_t[::50].cpu().numpy(), fields[0, ::50].cpu().numpy(), bins[512][::50].cpu().numpy()
    t1 = time.perf_counter()
    np.bincount(b_h, weights=m_h * f_h, minlength=512)
    t2 = time.perf_counter()
    results.append({"what": "NumPy on every 50th value of the chunk, 1 comp, 512 bins", "values": int(m_h.size),
                    "download_ms": round((t1 - t0) * 1e3, 3), "bincount_ms": round((t2 - t1) * 1e3, 3),
                    "scaled_to_all_values_ms": round((t2 - t0) * 1e3 * 50, 1)})

    # ---- the 1-D table on the nodes: ten layers of twenty rows
    bounds = np.linspace(3.4e6, 6.4e6, 11)
    rr = np.concatenate([np.linspace(a, b, 20) for a, b in zip(bounds[:-1], bounds[1:])])
    table = ctx.to_device(rr)
    out = torch.empty((4, n), device=dev, dtype=torch.float64)
    for ncomp in (1, 4):
        vals = ctx.to_device(np.cos(np.arange(ncomp * rr.size, dtype=np.float64)).reshape(ncomp, -1) + 4.0)
        for mode in (0, 2):
            check = []
            t = timed(lambda: check.append(lib.mm_radial_model_apply(ctx.handle, pts.data_ptr(), E, 125, table.ptr, vals.ptr,
                                                                     rr.size, ncomp, mode, fields.data_ptr(), out.data_ptr())),
                      args.reps)
            assert not any(check), check
            nbytes = n * (24 + 8 * ncomp + (8 * ncomp if mode else 0))
            results.append(row(f"chunk: mm_radial_model_apply, mode {mode}, {ncomp} comp", t, nbytes, ncomp=ncomp, mode=mode))
    del pts, out, fields, mass_t, bins
    torch.cuda.empty_cache()

    # ---- the shuffled cloud: 16 M values, every chunk spans every bin
    n = 16 * 1024 * 1024
    mass_t = torch.rand(n, generator=gen, device=dev, dtype=torch.float64) + 0.5
    fields = torch.randn((4, n), generator=gen, device=dev, dtype=torch.float64)
    bins = {nb: torch.randint(0, nb, (n,), generator=gen, device=dev, dtype=torch.int32) for nb in (64, 512)}
    results += sums(ctx, lib, mass_t, fields, bins, n, args.reps, "shuffled cloud")
    torch.cuda.synchronize()
    ctx.close()

    doc = {"what": "radial profiles beside mm_weighted_sum on the same arrays, device events, median of --reps after warm-up",
           "elements": E, "values": E * 125, "cloud_values": n, "reps": args.reps, "cases": results}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
