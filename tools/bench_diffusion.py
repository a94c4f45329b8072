"""mm_gll_diffusion_apply and smooth_gll, timed with device events after warm-up.

* One K u on 1 M order-4 elements (125 M nodes, the mesh of tools/bench_mass.py), C = 1 and 3, isotropic and with the
  radial / lateral split, as TB/s of the byte model 24 + 16 C bytes per node, beside mm_gll_mass (32 bytes per node) timed
  in the same run.
* One full smooth of gll_mesh(44, 4) (sigma = 2 element widths, steps = 4, rtol = 1e-10): wall time, PCG iterations per
  step, and the time of the three parts of an iteration measured on their own -- the apply, the gather + scatter-sum
  around it, and the vector updates with their dots.

Writes profiles/diffusion_bench.json and prints it.  Usage: python tools/bench_diffusion.py [--reps N] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimesh_amd import helpers as H, synth  # noqa: E402
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


def apply_cases(ctx, reps):
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
    out = {"elements": E, "nodes": n,
           "mass": {"ms_median": round(ms, 4), "ms_min": round(ms_min, 4), "TBps": round(n * MASS_BYTES / ms / 1e9, 3)},
           "apply": []}
    del mass
    gen = torch.Generator(device=dev).manual_seed(0)
    for ncomp in (1, 3):
        u = torch.rand((ncomp, E, P), generator=gen, device=dev, dtype=torch.float64)
        y = torch.empty_like(u)
        for aniso in (0, 1):
            def run():
                rc = lib.mm_gll_diffusion_apply(ctx.handle, 4, 3, pts.data_ptr(), E, deriv.ptr, weights.ptr, u.data_ptr(),
                                                ncomp, 2.0, None, aniso, 0.5, None, y.data_ptr())
                assert rc == 0, rc
            ms, ms_min = timed(run, reps)
            nbytes = n * (24 + 16 * ncomp)
            out["apply"].append({"ncomp": ncomp, "anisotropic": bool(aniso), "ms_median": round(ms, 4),
                                 "ms_min": round(ms_min, 4), "counted_bytes": nbytes,
                                 "TBps": round(nbytes / ms / 1e9, 3)})
        del u, y
        torch.cuda.empty_cache()
    return out


def smooth_case(ctx, reps):
    n_side, order, steps, rtol = 44, 4, 4, 1e-10
    scale = 2.0 ** 32                                     # copies of a shared node made bit-identical (tests/diffusion_cases.py)
    gp = np.round(synth.gll_mesh(n_side, order, seed=1) * scale) / scale
    sigma = 2.0 / (n_side - 1)
    rng = np.random.default_rng(0)
    f = (np.cos(np.pi * gp[..., 0]) + 0.3 * rng.normal(size=gp.shape[:2]))[None]
    op = ctx.diffusion(order, gp, kappa_h=sigma * sigma)
    f_d = ctx.to_device(f)
    op.smooth(f_d, steps=1, rtol=1e-2)                    # warm-up: builds the assembly
    ctx.synchronize()
    t0 = time.perf_counter()
    op.smooth(f_d, steps=steps, rtol=rtol)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    its = [step[0] for step in op.last_iterations]
    a = op._asm
    nu, n = a["nu"], a["n"]
    x = ctx.to_device(rng.normal(size=(1, nu)))
    work = [ctx.to_device(rng.normal(size=(1, nu))) for _ in range(5)]      # r, z, p, ap, kp
    r, z, p, ap, kp = work
    ve, ye = ctx.empty((1, n), np.float64), ctx.empty((1, n), np.float64)
    state = ctx.to_device(np.array([[1.0, 1.0, 1.0, 1.0, 1e-3, 1e-3, 1.0, 0.0]]))
    nact = ctx.zeros((1,), np.int64)
    lib, h = ctx.lib, ctx.handle

    def run_apply():
        op._apply(ve.ptr, 1, ye.ptr)

    def run_assembly():
        op._gather(x, 1, ve)
        a["op"].apply(ye, point_major=False, out=kp)

    def run_vectors():                                    # what an iteration does besides K p, without the readback
        lib.mm_divide_rows(h, r.ptr, a["mass"].ptr, nu, 1, z.ptr)
        op._dots(r, z, nu, 1, state, H.MM_PCG_RZ)
        lib.mm_pcg_scalars(h, state.ptr, 1, H.MM_PCG_PHASE_ALPHA, rtol, nact.ptr)
        lib.mm_pcg_direction(h, state.ptr, z.ptr, nu, 1, p.ptr)
        op._combine(a["mass"], p, 0.125, kp, nu, 1, ap)
        op._dots(p, ap, nu, 1, state, H.MM_PCG_PAP)
        lib.mm_pcg_scalars(h, state.ptr, 1, H.MM_PCG_PHASE_ALPHA, rtol, None)
        lib.mm_pcg_advance(h, state.ptr, p.ptr, ap.ptr, nu, 1, x.ptr, r.ptr)

    parts = {name: round(timed(fn, reps)[0], 4) for name, fn in (("apply_ms", run_apply), ("gather_scatter_ms", run_assembly),
                                                                 ("vector_updates_ms", run_vectors))}
    total_its = sum(its)
    out = {"mesh": f"gll_mesh({n_side}, {order})", "elements": int(gp.shape[0]), "nodes": int(n), "unique_nodes": int(nu),
           "sigma_element_widths": 2.0, "steps": steps, "rtol": rtol, "iterations_per_step": its,
           "wall_s": round(wall, 4), "ms_per_iteration": round(1e3 * wall / max(total_its, 1), 4), **parts}
    op.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusion_bench.json"))
    args = ap.parse_args()
    torch.cuda.init()
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    doc = {"what": "mm_gll_diffusion_apply beside mm_gll_mass (device events, median of --reps after warm-up) and one "
                   "smooth of gll_mesh(44, 4)",
           "bytes_per_node": {"mass": MASS_BYTES, "apply": "24 + 16 C"}, "reps": args.reps}
    doc["one_million_elements"] = apply_cases(ctx, args.reps)
    torch.cuda.empty_cache()
    doc["smooth"] = smooth_case(ctx, args.reps)
    torch.cuda.synchronize()
    ctx.close()
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
