"""The tiled kNN kernels (knn_strip_kernel modes 0, 1 and 2, knn_cell_kernel) against another build of the library.

  python tools/bench_knn_tiles.py --row strip            one row in this process: a JSON line {"k8": {...}, ...}
  python tools/bench_knn_tiles.py --parent-lib DIR --out profiles/NAME.json [--rows strip,graded,...]
      every row three times, alternately with the library under DIR (first in each pair) and with the package's own,
      each run in a fresh process (MM_KNN_KERNEL is read once per process); bound = the other library's slowest run
      plus its spread (max - min of its three); within = this library's median lies at or below it.

Rows: strip    10 M uniform 3-D sources and targets, k = 8, 20, 32, MM_KNN_KERNEL=strip        (mode 0)
      graded   the clouds of tools/bench_knn_graded.py (4 M: u^1, u^1.5, u^2, u^3 and the refined region), levels on,
               tree off, k = 20, 32                                                            (modes 1 and 2)
      cell     10 M uniform 2-D sources and targets, k = 8, 20, 25, 32, MM_KNN_KERNEL=cell     (int64 ids)
      cell_int the fused hex8 pipeline with eager lists, hex_mesh(129) onto hex_mesh(127), k = 16, 20, 25, 32,
               MM_KNN_KERNEL=cell                                                              (int32 ids)
      split    1 M sources, 50 M targets reaching past the box, k = 8, MM_KNN_KERNEL=strip     (nsplit > 1)
      headline bench.py --gpus 1 (the lane kernel, for comparison)
Figures: the knn_cell stage and knn_query of Context.last_timings(), ms, third call of each; beside them the kernels
that served the call (Context.last_knn_kernels)."""
import argparse
import json
import os
import runpy
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"strip": {"MM_KNN_KERNEL": "strip"}, "graded": {"MM_KNN_TREE": "0"}, "cell": {"MM_KNN_KERNEL": "cell"},
        "cell_int": {"MM_KNN_KERNEL": "cell"}, "split": {"MM_KNN_KERNEL": "strip"}, "headline": {}}
NOTE = ("parent commit and this one (the same Python layer, the library swapped) run alternately, three times, parent first "
        "in each pair, each run in a fresh process with the kernel forced: tools/bench_knn_tiles.py. ms. bound = the parent's "
        "slowest run plus its spread (max - min of its three); within = the new median lies at or below it. kernels = what "
        "Context.last_knn_kernels reported for the case, every run.")


def clouds(row):
    import numpy as np

    rng = np.random.default_rng(0)
    if row == "strip":
        n = 10_000_000
        yield "", rng.uniform(size=(n, 3)), rng.uniform(size=(n, 3)), (8, 20, 32)
    elif row == "cell":
        n = 10_000_000
        yield "", rng.uniform(size=(n, 2)), rng.uniform(size=(n, 2)), (8, 20, 25, 32)
    elif row == "split":
        yield "", rng.uniform(size=(1_000_000, 3)), rng.uniform(-0.1, 1.1, size=(50_000_000, 3)), (8,)
    elif row == "graded":
        n = 4_000_000
        for power in (1.0, 1.5, 2.0, 3.0):
            # (u^1 is uniform: at k = 20 the lane kernel serves it, not a tiled one)
            ks = (32,) if power == 1.0 else (20, 32)
            yield f"power_{power}_", rng.uniform(size=(n, 3)) ** power, rng.uniform(size=(n, 3)) ** power, ks

        def two_density(m):
            return np.concatenate([rng.uniform(size=(m // 2, 3)), 0.35 + 0.2 * rng.uniform(size=(m - m // 2, 3))])

        yield "refined_region_", two_density(n), two_density(n), (20, 32)


def case_figures(ctx):
    t = ctx.last_timings()
    return {"knn_cell_ms": round(t["knn_cell"], 4), "knn_query_ms": round(t["knn_query"], 4),
            "kernels": sorted(ctx.last_knn_kernels())}


def run_row(row, lib_dir):
    sys.path.insert(0, ROOT)
    from multimesh_amd import helpers

    if lib_dir:
        helpers.LIB_DIR = os.path.abspath(lib_dir)
    if row == "headline":
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3", "--no-cpu-baseline"]
        runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
        return
    from multimesh_amd.device import Context

    ctx = Context(0)
    ctx.set_profiling(True)
    out = {}
    if row == "cell_int":
        from multimesh_amd import synth

        pa, ca = synth.hex_mesh(129, seed=1)
        pb, _ = synth.hex_mesh(127, seed=7)
        fields = synth.vector_field(pa)[:1]
        ctx.set_lazy_lists(False)
        for k in (16, 20, 25, 32):
            for _ in range(3):
                ctx.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=k)
            out[f"k{k}"] = case_figures(ctx)
    for tag, src, tgt, ks in clouds(row):
        d_src, d_tgt = ctx.to_device(src), ctx.to_device(tgt)
        tree = ctx.knn_build(d_src)
        for k in ks:
            for _ in range(3):
                tree.query(d_tgt, k)
            out[f"{tag}k{k}"] = case_figures(ctx)
        tree.free()
    print(json.dumps(out))


def figures(row, line):
    """({name: ms}, {case: kernels}) of one run's JSON line."""
    if row == "headline":
        return {"headline.ms_per_step": line["ms_per_step"]}, {}
    ms = {f"{row}.{case}.{key}": v[key] for case, v in line.items() for key in ("knn_cell_ms", "knn_query_ms")}
    return ms, {f"{row}.{case}": v["kernels"] for case, v in line.items()}


def compare(parent_lib, rows, out_path):
    runs, kernels = {}, {}
    for row in rows:
        env = dict(os.environ, **ROWS[row])
        for _ in range(3):
            for side, lib in (("parent", parent_lib), ("new", "")):
                cmd = [sys.executable, os.path.abspath(__file__), "--row", row] + (["--lib-dir", lib] if lib else [])
                r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
                if r.returncode != 0:
                    sys.exit(f"{row} ({side}) ended with {r.returncode}: {r.stderr[-2000:]}")
                ms, served = figures(row, json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
                for name, v in ms.items():
                    runs.setdefault(name, {"parent": [], "new": []})[side].append(v)
                for case, names in served.items():
                    if kernels.setdefault(case, names) != names:
                        sys.exit(f"{case}: kernels {names} in one run, {kernels[case]} in another")
                print(row, side, json.dumps(ms), flush=True)
    for v in runs.values():
        p, n = sorted(v["parent"]), sorted(v["new"])
        v.update(parent_median=p[1], new_median=n[1], bound_parent_slowest_plus_spread=round(p[2] + p[2] - p[0], 4))
        v["within"] = v["new_median"] <= v["bound_parent_slowest_plus_spread"]
    with open(out_path, "w") as f:
        json.dump({"note": NOTE, "kernels": kernels, "rows": runs}, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", choices=sorted(ROWS))
    ap.add_argument("--lib-dir", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rows", default="strip,graded,cell,cell_int,split,headline")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.row:
        for key, val in ROWS[a.row].items():
            os.environ.setdefault(key, val)
        run_row(a.row, a.lib_dir)
    else:
        if not (a.parent_lib and a.out and os.path.isdir(a.parent_lib)):
            ap.error("--row, or --parent-lib DIR with --out FILE")
        if set(a.rows.split(",")) - set(ROWS):
            ap.error(f"--rows: among {sorted(ROWS)}")
        compare(a.parent_lib, a.rows.split(","), a.out)
