#!/usr/bin/env python3
"""Benchmark of the mesh-to-mesh interpolation hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload metric|cfg2|cfg3|cfg4|cfg5] [--scaling strong|weak]
                    [--full] [--dump-outputs DIR]

With N > 1 and no WORLD_SIZE in the environment this process is only a launcher: it starts N
fresh ranks (``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
127.0.0.1 ...``) BEFORE anything touches a GPU, passes their output through and exits with their
code (non-zero when the node has fewer than N devices).  Started by ``torch.distributed.run``
itself (RANK / LOCAL_RANK / WORLD_SIZE set) it is one rank: one process per GPU, RCCL over xGMI.

A "step" is one pass of the whole hot path (reference scripts/cli.py:62-100) over one batch of
synthetic targets with every input already resident in HBM: element centroids -> search-grid
build -> k nearest centroids -> hex8 Newton location -> weighted gather (-> one RCCL all-gather of
the interpolated field when N > 1).

Workloads:
  metric  BASELINE.json's metric configuration: 10M -> 10M nodes (216^3 jittered hex meshes),
          1 scalar field, k = 20.
  cfg3    the same with the 3-component vector field;  cfg2: 1M -> 1M.
  cfg4    100.5M-node target mesh (465^3, seed 7) cut into 8 contiguous shards
          (``shard_bounds(465^3, 8, s)``, ~12.57M targets = a 58-plane slab each) over the replicated
          216^3 source.  Rank r interpolates shard r (8 ranks = the whole mesh; fewer ranks = the
          first N shards; 1 rank: shard ``--cfg4-shard``, default 0), so per-GPU work is fixed.
  cfg5    order-4 GLL hexes: 43^3 source elements, targets = the unique GLL points of a 47^3-element
          mesh (found on the device: mm_unique_points), fused mm_interpolate_gll, k = 20, tolerance 1.05
          (reference components/interpolator.py:931-977, 1181-1233).  PARITY UNPINNED (salvus.fem absent).

Scaling at N > 1 (reference interpolator.py:1239-1254 chunks ONE target set):
  strong  (default for metric / cfg2 / cfg3 / cfg5) ONE target mesh; rank r takes rows
          ``shard_bounds(N_targets, world, r)``; one all-gather reassembles the field, which is compared
          WHOLE with a single-rank run.  The line also carries a weak-scaling measurement (`weak`)
          and the replicated (Amdahl) share of a step: centroids + grid build run on every rank.
  weak    every rank interpolates its own full-size target mesh (jitter seed 7 + rank); cfg4 is weak by
          construction (one fixed-size shard per rank).

Rank 0 prints ONE JSON line on stdout (everything else, RCCL's banner included, goes to stderr).  A plain run sets
up, warms up, times the K steps and prints the contract fields (metric, value, unit, higher_is_better, dtype,
ms_per_step = wall time of the K steps / K) with the configuration, the failed count and the fp mode.
--dump-outputs DIR then writes what the last timed step handed its caller as DIR/<name>.npy (float64, at most
DUMP_BYTES: a fixed sample of the rows beyond that, their row numbers in rows.npy); the inputs are seeded, so two
builds can be compared output for output.  --full adds what takes runs of its own:
  "roofline":      HBM roofline of the dominant single kernel, named as rocprofv3 names it,
  "roofline_valu": the VALU-issue floor of the two dominant kernels (instruction counts by class from the
                   committed counter passes x the measured issue cost of each class),
  "stages":        the byte accounting for every stage (SURVEY 8(d)'s figure and the bytes really moved),
  "gather_reapply": the stand-alone A9 gather on the operator of this very run,
  "fp_mode.other_mode", "resident_source", "host_arrays": the same step in the other arithmetic, on a source
                   mesh kept resident and from host arrays,
  "allgather":     the collective timed by itself + the whole-field comparison (N > 1),
  "cpu_baseline":  the reference's CPU path timed on this box's host cores on a bounded sample.
cfg5 times every stage inside its steps, so its plain line keeps "roofline", "roofline_valu" and "stages"; --full
adds "allgather" and "cpu_baseline".
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from multimesh_amd import synth  # noqa: E402
from multimesh_amd.distributed import shard_bounds  # noqa: E402
from multimesh_amd.helpers import STAGES  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); a device-to-device copy reaches ~5 TB/s (roofline.measured_copy_GBps)
CFG4_SHARDS = 8
LAZY_K = 8              # candidates the kNN stage delivers up front (mm_set_lazy_lists)
N_SIMD = 256 * 4        # MI355X: 256 CUs x 4 SIMDs
VERIFY_CHUNK = 16_000_000   # rows per single-rank call of the whole-field comparison
DUMP_BYTES = 60_000_000     # --dump-outputs: data written at most (64 MB in all with the row numbers and .npy headers)


def algorithmic_bytes(n_targets, n_elem, n_nodes, k, ncomp):
    """algorithmic bytes per launch of each stage (reference dtypes: int64 ids, fp64).

    knn_cell / locate_pass0 are single kernels inside the knn_query / locate stages and are
    priced with the whole stage's algorithmic bytes (they do the stage's work; the other
    kernels of the stage are its bookkeeping)."""
    knn = n_targets * (24 + 8 * k) + n_elem * 24
    loc = n_targets * (24 + 8 * k + 64 + 192 + 128)
    return {
        "centroid": n_elem * (8 * 8 + 8 * 24 + 24),
        "knn_build": n_elem * 24 * 2,                       # read centroids, write them cell-sorted
        "knn_query": knn,
        "locate": loc,
        "gather": n_targets * (128 + 72 * ncomp),
        "knn_cell": knn,
        "locate_pass0": loc,
    }


def actual_bytes(n_targets, n_elem, n_nodes, k, ncomp, fused_gather):
    """Bytes the implementation has to move through HBM at least once per launch:
    every array counted ONCE however often the kernels re-read it through L2 (node coordinates are
    shared by 8 elements, gathered field values by 8 targets), in the dtypes actually stored
    (int32 candidate rows of LAZY_K entries, 32-byte sorted records)."""
    kq = min(k, LAZY_K)
    knn_cell = n_targets * (32 + 4 * kq) + n_elem * 32        # target records in, int32 rows out, source records once
    loc = n_targets * (24 + 4 * kq) + n_elem * 64 + n_nodes * 24   # points + candidate rows, mesh once
    loc += n_targets * 8 * ncomp + n_nodes * 8 * ncomp if fused_gather else n_targets * 128
    return {
        "centroid": n_elem * 64 + n_nodes * 24 + n_elem * 24,
        "knn_build": n_elem * (24 + 8 + 8 + 24 + 32),        # centroids twice, {cell, rank} out and in, records out
        "knn_query": knn_cell + n_targets * (24 + 8 + 8 + 24 + 32),   # + the counting sort of the targets
        "locate": loc,
        "gather": n_targets * (128 + 8 * ncomp) + n_nodes * 8 * ncomp,
        "knn_cell": knn_cell,
        "locate_pass0": loc,
    }


def gll_bytes(n_targets, n_elem, P, dim, k, ncomp):
    """SURVEY.md §8(d) for the GLL path: locate ~ point + k candidates + one element's control nodes + the
    coefficient row; gather = element id + P coefficients + C * (P gathered + 1 written)."""
    return {
        "knn_query": n_targets * (8 * dim + 8 * k) + n_elem * 8 * dim,
        "locate": n_targets * (8 * dim + 8 * k + 8 * P * dim + 8 + 8 * P),
        "gather": n_targets * (8 + 8 * P + ncomp * (8 * P + 8)),
    }


#: stages that are ONE kernel launch each (candidates for the "dominant kernel" roofline), by the name
#: rocprofv3 --kernel-trace prints for them (profiles/*_kernel_stats.csv)
SINGLE_KERNEL_STAGES = ("centroid", "knn_cell", "locate_pass0", "gather")
KERNEL_OF_STAGE = {"centroid": "centroid_bbox_kernel", "knn_cell": "knn_lane_kernel<8, int, false>",
                   "locate_pass0": "locate_pass_kernel<true, int, true, int, true>", "gather": "gather8_kernel<true>"}
LOCATE_KERNEL = {"tol": "locate_pass_kernel<true, int, true, int, true>", "exact": "locate_pass_kernel<true, int, true, int, false>"}
#: what the counters say limits each of them: the two big kernels sit on the vector-issue
#: floor, the streaming ones on HBM
BOUND_OF_STAGE = {"centroid": "hbm", "knn_cell": "valu", "locate_pass0": "valu", "gather": "hbm"}
#: ... the locate pass by mode: the reference's arithmetic is bound by fp64 issue, the MM_FP_TOL one by the L1's misses in
#: flight (profiles/r04_mem_counters_tol.json: ~55 line requests outstanding per CU at ~560 cycles each)
LOCATE_BOUND = {"tol": "l1_miss_concurrency", "exact": "valu"}
METRIC_OF_WORKLOAD = {
    "metric": "interpolated points/sec, 10M->10M 3D mesh, 1 scalar field",
    "cfg2": "interpolated points/sec, 1M->1M 3D hex mesh, 1 scalar field (BASELINE configs[1])",
    "cfg3": "interpolated points/sec, 10M->10M 3D mesh, 3-component vector field (BASELINE configs[2])",
    "cfg4": "interpolated points/sec, 100M-target / 10M-source 3D mesh, one of 8 target shards per GPU (BASELINE configs[3])",
}
TOL_STATEMENT = ("MM_FP_TOL: node ids and failed count bit-identical to the reference; weights within 1e-12 (absolute, they are O(1)) "
                 "and values within 1e-12 * 8 * max|field| -- in general max(1e-12, 64 eps max|x| / shortest element edge)")
#: key of the kernel in profiles/*_knn_counters.json
COUNTER_KEY = {"knn_cell": "knn_lane_kernel", "locate_pass0": "locate_pass_kernel"}
SINGLE_KERNEL_STAGES_TIMED_LIVE = ("knn_cell", "locate_pass0")   # mm_set_profiling(ctx, 2)
STAGE_TABLE_STEPS = 3


def _latest(pattern):
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return files[-1] if files else None


def measured_traffic(kernel_stage):
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/*_pmc_traffic.json,
    FETCH_SIZE doubled for wide streaming reads as MI355X_MICROARCH.md prescribes); None if absent."""
    f = _latest("*_pmc_traffic.json")
    if not f:
        return None
    try:
        return json.load(open(f)).get(kernel_stage, {}).get("hbm_bytes_per_launch")
    except Exception:
        return None


def valu_floor(stage, ms, scale=1.0, pattern="*_knn_counters.json", key=None, kernel=None, run_steps=None):
    """VALU-issue floor of a kernel: wave-instructions per launch by class (profiles/*_knn_counters.json:
    SQ_INSTS_VALU and its ADD/MUL/FMA_F32 sub-counters, collected on the metric workload) x the issue cost of
    each class at saturation (profiles/*_valu_issue.json from tools/valu_issue.hip: the fp32 add/mul/fmac class
    issues every ~2.4 cycles per SIMD, everything else -- min/max/med3, compares, three-operand and 64-bit
    forms -- every ~4.4), spread over the chip's 1024 SIMDs at the measured clock.  `scale` rescales the counts
    when the launch is not the metric workload's (targets ratio).  key: the counter profile's kernel entry, or a
    list of them with run_steps = the steps the counter run made: the kernels' run totals / run_steps are summed (a
    stage of several launches per step).  None when the profiles are absent."""
    fc, fi = _latest(pattern), _latest("*_valu_issue.json")
    key = key or COUNTER_KEY.get(stage)
    if not (fc and fi and key):
        return None
    try:
        prof = json.load(open(fc))
        issue = json.load(open(fi))
        fast_names = ("SQ_INSTS_VALU_ADD_F32", "SQ_INSTS_VALU_MUL_F32", "SQ_INSTS_VALU_FMA_F32")
        if isinstance(key, (list, tuple)):
            ents = [prof[kk] for kk in key if kk in prof]
            if not ents:
                return None
            total = sum(e["SQ_INSTS_VALU_run_total"] for e in ents) / run_steps * scale
            fast = sum(e.get(n + "_run_total", 0.0) for e in ents for n in fast_names) / run_steps * scale
            have_mix = all("SQ_INSTS_VALU_ADD_F32_run_total" in e for e in ents)
        else:
            c = prof.get(key, {})
            total = c["SQ_INSTS_VALU"] * scale
            fast = sum(c.get(n, 0.0) for n in fast_names) * scale
            have_mix = "SQ_INSTS_VALU_ADD_F32" in c
        slow = total - fast
        cyc = fast * issue["fast_class_cycles"] + slow * issue["slow_class_cycles"]
        floor_ms = cyc / N_SIMD / (issue["clock_GHz"] * 1e9) * 1e3
        return {"kernel": kernel or KERNEL_OF_STAGE[stage], "valu_wave_insts_per_launch": round(total),
                "fast_class_insts": round(fast) if have_mix else None,
                "issue_cycles": {"fast_class": issue["fast_class_cycles"], "slow_class": issue["slow_class_cycles"]},
                "clock_GHz": issue["clock_GHz"], "floor_ms": round(floor_ms, 4), "ms": round(ms, 4),
                "frac": round(floor_ms / ms, 4) if ms > 0 else None,
                "source": [os.path.relpath(fc, ROOT), os.path.relpath(fi, ROOT)],
                "note": "floor = (fast-class insts x fast cycles + the rest x slow cycles) / 1024 SIMDs / clock; "
                        "counts from the committed counter passes of the metric workload, not re-measured in this run"}
    except Exception as exc:   # a malformed profile must not break the bench line
        return {"error": f"{type(exc).__name__}: {exc}"}


def counter_profile_mode():
    """The fp mode the newest committed counter profile of the metric workload was taken in ("tol" / "exact"; profiles
    before round 4 are all "exact")."""
    f = _latest("*_knn_counters.json")
    if not f:
        return None
    try:
        return json.load(open(f)).get("_fp_mode", "exact")
    except Exception:
        return None


def memory_side_profile(stage, ms):
    """What the TA / TCP counters of the committed pass say about the dominant kernel (profiles/*_mem_counters*.json,
    tools/mem_counters.sh): L1 -> L2 read requests per launch, their mean latency, and by Little's law the line requests
    in flight per CU -- the quantity that bounds a gather-heavy kernel when the vector pipes are idle."""
    f = _latest("*_mem_counters*.json")
    key = COUNTER_KEY.get(stage)
    if not (f and key):
        return None
    try:
        c = json.load(open(f)).get(key, {})
        req, lat = c["TCP_TCC_READ_REQ_sum"], c["TCP_TCC_READ_REQ_LATENCY_sum"]
        cycles = c["GRBM_GUI_ACTIVE"] / 8.0                # per XCD
        return {"kernel": KERNEL_OF_STAGE[stage], "l1_to_l2_read_requests_per_launch": round(req),
                "mean_read_latency_cycles": round(lat / req, 1), "cus": 256,
                "read_requests_in_flight_per_cu": round(lat / (cycles * 256.0), 1),
                "tcp_pending_stall_share": round(c.get("TCP_PENDING_STALL_CYCLES_sum", 0.0) / (cycles * 256.0), 3),
                "ta_busy_share": round(c.get("TA_TA_BUSY_sum", 0.0) / (cycles * 256.0), 3),
                "source": os.path.relpath(f, ROOT),
                "note": "from the committed counter passes of the metric workload (one rocprofv3 pass per small group), not "
                        "re-measured in this run; requests in flight = sum of request latencies / (kernel cycles x 256 CUs)"}
    except Exception as exc:
        return {"error": f"{type(exc).__name__}: {exc}"}


def cpu_baseline(pa, ca, pb, fields, k, sample_stride):
    """The reference CPU path (cKDTree + compiled reference C + NumPy) on a bounded sample."""
    from oracle import oracle as O
    from scipy.spatial import cKDTree

    use_ref = O.have_reference()
    t0 = time.perf_counter()
    cen = O.ref_centroid(ca, pa) if use_ref else O.centroid(ca, pa)
    t_cen = time.perf_counter() - t0
    t0 = time.perf_counter()
    tree = cKDTree(cen, balanced_tree=False)                 # reference scripts/cli.py:66
    t_build = time.perf_counter() - t0
    sample = np.ascontiguousarray(pb[::sample_stride])
    t0 = time.perf_counter()
    _, nn = tree.query(sample, k=k)                          # no workers= -> 1 core, as the reference
    t_query = time.perf_counter() - t0
    conn = synth.reorder_hex8(ca)
    t0 = time.perf_counter()
    if use_ref:
        enc, w, nf = O.ref_locate_hex8(nn, conn, pa, sample)
    else:
        enc, w, nf = O.locate_hex8(nn, conn, pa, sample)
    t_locate = time.perf_counter() - t0
    t0 = time.perf_counter()
    vals = O.gather_numpy(fields, enc, w)
    t_gather = time.perf_counter() - t0
    per_point = (t_query + t_locate + t_gather) / len(sample)
    t_full = t_cen + t_build + per_point * len(pb)

    # "Best-effort CPU" beside it, so the speed-up is not flattered: NOT the
    # reference's behaviour -- cKDTree.query(workers=-1) and the locate restatement on one thread per
    # core (the C call releases the GIL; the reference's triLinearInterpolator is serial).
    from concurrent.futures import ThreadPoolExecutor

    ncores = os.cpu_count() or 1
    t0 = time.perf_counter()
    _, nn_mt = tree.query(sample, k=k, workers=-1)
    t_query_mt = time.perf_counter() - t0
    chunks = np.array_split(np.arange(len(sample)), ncores * 4)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(ncores) as pool:
        parts = list(pool.map(lambda c: O.locate_hex8(nn_mt[c], conn, pa, sample[c]), chunks))
    t_locate_mt = time.perf_counter() - t0
    enc_mt = np.concatenate([p[0] for p in parts])
    same = bool(np.array_equal(enc_mt, enc))
    t_full_mt = t_cen + t_build + (t_query_mt + t_locate_mt + t_gather) / len(sample) * len(pb)
    all_cores = {"value": len(pb) / t_full_mt, "unit": "points/s", "cores": ncores,
                 "note": (f"not the reference's behaviour: cKDTree.query(workers=-1) {t_query_mt:.2f}s + locate "
                          f"restatement on {ncores} threads {t_locate_mt:.2f}s on the same sample; tree build "
                          f"({t_build:.2f}s) and gather stay serial; same node ids as the serial run: {same}")}
    return {
        "value": len(pb) / t_full,
        "unit": "points/s",
        "cores": 1,
        "kind": "reference" if use_ref else "port",
        "sample": ((f"MEASURED on all {len(pb)} targets (no extrapolation): full {len(cen)}-element source (centroid {t_cen:.2f}s + "
                    f"cKDTree build {t_build:.2f}s), query {t_query:.2f}s, locate {t_locate:.2f}s, gather {t_gather:.3f}s; host has "
                    f"{os.cpu_count()} cores, path is single-threaded like the reference") if sample_stride == 1 else
                   (f"EXTRAPOLATED from a 1/{sample_stride} sample: full {len(cen)}-element source (centroid {t_cen:.2f}s + "
                    f"cKDTree build {t_build:.2f}s) + every {sample_stride}th target ({len(sample)} points: query "
                    f"{t_query:.2f}s, locate {t_locate:.2f}s, gather {t_gather:.3f}s), per-point cost extrapolated to "
                    f"{len(pb)} targets; host has {os.cpu_count()} cores, path is single-threaded like the reference; "
                    "profiles/r04_cpu_full.json holds one run over ALL targets: 283.8 k points/s")),
        "nfailed": int(nf),
        "all_cores": all_cores,
    }, (sample_stride, enc, w, vals)


def hbm_copy_gbps(torch, dev, nbytes=1 << 31, reps=10):
    """Device-to-device copy rate (read + write bytes / time): what this card's HBM delivers to the
    simplest streaming kernel, reported beside the nominal 8 TB/s the fractions are priced against."""
    a = torch.empty(nbytes // 8, dtype=torch.float64, device=dev).fill_(1.0)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    e1.synchronize()
    return 2.0 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def dump_outputs(path, torch, values, counts):
    """--dump-outputs: `values` (device tensor [rows, C]) as values.npy -- above DUMP_BYTES a fixed sample of rows
    (default_rng(0), ascending; their row numbers in rows.npy) -- and every scalar count of `counts` as <name>.npy."""
    os.makedirs(path, exist_ok=True)
    n, ncomp = values.shape
    if n * ncomp * 8 > DUMP_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(n, DUMP_BYTES // (8 * ncomp + 8), replace=False))
        values = values.index_select(0, torch.from_numpy(rows).to(values.device))
        np.save(os.path.join(path, "rows.npy"), rows.astype(np.float64))
    elif os.path.exists(os.path.join(path, "rows.npy")):
        os.remove(os.path.join(path, "rows.npy"))     # of an earlier, sampled dump into the same directory
    np.save(os.path.join(path, "values.npy"), values.cpu().numpy().astype(np.float64))
    for name, c in counts.items():
        np.save(os.path.join(path, name + ".npy"), np.array([c], dtype=np.float64))


WORKLOADS = sorted(list(synth.CONFIGS) + ["cfg5"])


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="metric", choices=WORKLOADS)
    ap.add_argument("--scaling", default="auto", choices=("auto", "strong", "weak"),
                    help="N > 1: strong = one target set sharded over the ranks (default except cfg4), weak = one full "
                         "target set per rank")
    ap.add_argument("--n-src", type=int, default=0, help="override nodes per side of the source mesh")
    ap.add_argument("--n-tgt", type=int, default=0, help="override nodes per side of the target mesh")
    ap.add_argument("--ncomp", type=int, default=0)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--cfg4-shard", type=int, default=0, help="cfg4 at one rank: which of the 8 shards")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--weak-beside", action="store_true",
                    help="strong scaling at N > 1: also make the short weak-scaling side run (every rank a full target mesh)")
    ap.add_argument("--no-weak-beside", action="store_true", help="(the default since round 4; kept for old command lines)")
    ap.add_argument("--cpu-sample-stride", type=int, default=0)
    ap.add_argument("--fp-mode", default="tol", choices=("tol", "exact"),
                    help="arithmetic of the hex8 locate stage (mm_set_fp_mode): tol = certified fast Newton, node ids bit-exact, "
                         "values to 1e-12 (north_star's contract; the default); exact = the reference's operations, 0 ulp")
    ap.add_argument("--full", action="store_true",
                    help="also the measurements and checks beyond the headline: stage table, rooflines, the other fp mode, "
                         "resident source, stand-alone gather, host arrays, CPU baseline and parity, all-gather comparison")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the outputs of the last timed step as DIR/<name>.npy (float64, a fixed sample beyond 60 MB)")
    ap.add_argument("--as-rank", default="", metavar="r/G",
                    help="PROJECTION, one process, no process group: run exactly rank r's share of a G-rank strong-scaling "
                         "run of the workload alone on this GPU (tools/strong_projection.py loops over r and G)")
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------
# launcher: N > 1 without a torchrun environment
# ------------------------------------------------------------------------------------------
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def count_gpus_without_runtime():
    """GPUs of this node from the KFD topology in sysfs (nodes with SIMDs are GPUs; CPUs have simd_count 0):
    nothing here loads the HIP runtime, so the launcher process never initialises a device.  None when the
    count cannot be had (then the ranks themselves fail when a device is missing)."""
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        n = 0
        for node in os.listdir(base):
            with open(os.path.join(base, node, "properties")) as f:
                for line in f:
                    if line.startswith("simd_count"):
                        n += int(line.split()[1]) > 0
                        break
        visible = os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES"))
        if visible is not None and visible.strip() != "":
            n = min(n, len([v for v in visible.split(",") if v.strip() != ""]))
        return n
    except OSError:
        pass
    # no KFD topology in sysfs (a container without the driver's sysfs tree): ask a CHILD process, which may
    # initialise whatever it likes and is gone before the ranks start
    try:
        r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"],
                           capture_output=True, text=True, timeout=300)
        return int(r.stdout.strip().splitlines()[-1])
    except Exception:
        return None


def under_profiler():
    """A rocprofiler tool library is preloaded into this process (rocprofv3 -- python3 bench.py ...): its
    library has initialised the GPU already, so starting ranks from here would be a launcher hop under it."""
    env = os.environ
    return any(k in env for k in ("ROCPROFILER_REGISTER_FORCE_LOAD", "ROCPROF_OUTPUT_PATH", "ROCP_TOOL_LIBRARIES",
                                  "ROCPROFILER_LIBRARY")) or "rocprofiler" in env.get("LD_PRELOAD", "")


def launch_ranks(args, argv):
    """Start ``args.gpus`` ranks as CHILD processes and return their exit code.  Nothing in this process
    touches the GPU runtime (devices are counted from sysfs), and nothing is exec'ed over it: the ranks are
    fresh interpreters started by torch.distributed.run."""
    rehearse = os.environ.get("MM_BENCH_REHEARSE") == "1"    # ranks share GPU 0, gloo carries the collectives
    if under_profiler():
        print("bench.py: --gpus N > 1 starts its own ranks and must not run under a profiler; profile one rank "
              "(rocprofv3 ... -- python3 bench.py --gpus 1 ...)", file=sys.stderr)
        return 2
    have = count_gpus_without_runtime()
    if have is not None and have < args.gpus and not rehearse:
        print(f"bench.py: --gpus {args.gpus} but this node has {have} GPU(s)", file=sys.stderr)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.run(cmd, env=env).returncode


class StdoutToStderr:
    """Everything written to file descriptor 1 while this is active -- RCCL prints a version banner there
    when a communicator is created -- goes to stderr; ``emit`` writes to the real stdout.  The contract is ONE
    JSON line on stdout."""

    def __enter__(self):
        sys.stdout.flush()
        self.real = os.dup(1)
        os.dup2(2, 1)
        return self

    def emit(self, text):
        os.write(self.real, (text + "\n").encode())

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.real, 1)
        os.close(self.real)


# ------------------------------------------------------------------------------------------
# one rank
# ------------------------------------------------------------------------------------------
class Dist:
    """The process group of a run (or its single-process stand-in)."""

    def __init__(self, torch, dist, dev, world, rehearse, use_dist):
        self.torch, self.dist, self.dev, self.world, self.rehearse, self.use = torch, dist, dev, world, rehearse, use_dist
        self.backend = ("gloo (REHEARSAL: ranks share GPU 0)" if rehearse else "nccl (RCCL)") if use_dist else None

    def barrier(self):
        if self.use:
            self.dist.barrier()

    def all_gather(self, t_all, t_out, async_op=False):
        """The one collective of the path: equal, padded blocks -> [world*chunk, C]."""
        if self.rehearse:     # gloo has no device all-gather: staged through the host (control flow only)
            parts = [self.torch.empty(t_out.shape, dtype=t_out.dtype) for _ in range(self.world)]
            self.dist.all_gather(parts, t_out.cpu())
            t_all.copy_(self.torch.cat(parts))
            return None
        return self.dist.all_gather_into_tensor(t_all, t_out, async_op=async_op)

    def all_max(self, x):
        if not self.use:
            return x
        t = self.torch.tensor([x], dtype=self.torch.float64, device="cpu" if self.rehearse else self.dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def all_sum_int(self, x):
        if not self.use:
            return x
        t = self.torch.tensor([x], dtype=self.torch.int64, device="cpu" if self.rehearse else self.dev)
        self.dist.all_reduce(t)
        return int(t.item())


def init_rank(args):
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        return None
    rehearse = os.environ.get("MM_BENCH_REHEARSE") == "1"
    dev_index = 0 if rehearse else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    # MM_BENCH_FORCE_DIST=1 exercises the RCCL path (init, barrier, all-gather) even at world size 1
    use_dist = world > 1 or (os.environ.get("MM_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    return torch, dist, rank, world, dev_index, dev, Dist(torch, dist, dev, world, rehearse, use_dist)


def timed_steps(args, torch, D, step, drain):
    """W untimed warm-up steps, then EXACTLY K steps bracketed by barrier + synchronize on both sides;
    the MAX over ranks of the elapsed wall time."""
    for _ in range(args.warmup):
        step(False)
    drain()
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(True)
    drain()                            # every gather of the timed steps has completed ...
    torch.cuda.synchronize()           # ... and so has everything else on the device
    D.barrier()
    return D.all_max(time.perf_counter() - t0)


def run_rank(args, out):
    init = init_rank(args)
    if init is None:
        return 2
    if args.workload == "cfg5":
        return run_rank_gll(args, out, *init)
    return run_rank_hex8(args, out, *init)


def run_rank_hex8(args, out, torch, dist, rank, world, dev_index, dev, D):
    use_dist, rehearse = D.use, D.rehearse
    cfg = dict(synth.CONFIGS[args.workload])
    n_src = args.n_src or cfg["n_src"]
    n_tgt = args.n_tgt or cfg["n_tgt"]
    ncomp = args.ncomp or cfg["ncomp"]
    k = args.k
    sharded = args.workload == "cfg4"
    scaling = args.scaling if args.scaling != "auto" else ("weak" if sharded else "strong")
    # --as-rank r/G: this single process plays rank r of a G-rank strong-scaling run, alone on its GPU (a PROJECTION of
    # what that rank's step would cost: no process group, no collective)
    as_rank = bool(args.as_rank)
    proj_rank, proj_world = 0, world
    if as_rank:
        try:
            proj_rank, proj_world = (int(v) for v in args.as_rank.split("/"))
            assert 0 <= proj_rank < proj_world
        except Exception:
            print("bench.py: --as-rank wants r/G with 0 <= r < G", file=sys.stderr)
            return 2
        if world != 1 or sharded or scaling != "strong":
            print("bench.py: --as-rank is a one-process projection of a strong-scaling rank (not cfg4, --gpus 1)", file=sys.stderr)
            return 2
    if sharded and scaling == "strong":
        if rank == 0:
            print("bench.py: cfg4 is one fixed shard per rank (weak scaling by construction)", file=sys.stderr)
        return 2

    # ---- synthetic inputs (host), then resident in HBM before any timing ----
    pa, ca = synth.hex_mesh(n_src, seed=1)
    n_all = n_tgt ** 3
    if sharded:
        # rank r owns shard r of the 8 the 100.5M-node target mesh is cut into (never a cube of its own)
        if not 0 <= args.cfg4_shard < CFG4_SHARDS or world > CFG4_SHARDS:
            if rank == 0:
                print("bench.py: cfg4 has 8 shards", file=sys.stderr)
            return 2

        def bounds(r):
            return shard_bounds(n_all, CFG4_SHARDS, r if world > 1 else args.cfg4_shard)

        def tgt_rows(r, a, b):
            """rows [a, b) of rank r's block of targets"""
            return synth.hex_mesh_rows(n_tgt, bounds(r)[0] + a, bounds(r)[0] + b, seed=7)

        chunk = -(-n_all // CFG4_SHARDS)          # ceil: the last shard is 7 rows short, blocks are padded
        lo, hi = bounds(rank)
        target_desc = (f"shard {rank if world > 1 else args.cfg4_shard} of {CFG4_SHARDS} of the {n_tgt}^3 = {n_all}-node target "
                       f"mesh (rows {lo}..{hi}: a {(hi - 1) // n_tgt ** 2 - lo // n_tgt ** 2 + 1}-plane slab), rank r <-> shard r")
    elif scaling == "strong":
        def bounds(r):
            return shard_bounds(n_all, proj_world, proj_rank if as_rank else r)

        def tgt_rows(r, a, b):
            return synth.hex_mesh_rows(n_tgt, bounds(r)[0] + a, bounds(r)[0] + b, seed=7)

        chunk = -(-n_all // proj_world)
        lo, hi = bounds(rank)
        target_desc = (f"ONE {n_tgt}^3 = {n_all}-node target mesh (jitter seed 7)" +
                       (f", rank r takes rows shard_bounds({n_all}, {world}, r) (this rank: {lo}..{hi})" if world > 1 else "") +
                       (f"; PROJECTION: rows shard_bounds({n_all}, {proj_world}, {proj_rank}) = {lo}..{hi}, the share of rank "
                        f"{proj_rank} of {proj_world}, run alone" if as_rank else ""))
    else:
        def bounds(r):
            return 0, n_all

        def tgt_rows(r, a, b):
            return synth.hex_mesh_rows(n_tgt, a, b, seed=7 + r)

        chunk = n_all
        target_desc = f"every rank its own {n_tgt}^3-node target mesh (jitter seed 7 + rank)"
    n_rows = [bounds(r)[1] - bounds(r)[0] for r in (range(world) if world > 1 else [rank])]
    n_local = bounds(rank)[1] - bounds(rank)[0]
    total_targets = sum(n_rows)
    pb = tgt_rows(rank, 0, n_local)
    fields = synth.vector_field(pa)[:ncomp]
    t_nodes = torch.from_numpy(pa).to(dev)
    t_conn = torch.from_numpy(ca).to(dev)
    t_pts = torch.from_numpy(pb).to(dev)
    t_fields = torch.from_numpy(fields).to(dev)

    from multimesh_amd.device import Context

    stream = torch.cuda.current_stream().cuda_stream
    ctx = Context(dev_index, stream=stream)
    ctx.set_fp_mode(args.fp_mode)
    COUNTER_KEY["locate_pass0"] = "locate_pass_kernel" if args.fp_mode == counter_profile_mode() or counter_profile_mode() is None else "locate_pass_kernel_exact"
    KERNEL_OF_STAGE["locate_pass0"] = LOCATE_KERNEL[args.fp_mode]
    BOUND_OF_STAGE["locate_pass0"] = LOCATE_BOUND[args.fp_mode]
    # Stage timers cost the stream two events per stage (~5 us each between kernels, ~40 us per step for all seven):
    # during the timed steps only the two dominant kernels are timed (the roofline's durations, live, over the
    # timed region); the other stages' table comes from STAGE_TABLE_STEPS extra, untimed steps after it.
    ctx.set_profiling(2)

    def make_run(points, n_loc, blk):
        """step / drain closures of one measurement over `points` (this rank's targets) with blocks of `blk`
        rows in the all-gather.  Two sets of output buffers: with more than one rank the all-gather of step s
        runs on RCCL's own stream while step s+1 computes into the other set."""
        nbuf = 2 if use_dist else 1
        st = {"outs": [torch.zeros((blk, ncomp), dtype=torch.float64, device=dev) for _ in range(nbuf)],
              "alls": [torch.empty((world * blk, ncomp), dtype=torch.float64, device=dev) if use_dist else None
                       for _ in range(nbuf)],
              "pending": [None] * nbuf, "n": 0, "stage_ms": {s: 0.0 for s in STAGES}, "nfailed": 0, "last": 0}

        def step(record):
            b = st["n"] % nbuf
            st["n"] += 1
            st["last"] = b
            if st["pending"][b] is not None:
                st["pending"][b].wait()          # the gather that last read this buffer set (two steps ago)
                st["pending"][b] = None
            _, nf = ctx.interpolate_hex8(t_nodes, t_conn, points, t_fields, nelem_to_search=k, out=st["outs"][b][:n_loc])
            if use_dist:
                # asynchronous: the gather overlaps the next step's kernels
                st["pending"][b] = D.all_gather(st["alls"][b], st["outs"][b], async_op=True)
            if record:
                st["nfailed"] += nf
                for s, v in ctx.last_timings().items():
                    st["stage_ms"][s] += v

        def drain():
            for b in range(nbuf):
                if st["pending"][b] is not None:
                    st["pending"][b].wait()
                    st["pending"][b] = None

        return st, step, drain

    st, step, drain = make_run(t_pts, n_local, chunk)
    elapsed = timed_steps(args, torch, D, step, drain)
    stage_ms = st["stage_ms"]
    nfailed_total = D.all_sum_int(st["nfailed"])
    t_out, t_all = st["outs"][st["last"]], st["alls"][st["last"]]
    locate_stats = ctx.last_locate_stats()      # of the last step: solves MM_FP_TOL repeated in the reference's arithmetic
    if args.dump_outputs and rank == 0:
        # the field the caller receives: this rank's rows, or with a collective every rank's rows gathered
        values = (torch.cat([t_all[r * chunk:r * chunk + n_rows[r]] for r in range(world)]) if use_dist
                  else t_out[:n_local])
        dump_outputs(args.dump_outputs, torch, values, {"nfailed": nfailed_total})
        del values
    if args.full:
        ctx.set_profiling(True)
        table = {s: 0.0 for s in STAGES}
        for _ in range(STAGE_TABLE_STEPS):
            step(False)
            for s, v in ctx.last_timings().items():
                table[s] += v
        drain()
        ctx.set_profiling(2)
        for s in STAGES:
            if s not in SINGLE_KERNEL_STAGES_TIMED_LIVE:
                stage_ms[s] = table[s] / STAGE_TABLE_STEPS * max(args.steps, 1)
    # the other arithmetic beside it (a few untimed-region steps on the same inputs): what the mode buys
    other_mode = None
    if args.full and rank == 0 and not as_rank:
        other = "exact" if args.fp_mode == "tol" else "tol"
        ctx.set_fp_mode(other)
        o_out = torch.zeros((chunk, ncomp), dtype=torch.float64, device=dev)
        for _ in range(2):
            ctx.interpolate_hex8(t_nodes, t_conn, t_pts, t_fields, nelem_to_search=k, out=o_out[:n_local])
        torch.cuda.synchronize()
        o_ms, o_pass = 0.0, 0.0
        o_steps = 5
        t0 = time.perf_counter()
        for _ in range(o_steps):
            ctx.interpolate_hex8(t_nodes, t_conn, t_pts, t_fields, nelem_to_search=k, out=o_out[:n_local])
            o_pass += ctx.last_timings()["locate_pass0"]
        torch.cuda.synchronize()
        o_ms = (time.perf_counter() - t0) / o_steps * 1e3
        diff = float((o_out[:n_local] - t_out[:n_local]).abs().max().item()) if n_local else 0.0
        other_mode = {"mode": other, "ms_per_step": round(o_ms, 4), "locate_pass0_ms": round(o_pass / o_steps, 4),
                      "kernel": LOCATE_KERNEL[other], "steps": o_steps,
                      "max_abs_difference_of_the_interpolated_values": diff,
                      "note": "the same step in the other arithmetic of mm_set_fp_mode, wall clock over a few steps after the "
                              "timed region (single rank, no collective)"}
        ctx.set_fp_mode(args.fp_mode)
        del o_out
    # ... and the same step with the source mesh kept resident (mm_source_create: centroids + search grid built once,
    # the reference's "one cKDTree, many queries", scripts/cli.py:141-195).  NOT `value`: the metric's step rebuilds.
    resident_source = None
    if args.full and rank == 0 and not as_rank:
        src = ctx.source(t_nodes, t_conn)
        r_out = torch.zeros((chunk, ncomp), dtype=torch.float64, device=dev)
        for _ in range(2):
            src.interpolate(t_pts, t_fields, nelem_to_search=k, out=r_out[:n_local])
        torch.cuda.synchronize()
        r_steps = 5
        t0 = time.perf_counter()
        for _ in range(r_steps):
            src.interpolate(t_pts, t_fields, nelem_to_search=k, out=r_out[:n_local])
        torch.cuda.synchronize()
        r_ms = (time.perf_counter() - t0) / r_steps * 1e3
        resident_source = {"ms_per_call": round(r_ms, 4), "points_per_s": n_local / (r_ms * 1e-3), "calls": r_steps,
                           "equals_the_rebuilding_step": bool(torch.equal(r_out[:n_local], t_out[:n_local])),
                           "note": "mm_interpolate_hex8_on over a source made resident once by mm_source_create (kNN query + "
                                   "locate + gather per call); never `value`"}
        src.free()
        del r_out

    # ---- the collective by itself: a BLOCKING all-gather, timed on the stream; then the WHOLE gathered field
    # against what one rank computes alone ----
    allgather = None
    if args.full and use_dist:
        ms = []
        for _ in range(3):
            torch.cuda.synchronize()
            D.barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            D.all_gather(t_all, t_out)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ag_ms = D.all_max(sorted(ms)[1])
        nbytes_in = (world - 1) * chunk * ncomp * 8
        allgather = {"backend": D.backend, "ms": round(ag_ms, 4), "bytes_received_per_gpu": nbytes_in,
                     "GBps_per_gpu": round(nbytes_in / (ag_ms * 1e-3) / 1e9, 1) if ag_ms > 0 and nbytes_in else None,
                     "note": "median of 3 blocking all_gather_into_tensor calls (max over ranks); in the timed steps "
                             "the gather is asynchronous and overlaps the next step's kernels"}
        if rank == 0:
            # rank 0 re-interpolates EVERY rank's block on its own GPU, alone, and compares the gathered rows bit
            # for bit (strong scaling: that is the 1-GPU result of the one target set, row for row)
            t0 = time.perf_counter()
            equal, rows = True, 0
            ref = torch.empty((min(VERIFY_CHUNK, max(n_rows)), ncomp), dtype=torch.float64, device=dev)
            for r in range(world):
                for a in range(0, n_rows[r], VERIFY_CHUNK):
                    b = min(a + VERIFY_CHUNK, n_rows[r])
                    pts_r = t_pts[a:b] if r == rank else torch.from_numpy(tgt_rows(r, a, b)).to(dev)
                    ctx.interpolate_hex8(t_nodes, t_conn, pts_r, t_fields, nelem_to_search=k, out=ref[:b - a])
                    equal = equal and bool(torch.equal(ref[:b - a], t_all[r * chunk + a:r * chunk + b]))
                    rows += b - a
                    del pts_r
            allgather["gathered_equals_single_rank"] = equal
            allgather["rows_compared"] = rows
            allgather["compare_s"] = round(time.perf_counter() - t0, 2)
            del ref
        D.barrier()

    # ---- strong scaling: the weak-scaling figure beside it (every rank a full target mesh of its own) ----
    weak = None
    if use_dist and scaling == "strong" and world > 1 and args.weak_beside:
        pw = torch.from_numpy(synth.hex_mesh_rows(n_tgt, 0, n_all, seed=7 + rank)).to(dev)
        wargs = argparse.Namespace(steps=min(args.steps, 5), warmup=min(args.warmup, 2))
        stw, stepw, drainw = make_run(pw, n_all, n_all)
        el = timed_steps(wargs, torch, D, stepw, drainw)
        weak = {"value": n_all * world * wargs.steps / el, "unit": "points/s", "ms_per_step": el / wargs.steps * 1e3,
                "steps": wargs.steps, "targets_per_gpu": n_all,
                "note": "every rank its own full target mesh (jitter seed 7 + rank), same collective"}
        del pw, stw, stepw, drainw

    rc = 0
    if rank == 0:
        steps = max(args.steps, 1)
        ms_per_step = elapsed / steps * 1e3
        value = total_targets * steps / elapsed
        n_elem, n_nodes = ca.shape[0], pa.shape[0]
        knn_kernel = os.environ.get("MM_KNN_KERNEL", "lane")
        line = {
            "metric": METRIC_OF_WORKLOAD.get(args.workload, METRIC_OF_WORKLOAD["metric"]),
            "value": value, "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "projection": ({"as_rank": f"{proj_rank}/{proj_world}",
                            "note": "NOT a scaling measurement: one process ran rank r's share of a G-rank strong-scaling step alone "
                                    "(no process group, no collective); tools/strong_projection.py"} if as_rank else None),
            "config": {"workload": f"{args.workload}: hex8 3D {n_nodes} source nodes -> {total_targets} targets in all, "
                                   f"{n_local} on rank 0 (n_src={n_src}, n_tgt={n_tgt} per side, jittered unit cube), "
                                   f"{ncomp} field component(s), k={k}; targets: " + target_desc,
                       "source_nodes": n_nodes, "source_elements": n_elem, "targets_per_gpu": n_local,
                       "targets_total": total_targets,
                       "candidate_lists": f"evaluated lazily: the {LAZY_K} nearest centroids up front, the full "
                                          f"k={k} list only for targets that exhaust them; every output is "
                                          "bit-identical to the eager evaluation (mm_set_lazy_lists(0))",
                       "knn_kernel": knn_kernel,
                       "parallelism": (f"{scaling} scaling: targets sharded x{world}, source replicated, 1 all-gather per "
                                       f"step over {D.backend} (asynchronous: overlaps the next step's kernels)")
                       if use_dist else "single GPU"},
            "nfailed": nfailed_total,
            "fp_mode": {"mode": args.fp_mode,
                        "tolerance": TOL_STATEMENT if args.fp_mode == "tol" else "0 ulp: every output bit-identical to the reference",
                        "solves_repeated_in_the_reference_arithmetic": locate_stats["redone_exact"],
                        "share_of_targets": round(locate_stats["redone_exact"] / max(n_local, 1), 5),
                        "targets_through_the_reference_order_kernel": locate_stats["reference_order"],
                        "other_mode": other_mode},
        }
        if weak:
            line["weak"] = weak
        if args.full:
            fused = stage_ms["gather"] == 0.0
            abytes = algorithmic_bytes(n_local, n_elem, n_nodes, k, ncomp)
            rbytes = actual_bytes(n_local, n_elem, n_nodes, k, ncomp, fused)
            stages = {}
            if fused:
                # values-only call: the weighted sum (A9) is formed inside the locate kernels at the
                # point of acceptance, so the locate stage carries the gather's algorithmic bytes too
                abytes["locate"] += abytes["gather"]
                abytes["locate_pass0"] += abytes["gather"]

            def account(ms, alg, act):
                gb_alg = alg / (ms * 1e-3) / 1e9
                gb_act = act / (ms * 1e-3) / 1e9
                d = {"ms": round(ms, 4), "algorithmic_bytes": alg, "actual_bytes": act,
                     "achieved_GBps": round(gb_alg, 1), "actual_GBps": round(gb_act, 1),
                     "frac_actual": round(gb_act / HBM_PEAK_GBPS, 4)}
                if gb_alg <= HBM_PEAK_GBPS:
                    d["frac"] = round(gb_alg / HBM_PEAK_GBPS, 4)
                else:
                    # SURVEY §8(d) prices re-reads that are L2 hits (a node's coordinates once per element,
                    # a field value once per target): not a fraction of HBM peak
                    d["frac"] = None
                    d["note"] = "section 8(d) bytes include L2-resident re-reads; see frac_actual"
                return d

            for s in STAGES:
                ms = stage_ms[s] / steps
                if ms == 0.0:
                    stages[s] = {"ms": 0.0, "fused_into": "locate"}
                    continue
                stages[s] = account(ms, abytes[s], rbytes[s])
            dominant = max(SINGLE_KERNEL_STAGES, key=lambda s: stage_ms[s])
            d = stages[dominant]
            roofline = {"bound": "hbm", "limited_by": BOUND_OF_STAGE[dominant],
                        "kernel": KERNEL_OF_STAGE[dominant] if (dominant != "knn_cell" or knn_kernel == "lane")
                        else f"knn_{knn_kernel}_kernel", "stage": dominant,
                        "achieved": d["achieved_GBps"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": d["frac"], "ms": d["ms"], "algorithmic_bytes": abytes[dominant],
                        "actual_bytes": rbytes[dominant], "frac_actual_bytes": d["frac_actual"],
                        "traffic": measured_traffic(dominant),
                        "timing": "hipEvents on the context's stream around this kernel's launches, averaged over the timed steps "
                                  "(only the two dominant kernels are timed there; the other stages' table comes from "
                                  f"{STAGE_TABLE_STEPS} extra steps after the timed region)",
                        "note": "priced against the HBM roofline as SURVEY 8(d) asks (`bound`); `limited_by` is what the "
                                "counters say actually limits the kernel -- for the kNN and locate kernels the vector-issue "
                                "rate, quantified in roofline_valu"}
            # VALU-issue floors: only for the launch the counter passes were taken on (the metric workload, one rank, the
            # mode the profile names) -- rescaled counts put "floors" above the measured time on other workloads
            roofline_valu = None
            counters_mode = counter_profile_mode()
            if args.workload == "metric" and world == 1 and not as_rank and n_local == 10_077_696:
                # (profiles since round 4 hold both instances of the locate pass: "locate_pass_kernel" = the profile's own
                # mode, "locate_pass_kernel_exact" the reference arithmetic beside it)
                have_locate = counters_mode == args.fp_mode or (counters_mode == "tol" and args.fp_mode == "exact")
                roofline_valu = {s: valu_floor(s, stages[s]["ms"]) for s in ("knn_cell", "locate_pass0")
                                 if stages[s].get("ms") and (s != "locate_pass0" or have_locate)}
                for v in roofline_valu.values():
                    if v and v.get("frac") and v["frac"] > 1.0:     # a floor above the measured time is not a floor
                        v["note"] = "counter profile does not match this build: " + v.get("note", "")
                        v["frac"] = None
            e2e_bytes = 952 + 72 * (ncomp - 1)          # 184 + 568 + 200 at C = 1, k = 20 (+72 per component)
            e2e_bytes += 8 * (k - 20) * 2
            replicated_ms = stages["centroid"]["ms"] + stages["knn_build"]["ms"]
            line.update({
                "roofline": roofline,
                "roofline_valu": roofline_valu if roofline_valu is not None else {
                    "omitted": "instruction-count floors are only printed for the launch the committed counter passes were taken on "
                               "(--workload metric, one rank)"},
                "roofline_memory_side": ({st: memory_side_profile(st, stages[st]["ms"]) for st in ("knn_cell", "locate_pass0")}
                                         if args.workload == "metric" and args.fp_mode == "tol" else None),
                "roofline_end_to_end": {"algorithmic_bytes_per_target": e2e_bytes,
                                        "achieved_GBps_per_gpu": round(e2e_bytes * n_local / (ms_per_step * 1e-3) / 1e9, 1),
                                        "frac": round(e2e_bytes * n_local / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)},
                "resident_source": resident_source,
                "replicated_per_rank": {"ms": round(replicated_ms, 4), "share_of_step": round(replicated_ms / ms_per_step, 4),
                                        "note": "centroids + search-grid build of the replicated source mesh run on every rank "
                                                "whatever its share of the targets: the Amdahl term of strong scaling "
                                                "(rank 0's stage timers)"},
                "stages": stages,
            })
            if allgather:
                line["allgather_ms"] = allgather["ms"]
                line["allgather"] = allgather
                if allgather.get("gathered_equals_single_rank") is False:
                    rc = 1
            roofline["measured_copy_GBps"] = round(hbm_copy_gbps(torch, dev), 1)

            # ---- stand-alone A9: the operator of THIS run re-applied to the field (the stored_array pattern) ----
            vals_op, enc, w, _ = ctx.interpolate_hex8(t_nodes, t_conn, t_pts, t_fields, nelem_to_search=k, want_operator=True)
            reps = max(args.steps, 5)
            g_out = ctx.gather(t_fields, enc, w)
            ctx.gather(t_fields, enc, w).free()
            g_ms = 0.0
            ctx.set_profiling(True)
            for _ in range(reps):
                o = ctx.gather(t_fields, enc, w)
                g_ms += ctx.last_timings()["gather"]
                o.free()
            ctx.set_profiling(2)
            g_ms /= reps
            ga = account(g_ms, n_local * (128 + 72 * ncomp), n_local * (128 + 8 * ncomp) + n_nodes * 8 * ncomp)
            ga["kernel"] = "gather8_kernel<true>"
            g_diff = float(np.abs(g_out.numpy() - t_out[:n_local].cpu().numpy()).max()) if n_local else 0.0
            # (MM_FP_TOL forms the fused sum as a chain of fused multiply-adds: equal to the gather kernel's NumPy-order sum to rounding)
            ga["equals_fused_values"] = bool(g_diff == 0.0) if args.fp_mode == "exact" else bool(g_diff <= 1e-12 * 8 * float(np.abs(fields).max()))
            ga["max_abs_diff_vs_fused_values"] = g_diff
            ga["traffic"] = measured_traffic("gather")
            ga["note"] = ("mm_gather on the (node ids, weights) rows of this run's targets: section 8(d) prices 64 B of gathered "
                          "field values per target and component, which are L2 hits (each node serves ~8 targets); actual_bytes "
                          "counts ids + weights + output + the field once")
            line["gather_reapply"] = ga
            stages["gather_reapply"] = ga
            del vals_op, enc, w, g_out

            if world == 1 and not as_rank:
                # PCIe-inclusive rate (never `value`): the same step fed from HOST arrays, i.e. what the
                # legacy host-pointer boundary costs: H2D of mesh + targets + field, D2H of the result
                out_h = np.zeros((n_local, ncomp))          # the reference's callers pass zero-initialised outputs (cli.py:77-78)
                ctx.interpolate_hex8_host(pa, ca, pb, fields, nelem_to_search=k, out=out_h)      # warm-up: device copies allocated
                t0 = time.perf_counter()
                vals_h, _ = ctx.interpolate_hex8_host(pa, ca, pb, fields, nelem_to_search=k, out=out_h)
                t_host = time.perf_counter() - t0
                nbytes = pa.nbytes + ca.nbytes + pb.nbytes + fields.nbytes + out_h.nbytes
                line["host_arrays"] = {"ms": t_host * 1e3, "points_per_s": n_local / t_host, "bytes_over_pcie": nbytes,
                                       "link_GBps_if_transfers_alone": round(nbytes / t_host / 1e9, 1),
                                       "equals_resident_run": bool(np.array_equal(vals_h, t_out[:n_local].cpu().numpy())),
                                       "note": "mm_interpolate_hex8_host: one step fed from pageable NumPy arrays (H2D on a second "
                                               "stream beside the kernels + D2H), device copies cached in the context; not `value`"}
                del vals_h
            if world == 1 and not args.no_cpu_baseline and not as_rank:
                stride = args.cpu_sample_stride or max(1, n_local // 2_500_000)   # ~12 s of single-threaded CPU work
                base, (stride, enc_c, w_c, vals_c) = cpu_baseline(pa, ca, pb, fields, k, stride)
                line["cpu_baseline"] = base
                line["speedup_vs_cpu_baseline"] = value / base["value"]
                # parity gate on the sample the CPU just computed: node ids exactly, always; values bit for
                # bit in MM_FP_EXACT, within the stated tolerance in MM_FP_TOL (weights too)
                got = t_out[:n_local].cpu().numpy()[::stride]
                _, enc_g, w_g, _ = ctx.interpolate_hex8(t_nodes, t_conn, t_pts, t_fields, nelem_to_search=k, want_operator=True)
                enc_s, w_s = enc_g.numpy()[::stride], w_g.numpy()[::stride]
                ids_equal = bool(np.array_equal(enc_s, enc_c))
                if args.fp_mode == "exact":
                    vals_ok = bool(np.array_equal(got, vals_c)) and bool(np.array_equal(w_s, w_c))
                else:
                    vals_ok = (float(np.abs(got - vals_c).max()) <= 1e-12 * 8 * float(np.abs(fields).max())
                               and float(np.abs(w_s - w_c).max()) <= 1e-12)
                line["parity_vs_cpu_sample"] = ids_equal and vals_ok
                line["parity_detail"] = {"node_ids_bit_equal": ids_equal, "values_within_stated_tolerance": vals_ok,
                                         "max_abs_value_diff": float(np.abs(got - vals_c).max()),
                                         "max_abs_weight_diff": float(np.abs(w_s - w_c).max()),
                                         "sample_points": int(len(got)), "mode": args.fp_mode}
                del enc_g, w_g
                if not line["parity_vs_cpu_sample"]:
                    rc = 1
        out.emit(json.dumps(line))

    ctx.close()
    if use_dist:
        D.barrier()
        dist.destroy_process_group()
    return rc


# ------------------------------------------------------------------------------------------
# cfg5: order-4 GLL hexes (reference components/interpolator.py:931-977)
# ------------------------------------------------------------------------------------------
def run_rank_gll(args, out, torch, dist, rank, world, dev_index, dev, D):
    """cfg5 under the same contract: a step = device np.unique of the element-nodal target points (A11) +
    the fused GLL path mm_interpolate_gll (centroids, grid, kNN, Newton location on the 125-node map, weighted
    sum) over this rank's share of the unique points (+ the all-gather)."""
    order, dim = 4, 3
    ne_src = (args.n_src or 44) - 1
    ne_tgt = (args.n_tgt or 48) - 1
    k = args.k
    ncomp = args.ncomp or 1
    P = (order + 1) ** dim
    scaling = "strong" if args.scaling in ("auto", "strong") else "weak"
    src = synth.gll_mesh(ne_src + 1, order, seed=1)                       # [E, 125, 3]
    tgt_en = synth.gll_mesh(ne_tgt + 1, order, seed=7).reshape(-1, dim)   # element-nodal target points
    fields = np.stack([f(src.reshape(-1, dim)).reshape(src.shape[:2])
                       for f in (synth.field_smooth, synth.field_linear, synth.field_xyz)][:ncomp])
    from multimesh_amd.device import Context

    stream = torch.cuda.current_stream().cuda_stream
    ctx = Context(dev_index, stream=stream)
    ctx.set_profiling(True)
    t_src = torch.from_numpy(src).to(dev)
    t_en = torch.from_numpy(tgt_en).to(dev)
    t_fields = torch.from_numpy(fields).to(dev)
    # the unique set once, to size the buffers (the timed steps recompute it into caller-owned buffers)
    d_u, d_inv = ctx.unique_points(t_en, ordered=False)
    t_ubuf = torch.empty(tgt_en.shape, dtype=torch.float64, device=dev)
    t_ibuf = torch.empty((tgt_en.shape[0],), dtype=torch.int64, device=dev)
    n_unique = d_u.shape[0]
    if scaling == "strong":
        lo, hi = shard_bounds(n_unique, world, rank)
        chunk = -(-n_unique // world)
        n_rows = [shard_bounds(n_unique, world, r)[1] - shard_bounds(n_unique, world, r)[0] for r in range(world)]
    else:
        lo, hi, chunk, n_rows = 0, n_unique, n_unique, [n_unique] * world
    n_local = hi - lo
    nbuf = 2 if D.use else 1
    outs = [torch.zeros((chunk, ncomp), dtype=torch.float64, device=dev) for _ in range(nbuf)]
    alls = [torch.empty((world * chunk, ncomp), dtype=torch.float64, device=dev) if D.use else None for _ in range(nbuf)]
    st = {"n": 0, "pending": [None] * nbuf, "unique_ms": 0.0, "stage_ms": {s: 0.0 for s in STAGES}, "missing": 0, "last": 0}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def step(record):
        b = st["n"] % nbuf
        st["n"] += 1
        st["last"] = b
        if st["pending"][b] is not None:
            st["pending"][b].wait()
            st["pending"][b] = None
        ev0.record()
        u, inv = ctx.unique_points(t_en, unique_out=t_ubuf, inverse_out=t_ibuf, ordered=False)   # A11 on the device (order-free form)
        ev1.record()
        _, miss = ctx.interpolate_gll(order, t_src, u.rows(lo, hi), t_fields, nelem_to_search=k, tolerance=1.05,
                                      out=outs[b][:n_local])
        if D.use:
            st["pending"][b] = D.all_gather(alls[b], outs[b], async_op=True)
        if record:
            st["missing"] += miss
            st["unique_ms"] += ev0.elapsed_time(ev1)
            for s, v in ctx.last_timings().items():
                st["stage_ms"][s] += v

    def drain():
        for b in range(nbuf):
            if st["pending"][b] is not None:
                st["pending"][b].wait()
                st["pending"][b] = None

    elapsed = timed_steps(args, torch, D, step, drain)
    missing = D.all_sum_int(st["missing"])
    t_out = outs[st["last"]]
    if args.dump_outputs and rank == 0:
        # values at the unique target points in their order of first occurrence (every rank's rows gathered with a collective)
        values = (torch.cat([alls[st["last"]][r * chunk:r * chunk + n_rows[r]] for r in range(world)]) if D.use
                  else t_out[:n_local])
        dump_outputs(args.dump_outputs, torch, values, {"nmissing": missing})
        del values
    allgather = None
    if args.full and D.use:
        t_all = alls[st["last"]]
        torch.cuda.synchronize()
        D.barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        D.all_gather(t_all, t_out)
        e1.record()
        e1.synchronize()
        allgather = {"backend": D.backend, "ms": round(D.all_max(e0.elapsed_time(e1)), 4)}
        if rank == 0:
            ref = torch.empty((max(n_rows), ncomp), dtype=torch.float64, device=dev)
            equal = True
            for r in range(world):
                a, b = shard_bounds(n_unique, world, r) if scaling == "strong" else (0, n_unique)
                ctx.interpolate_gll(order, t_src, d_u.rows(a, b), t_fields, nelem_to_search=k, tolerance=1.05, out=ref[:b - a])
                equal = equal and bool(torch.equal(ref[:b - a], t_all[r * chunk:r * chunk + b - a]))
            allgather["gathered_equals_single_rank"] = equal
            allgather["rows_compared"] = sum(n_rows)
        D.barrier()

    rc = 0
    if rank == 0:
        steps = max(args.steps, 1)
        ms_per_step = elapsed / steps * 1e3
        total = sum(n_rows) if world > 1 else n_local
        value = total * steps / elapsed
        sm = {s: v / steps for s, v in st["stage_ms"].items()}
        gb = gll_bytes(n_local, src.shape[0], P, dim, k, ncomp)
        loc_ms = sm["locate"]
        # the fused entry forms the weighted sum where a target is accepted: the locate stage carries the gather's bytes
        alg = gb["locate"] + gb["gather"]
        # what has to cross HBM at least once: every element's control nodes and nodal values once, per target its
        # coordinates, the candidate row (int32 inside the pipeline) and the values written
        n_src_elem = int(src.shape[0])
        act = n_src_elem * P * (dim * 8 + 8 * ncomp) + n_local * (dim * 8 + 4 * min(k, 8) + 8 * ncomp)
        frac_alg = alg / (loc_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS
        roofline = {"bound": "hbm", "limited_by": "valu (fp64 Newton on the 125-node map)",
                    "kernel": "locate_gll_first_pass_kernel<4, 3, int, true> + locate_gll_pass_kernel<4, 3, int, true> (all passes of the stage)",
                    "stage": "locate",
                    "achieved": round(alg / (loc_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    # (a section-8(d) figure above the peak is not a fraction of anything: the 3000 + 1000 B of control
                    # nodes and nodal values it prices per TARGET are staged once per element and shared by ~90 targets)
                    "frac": round(frac_alg, 4) if frac_alg <= 1.0 else None, "ms": round(loc_ms, 4),
                    "algorithmic_bytes": alg, "actual_bytes": act,
                    "frac_actual_bytes": round(act / (loc_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4), "traffic": None,
                    "note": "SURVEY 8(d) GLL bytes: locate 24 + 8k + 3000 + 8 + 1000 and gather 8 + 1000 + 1008 C per target "
                            "(`achieved`; above the HBM peak when the element data is reused from LDS / L2, then `frac` is null); "
                            "`actual_bytes` counts every array once; the stage is bound by fp64 vector issue and LDS latency "
                            "(roofline_valu), see DESIGN.md"}
        line = {
            "metric": "interpolated points/sec, order-4 GLL hex mesh (cfg5), 1 scalar field",
            "value": value, "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"cfg5: order-4 GLL hexes, {src.shape[0]} source elements ({ne_src}^3, {src.shape[0] * P} "
                                   f"element-nodal points) -> the {n_unique} unique GLL points of a {ne_tgt}^3-element target mesh "
                                   f"({tgt_en.shape[0]} element-nodal points), {ncomp} field component(s), k={k}, tolerance 1.05, "
                                   "snap_to_nearest off; a step = device np.unique of the target points + mm_interpolate_gll",
                       "parity": "UNPINNED: the reference's GLL numerics live in the absent salvus.fem; checked against this "
                                 "repository's own CPU restatement (oracle/mm_oracle.c) only",
                       "source_elements": int(src.shape[0]), "targets_per_gpu": n_local, "targets_total": total,
                       "parallelism": (f"{scaling} scaling: unique targets sharded x{world}, source replicated, 1 all-gather "
                                       f"per step over {D.backend}") if D.use else "single GPU"},
            "nmissing": missing,
            "roofline": roofline,
            # vector-issue floor of the Newton passes (instruction counts of profiles/*_gll_counters.json, collected on the
            # default cfg5 sizes with tools/knn_counters.sh; per launch, rescaled by this rank's share of the targets)
            "roofline_valu": {"locate": valu_floor("locate", loc_ms, scale=n_local / max(n_unique, 1), pattern="*_gll_counters.json",
                                                   key=["locate_gll_first_pass_kernel", "locate_gll_pass_kernel"], run_steps=3,
                                                   kernel="locate_gll_first_pass_kernel<4, 3, int, true> + locate_gll_pass_kernel<4, 3, int, true>")},
            "stages": {"unique_points": {"ms": round(st["unique_ms"] / steps, 4),
                                         "note": "mm_unique_points_any_order (hash table; the unique rows are only interpolated and scattered back) over all element-nodal target points (replicated on every rank)"},
                       **{s: {"ms": round(v, 4)} for s, v in sm.items() if v > 0}},
        }
        if allgather:
            line["allgather_ms"] = allgather["ms"]
            line["allgather"] = allgather
            if allgather.get("gathered_equals_single_rank") is False:
                rc = 1
        if args.full and world == 1 and not args.no_cpu_baseline:
            # the oracle's restatement of the same loop on a bounded sample ("port": salvus.fem is absent)
            from oracle import oracle as O
            from scipy.spatial import cKDTree

            stride = args.cpu_sample_stride or max(1, n_local // 2_400_000)   # ~10-15 s of single-threaded CPU work
            uniq = d_u.numpy()
            sample = np.ascontiguousarray(uniq[::stride])
            t0 = time.perf_counter()
            cen = src.mean(axis=1)
            tree = cKDTree(cen, balanced_tree=False)
            t_build = time.perf_counter() - t0
            t0 = time.perf_counter()
            _, nn = tree.query(sample, k=k)
            t_query = time.perf_counter() - t0
            t0 = time.perf_counter()
            elem_c, co_c, miss_c = O.locate_gll(order, nn, src, sample, 1.05, False)
            t_loc = time.perf_counter() - t0
            t0 = time.perf_counter()
            vals_c = O.gather_elem(fields, elem_c, co_c)
            t_g = time.perf_counter() - t0
            t_full = t_build + (t_query + t_loc + t_g) / len(sample) * n_local
            line["cpu_baseline"] = {"value": n_local / t_full, "unit": "points/s", "cores": 1, "kind": "port",
                                    "sample": (f"EXTRAPOLATED from every {stride}th unique target ({len(sample)} points: cKDTree query "
                                               f"{t_query:.2f}s, oracle mmo_locate_gll {t_loc:.2f}s, gather {t_g:.3f}s; tree build "
                                               f"{t_build:.2f}s); np.unique of the element-nodal points not included; the reference "
                                               "itself runs a Python loop around salvus.fem here and cannot be timed")}
            line["speedup_vs_cpu_baseline"] = value / line["cpu_baseline"]["value"]
            got = t_out[:n_local].cpu().numpy()[::stride]
            line["parity_vs_cpu_sample"] = bool(np.array_equal(got, vals_c))
            if not line["parity_vs_cpu_sample"]:
                rc = 1
        out.emit(json.dumps(line))
    ctx.close()
    if D.use:
        D.barrier()
        dist.destroy_process_group()
    return rc


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args, sys.argv[1:])
    with StdoutToStderr() as out:
        return run_rank(args, out)


if __name__ == "__main__":
    sys.exit(main())
