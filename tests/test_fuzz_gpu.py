"""A seeded slice of the four fuzzers (tests/fuzz_cases.py; tools/fuzz_*.py are its long runs) on the GPU.

Every test is one (fuzzer, route, seed) batch of fuzz_cases.SUITE_CORPUS at the "suite" sizes, its cases run in order on ONE
module-scoped Context: what survives between calls -- replayed sort positions, the one-pass build's confirmation, the
lane_hint verdict keyed on (npts, ncells), pooled scratch -- carries from case to case and from batch to batch, and the kNN
draws follow-up cases (the same counts, another distribution) to lean on it.  tests/test_fuzz_cases.py checks on the CPU
that these seeds draw every k, kind, dimension, margin, tolerance and flag of the tools' choice lists.

Routes: the kNN's default dispatch, MM_KNN_TREE=1 and MM_KNN_FORCE_LIST=1 in this process; MM_KNN_KERNEL=strip / lane in a
child process each (read once per process); the pipeline in MM_FP_EXACT and MM_FP_TOL, lists lazy or eager per case; one
child process under MM_GUARD_ALLOC=1 (the library's guard-page allocator), six cases per fuzzer.

test_every_reachable_knn_kernel_ran asserts that the kNN and pipeline batches together launched every kernel of
device.KNN_KERNELS the dispatch can reach at these sizes: lane, strip, cell, list, generic, levels, tree, one_pass and
target_replay -- all of them; none is out of reach under the suite's caps (levels: a 3-D graded or clustered cloud of
at least kLevelMinSources = 4096 sources, mm_knn_grid.inc.h, asked for k > 32, mm_knn.hip query_long_lists; tree:
MM_KNN_TREE=1, the same count, k <= kLaneMaxK = 20; one_pass and target_replay: check_pipeline's second call over the
mesh and targets of its first, mm_pipeline.hip may_guess).

A failure's message is the tool's case line and diagnosis, then the line that draws the case again:
fuzz_cases.cases(name, seed, case + 1, "suite").

Measured once on an MI355X, seconds per test, oracle included (the whole file: 27 tests in 6.5 s):
  test_knn_batch            default-124 0.49 (first use of the context; 0.24 more to set it up), default-127 0.10,
                            default-185 0.13, default-1 0.11, tree-181 0.07, tree-265 0.10, list-42 0.10
  test_pipeline_batch       exact-111 0.06, exact-112 0.29, exact-113 0.11, exact-114 0.09,
                            tol-121 0.16, tol-122 0.06, tol-123 0.20, tol-124 0.18
  test_gll_batch            0.13, 0.08, 0.12, 0.22        test_unique_batch  0.06, 0.05, 0.04, 0.04
  test_knn_batch_forced_kernel  strip 0.69, lane 0.83 (a child process each)
  test_short_corpus_under_guarded_allocations  1.14 (a child process)
  test_every_reachable_knn_kernel_ran  < 0.01 (the batches are run once per process)
Kernels the kNN and pipeline batches launched in that run: all nine of KNN_KERNELS.
"""
import os
import subprocess
import sys
import time

import pytest

import fuzz_cases as F
from multimesh_amd import device
from multimesh_amd.device import Context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_ENV = {"tree": {"MM_KNN_TREE": "1"}, "list": {"MM_KNN_FORCE_LIST": "1"}}
REACHABLE = ("lane", "strip", "cell", "list", "generic", "levels", "tree", "one_pass", "target_replay")


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


_RAN = {}


def _batch(ctx, name, route, seed, ncases):
    """One batch on the module's context, once per process -> the kNN kernels it launched."""
    key = (name, route, seed)
    if key not in _RAN:
        t0 = time.time()
        with pytest.MonkeyPatch.context() as mp:
            for var, value in ROUTE_ENV.get(route, {}).items():
                mp.setenv(var, value)
            if name == "pipeline":
                ctx.set_fp_mode(route)
            try:
                kernels, infos = F.run_batch(ctx, name, seed, ncases)
            finally:
                if name == "pipeline":
                    ctx.set_fp_mode("exact")
        _RAN[key] = kernels
        print(f"{name} {route} seed {seed}: {ncases} cases in {time.time() - t0:.2f} s; kNN kernels {sorted(kernels)}")
        for info in infos:
            print("  " + info["line"].replace("\n", "\n  "))
    return _RAN[key]


def _ids(name, routes):
    return [pytest.param(route, seed, n, id=f"{route}-{seed}") for route, seed, n in F.SUITE_CORPUS[name] if route in routes]


@pytest.mark.parametrize("route,seed,ncases", _ids("knn", ("default", "tree", "list")))
def test_knn_batch(ctx, route, seed, ncases):
    kernels = _batch(ctx, "knn", route, seed, ncases)
    if route == "tree":
        assert "tree" in kernels, sorted(kernels)
    if route == "list":
        assert kernels <= {"list", "generic", "levels"}, sorted(kernels)


@pytest.mark.parametrize("route,seed,ncases", _ids("pipeline", ("exact", "tol")))
def test_pipeline_batch(ctx, route, seed, ncases):
    _batch(ctx, "pipeline", route, seed, ncases)
    assert ctx.fp_mode() == "exact"


@pytest.mark.parametrize("route,seed,ncases", _ids("gll", ("default",)))
def test_gll_batch(ctx, route, seed, ncases):
    _batch(ctx, "gll", route, seed, ncases)


@pytest.mark.parametrize("route,seed,ncases", _ids("unique", ("default",)))
def test_unique_batch(ctx, route, seed, ncases):
    _batch(ctx, "unique", route, seed, ncases)


_CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import fuzz_cases as F
from multimesh_amd.device import Context
kernels = set()
with Context(0) as ctx:
    for name, seed, ncases in %r:
        kernels |= F.run_batch(ctx, name, seed, ncases)[0]
print("kernels:", ",".join(sorted(kernels)))
print("ok")
"""

_CHILD_KERNELS = {}


def _child(batches, env, timeout):
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), batches)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-3000:])
    return set(r.stdout.strip().splitlines()[-2].split(":", 1)[1].strip().split(","))


@pytest.mark.parametrize("kernel", ["strip", "lane"])
def test_knn_batch_forced_kernel(kernel):
    # MM_KNN_KERNEL is read once per process: a fresh child process per kernel
    batches = [("knn", seed, n) for seed, n in F.batches("knn", kernel)]
    kernels = _child(batches, dict(os.environ, MM_KNN_KERNEL=kernel), 120)
    _CHILD_KERNELS[kernel] = kernels
    assert kernel in kernels, sorted(kernels)
    if kernel == "strip":
        assert not kernels & {"lane", "cell"}, sorted(kernels)


def test_short_corpus_under_guarded_allocations():
    # started as tests/test_guarded_gpu.py starts its child: the switch is read once per process, and a fault, should
    # one come, stays out of the test runner's own GPU context
    batches = [(name, seed, n) for name in ("knn", "pipeline", "gll", "unique") for seed, n in F.batches(name, "guarded")]
    assert [n for _, _, n in batches] == [F.GUARDED_BATCH] * 4
    _child(batches, dict(os.environ, MM_GUARD_ALLOC="1"), 900)


def test_every_reachable_knn_kernel_ran(ctx):
    ran = set()
    for name, routes in (("knn", ("default", "tree", "list")), ("pipeline", ("exact", "tol"))):
        for route, seed, n in F.SUITE_CORPUS[name]:
            if route in routes:
                ran |= _batch(ctx, name, route, seed, n)
    print("kNN kernels launched by the kNN and pipeline batches:", sorted(ran))
    assert set(REACHABLE) <= set(device.KNN_KERNELS)
    assert ran >= set(REACHABLE), sorted(set(REACHABLE) - ran)
