"""The operator transpose under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): the handle's
sorted weights, target indices, row offsets and long-row list, the sort's buffers and every array the Python layer makes
end at the end of their mapping with unmapped addresses behind them, so a read past a sorted array would fault at once.
A net, not a provocation: the inputs are ordinary operators -- node and element form, short and long rows, and sizes whose
arrays fill their last 16-byte granule exactly (the 4-byte target indices and offsets: counts that are multiples of 4;
whole pages: multiples of 128 * 4096) -- and the results are compared with NumPy bit for bit.

The switch is read once per process, so the checks run in a child process, as in tests/test_guarded_gpu.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_CHECKS = r"""
import sys
import numpy as np
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import transpose_cases as T
from multimesh_amd.device import Context

ctx = Context(0)
rng = np.random.default_rng(4242)

# node form: short rows; the contribution count N * P and the node count + 1 end a granule or a page
for n, P, nsrc in [(4096, 8, 4095), (1 << 16, 8, (1 << 16) - 1), (3001, 1, 511), (777, 27, 1023), (512, 128, 2047)]:
    ids = rng.integers(0, nsrc, size=(n, P))
    w = T.wide(rng, (n, P))
    op = ctx.transpose_nodes(ids, w, nsrc)
    for ncomp in (1, 3):
        v = T.wide(rng, (n, ncomp))
        assert T.same_bits(op.apply(v).numpy(), T.transpose_nodes(ids, w, v, nsrc)), ("nodes", n, P, nsrc, ncomp)
    op.free()
# node form: long rows (the wave kernel), whole and broken steps of 64 at the END of the sorted arrays
for name in ("straddle_sorted", "straddle_reverse_sorted", "straddle_unsorted", "skewed"):
    ids, w, nsrc = T.node_case(name)
    op = ctx.transpose_nodes(ids, w, nsrc)
    v = T.case_values(name, len(ids), 2)
    assert T.same_bits(op.apply(v).numpy(), T.transpose_nodes(ids, w, v, nsrc)), name
    assert T.same_bits(op.apply(np.ascontiguousarray(v.T), point_major=False).numpy(), T.transpose_nodes(ids, w, v, nsrc)), name
    op.free()
for length in (33, 64, 129, 192, 4096, 65536):      # one long row that IS the whole operator: its last step ends the arrays
    ids = np.zeros((length, 1), np.int64)
    w = T.wide(rng, (length, 1))
    v = T.wide(rng, (length, 1))
    op = ctx.transpose_nodes(ids, w, 3)
    assert T.same_bits(op.apply(v).numpy(), T.transpose_nodes(ids, w, v, 3)), ("long", length)
    op.free()
# element form: every group width, two nodes per lane (P = 125), targets outside, counts that end a granule
for n, P, nelem in [(4096, 4, 255), (4096, 8, 63), (2048, 9, 127), (1024, 25, 31), (4096, 27, 511), (1024, 64, 15), (1000, 125, 63)]:
    elem = rng.integers(-1, nelem, size=n)
    co = T.wide(rng, (n, P))
    op = ctx.transpose_elem(elem, co, nelem)
    for ncomp in (1, 4):
        v = T.wide(rng, (n, ncomp))
        assert T.same_bits(op.apply(v).numpy(), T.transpose_elem(elem, co, v, nelem)), ("elem", n, P, nelem, ncomp)
    op.free()
elem, co, nelem = T.elem_case("elem_straddle")
v = T.case_values("elem_straddle", len(elem), 3)
op = ctx.transpose_elem(elem, co, nelem)
assert T.same_bits(op.apply(v).numpy(), T.transpose_elem(elem, co, v, nelem)), "elem_straddle"
op.free()
elem = np.zeros(8192, np.int64)              # one element holds every target
co = T.wide(rng, (8192, 27))
v = T.wide(rng, (8192, 1))
op = ctx.transpose_elem(elem, co, 2)
assert T.same_bits(op.apply(v).numpy(), T.transpose_elem(elem, co, v, 2)), "one element"
op.free()
# empty operators
op = ctx.transpose_nodes(np.zeros((0, 8), np.int64), np.zeros((0, 8)), 64)
assert not op.apply(np.zeros((0, 1))).numpy().any()
op.free()
print("ok")
"""


def test_transpose_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
