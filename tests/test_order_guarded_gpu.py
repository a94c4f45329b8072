"""mm_gll_tensor_apply and mm_element_deviation under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/order_cases.py bit for
bit (NaN positions compared, payloads not), counts exactly.

At the end of a mapping: the values in the three layouts, scale_in f64[E, P_in], div_out f64[E, P_out], the 1-D table
f64[m_out][m_in] (6 to 10 doubles) and the outputs, at element counts of one tile minus one, one tile and one tile plus one.
A net under: the table's last row (m_out m_in doubles are loaded, by as many lanes); a partial last tile in every layout
-- layout 2's run of TILE * C items, whose last step holds fewer items than TILE -- plain and with the transposed table;
the prefetch of the next tile, which must not reach past the last element; scale_in / div_out of the last element; the
deviation kernel's last element and its node 0.

The inputs are those of tests/guarded_cases.py, whose edges tests/test_guarded_cases.py counts without a GPU.  The switch is
read once per process, so the checks run in a child process, as in tests/test_resolution_guarded_gpu.py; the child prints
the name of every case before it runs it."""
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
import guarded_cases as G
import order_cases as OC
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.order_cases():
    print(case["name"], flush=True)
    oi, oo, dim = case["order_in"], case["order_out"], case["dim"]
    for layout in (0, 1, 2):
        values = OC.from_planes(case["planes"], layout)
        for transpose in (False, True):
            R = OC.transposed_table(oi, oo) if transpose else OC.table(oi, oo)
            for scale, div in ((None, None), (case["scale_in"], case["div_out"])):
                want = OC.tensor_apply(R, dim, values, layout, scale, div)
                got = ctx.gll_tensor_apply(oi, oo, dim, values, layout=layout, transpose=transpose, scale_in=scale, div_out=div)
                assert got.numpy().tobytes() == want.tobytes(), (case["name"], layout, transpose, scale is None)
for case in G.deviation_cases():
    print("deviation", case["name"], flush=True)
    dev, edge = ctx.element_deviation(case["a"], case["b"])
    want_dev, want_edge = OC.element_deviation(case["a"], case["b"])
    assert dev.numpy().tobytes() == want_dev.tobytes() and edge.numpy().tobytes() == want_edge.tobytes(), case["name"]
print("ok")
"""


def test_order_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
