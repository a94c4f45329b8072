"""mm_region_distance under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array ends at the
end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A net, not a
provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/regions_cases.py bit for
bit, counts exactly.

At the end of a mapping: the points, the edge table, the signed distance and the flags, each sized to a granule, to neither and
to whole pages (tests/test_regions.py counts the classes without a GPU); the chunk records and the bits of ta, which are scratch
of the context and so allocations of their own under the guard.  The last edge of the last, partial chunk sets some node's
distance and some node's crossing: its row is the last of the table.

The switch is read once per process, so the checks run in a child process, as in tests/test_topography_guarded_gpu.py; the
child prints the name of every case before it runs it."""
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
import regions_cases as RC
from multimesh_amd import regions as RG
from multimesh_amd.device import Context

ctx = Context(0)
for case in RC.guarded_cases():
    print(case["name"], flush=True)
    args = (case["edges"], case["anchor"], case["anchor_inside"], case["cutoff"], case["scale"])
    s, inside, ni, nhit, ninvalid = RC.region_distance(case["points"], *args)
    for want_signed, want_inside in ((True, True), (True, False), (False, True)):
        res, n = RG.region_distance_call(ctx, case["points"], *args, want_signed=want_signed, want_inside=want_inside, want_info=True)
        assert n == ni and res["info"].numpy().tolist() == [nhit, ninvalid], case["name"]
        assert not want_signed or RC.same_bits(res["signed"].numpy().reshape(-1), s), case["name"]
        assert not want_inside or np.array_equal(res["inside"].numpy().reshape(-1), inside), case["name"]
print("ok")
"""


def test_regions_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
