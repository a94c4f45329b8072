"""mm_idw_gather under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/scattered_cases.py bit for
bit (NaN positions compared, payloads not), counts exactly.

At the end of a mapping: the rows idx int64[N, k] and dist f64[N, k] (k = 1 and 5: 8 N k bytes end on a granule for even
N only; k = 8: read 16 bytes at a time), the fields f64[C, 5] (C odd: 40 C bytes end on no granule), the outputs.
A net under: the last entry of the last row in both row readers (k even: k / 2 pairs; k odd: k single entries); padded
entries (index nsrc, distance inf), whose field is never read; source nsrc - 1 of the last component, by an exact hit of
the last target and by weights; targets that max_distance leaves without a sample.

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
import scattered_cases as SC
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.scattered_cases():
    print(case["name"], flush=True)
    fields, idx, dist = case["fields"], case["idx"], case["dist"]
    for cut, power in ((np.inf, 2), (case["cut"], 3)):
        ref, ref_out, ref_near, ref_used = SC.idw(fields, idx, dist, G.NSRC, power=power, max_distance=cut, fill=-5.0)
        for point_major in (False, True):
            out, nout, near, used = ctx.idw_gather(fields, idx, dist, power=power, max_distance=cut, fill_value=-5.0,
                                                   point_major=point_major, want_nearest=True, want_count=True)
            got = out.numpy().T if point_major else out.numpy()
            assert nout == ref_out and SC.same_bits(got, ref), (case["name"], cut, point_major)
            assert SC.same_bits(near.numpy(), ref_near) and np.array_equal(used.numpy(), ref_used), (case["name"], cut)
print("ok")
"""


def test_scattered_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
