"""mm_layered_model_apply under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array
ends at the end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A
net, not a provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/layered_cases.py, evaluated on the (lat, lon, depth) the device
returned (its acos and atan2 are the one part no statement pins), bit for
bit (NaN positions compared, payloads not), counts exactly.

At the end of a mapping: the points, the two axes (6 and 8 values: granules; 7, 9 and 13: not), bounds
f64[nlat, nlon, 5] and values f64[nlat, nlon, 4, ncomp], the prefilled output, layer, span and the coordinates.
A net under: lat[i + 1] / lon[j + 1] of a node in -- or, in clamp mode, clamped onto -- the last row and column (i is
clipped to n - 2 before the read), and of a node in the cell that closes a global axis; the corner columns [ja1][io1] of
the last map node; bounds[nlayer] of the last interface for a depth equal to it and below it; the values of the last
layer of the last column; a pinched-out layer.  Both lateral modes, both picks, fill and clamp.
As in tests/test_layered_gpu.py the device's angles are held to NumPy's within 1e-11 degrees and its depth to NumPy's bits,
so a node cannot change sides of an edge by more than that without this test noticing.

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
import layered_cases as LC
from multimesh_amd import layered as LY
from multimesh_amd.device import Context

ctx = Context(0)
for case in G.layered_cases():
    print(case["name"], flush=True)
    pts, lat, lon, bounds, values = (case[k] for k in ("points", "lat", "lon", "bounds", "values"))
    n = pts.size // 3
    dp = LC.element_depth(pts) if pts.ndim == 3 else None
    for lateral in ("cell", "bilinear"):
        for pick in ("node", "element") if dp is not None else ("node",):
            for outside in ("fill", "clamp"):
                count = ctx.to_device(np.array([3], dtype=np.int64))
                res = LY.layered_model_apply(ctx, pts, lat, lon, bounds, values, lon_periodic=case["periodic"], lateral=lateral,
                                             pick=pick, outside=outside, fill_value=-1.5, want_layers=True, want_span=True,
                                             want_latlondepth=True, noutside=count)
                got = {k: a.numpy() for k, a in res.items()}
                lld, ref = got["latlondepth"].reshape(n, 3), LC.latlondepth(pts.reshape(n, 3))
                if case["periodic"]:
                    ref[:, 1] = LC.wrap(ref[:, 1], lon[0])
                dlon = np.abs(lld[:, 1] - ref[:, 1])
                assert max(np.abs(lld[:, 0] - ref[:, 0]).max(), np.minimum(dlon, np.abs(dlon - 360.0)).max()) <= 1e-11, case["name"]
                assert LC.same_bits_nan(lld[:, 2], ref[:, 2]), case["name"]
                want, layer, span, nout = LC.model_apply(got["latlondepth"].reshape(n, 3), dp, lat, lon, bounds, values,
                                                         getattr(LC, lateral.upper()), getattr(LC, pick.upper()),
                                                         getattr(LC, outside.upper()), -1.5)
                what = (case["name"], lateral, pick, outside)
                assert np.array_equal(got["layer"].reshape(n), layer), what
                assert LC.same_bits_nan(got["span"].reshape(n, 2), span) and LC.same_bits_nan(got["out"].reshape(want.shape), want), what
                assert int(count.numpy()[0]) == 3 + nout, what
print("ok")
"""


def test_layered_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
