"""mm_radial_stretch under GUARDED allocations (MM_GUARD_ALLOC=1, multimesh_amd/csrc/mm_context.hip): every array ends at the
end of its mapping with unmapped addresses behind it, so a read or write past an array would fault at once.  A net, not a
provocation: the inputs are ordinary, and the results are compared with the NumPy statement of tests/topography_cases.py,
evaluated on the angles the device returned (its acos and atan2 are the one part no statement pins), bit for bit (NaN positions
compared, payloads not), counts exactly.

At the end of a mapping: the points and the reference radii (8, 101 and 1024 nodes: a granule, neither, whole pages), the two
axes (6, 8 and 2 values: granules; 7, 9 and 13: not; 512: a page), the anchors (4: a granule; 5: not -- 64 anchors at the
most, never a page), shifts f64[nlat, nlon, na] in the three classes, the moved points, the radius and the coordinates.
A net under: lat[i + 1] / lon[j + 1] of a node in -- or, in clamp mode, clamped onto -- the last row and column (i is clipped
to n - 2 before the read), and of a node in the cell that closes a global axis; the corner column [ja1][io1] of the last map
node, whose last anchor's shift is the last double of the table, for a node below the bottom anchor; the anchors' last entry
for a node exactly on it.  Both directions, both lateral modes, keep and clamp, in place and out of place.
As in tests/test_topography_gpu.py the device's angles are held to NumPy's within 1e-11 degrees and r to NumPy's bits.

The inputs are those of tests/topography_cases.py (guarded_cases), whose edges tests/test_topography.py counts without a GPU.
The switch is read once per process, so the checks run in a child process, as in tests/test_layered_guarded_gpu.py; the child
prints the name of every case before it runs it."""
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
import topography_cases as TC
from multimesh_amd import topography as TP
from multimesh_amd.device import Context

ctx = Context(0)
for case in TC.guarded_cases():
    print(case["name"], flush=True)
    pts, lat, lon, anchors, shifts = (case[k] for k in ("points", "lat", "lon", "anchors", "shifts"))
    n = len(pts)
    ref_lld, r = TC.device_view(pts, lon, case["periodic"])
    for direction in ("apply", "flatten"):
        ref = case["ref"] if direction == "apply" else None
        for lateral in ("cell", "bilinear"):
            for outside in ("keep", "clamp"):
                for in_place in (False, True):
                    dev = ctx.to_device(pts)
                    count = ctx.to_device(np.array([3], dtype=np.int64))
                    res = TP.radial_stretch(ctx, dev, lat, lon, anchors, shifts, lon_periodic=case["periodic"], direction=direction,
                                            ref_radius=ref, lateral=lateral, outside=outside, out=dev if in_place else None,
                                            want_radius=True, want_latlondepth=True, noutside=count)
                    got = {k: a.numpy() for k, a in res.items()}
                    lld = got["latlondepth"]
                    dlon = np.abs(lld[:, 1] - ref_lld[:, 1])
                    assert max(np.abs(lld[:, 0] - ref_lld[:, 0]).max(), np.minimum(dlon, np.abs(dlon - 360.0)).max()) <= 1e-11, case["name"]
                    assert TC.same_bits_nan(lld[:, 2], TC.R_EARTH - r), case["name"]
                    want, radius, nout = TC.stretch(lld, r, pts, ref, lat, lon, anchors, shifts, getattr(TC, direction.upper()),
                                                    getattr(TC, lateral.upper()), getattr(TC, outside.upper()))
                    what = (case["name"], direction, lateral, outside, in_place)
                    assert TC.same_bits_nan(got["points"], want) and TC.same_bits_nan(got["radius"], radius), what
                    assert int(count.numpy()[0]) == 3 + nout, what
print("ok")
"""


def test_topography_under_guarded_allocations():
    env = dict(os.environ, MM_GUARD_ALLOC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHECKS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
