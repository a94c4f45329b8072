"""Every device entry point on memory nobody has written, pre-filled with a set byte (MM_SCRATCH_FILL, csrc/mm_context.hip).

Every entry point lays its scratch out over what the previous call left in the context's pool, and the grow-only buffers
and ``mm_device_alloc`` hand out memory as the allocator gives it.  A fresh context's memory is zero in practice, and under
MM_GUARD_ALLOC every carve is a fresh mapping: a kernel that reads a count, a flag or a partial sum before the call wrote it
passes every other test.  Here each call runs twice on each of three contexts whose unwritten memory holds 0x00 (fresh
memory as it is today), 0x5A (a finite double near 1e125, a large positive int, a set flag) and 0xFF (NaN, -1, all bits):
the six results must be the same bits, counts included, and equal the CPU statement exactly as the case's own test compares
it.  No tolerance is introduced.  The cases and their inputs -- those of the existing tables -- are in scratch_fill_cases.py.

One child process per group, as in the guarded tests; the child prints each case before it runs it.  The positive controls
show that the switch fills (scratch, fresh allocations, guarded pieces), that it is off by default and that a bad value is
refused.  The first test needs no GPU: it keeps the sweep complete as entry points are added."""
import os
import subprocess
import sys

import pytest

import scratch_fill_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PRELUDE = 'import sys\nsys.path.insert(0, ".")\nsys.path.insert(0, "tests")\nimport scratch_fill_cases as S\n'


def _child(body, **env):
    full = {k: v for k, v in os.environ.items() if k not in ("MM_SCRATCH_FILL", "MM_GUARD_ALLOC")}
    full.update(env)
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body], cwd=ROOT, env=full, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------------- without a GPU
def test_every_entry_point_is_swept_or_excluded_with_a_reason():
    declared = S.signature_tables()
    assert len(declared) >= 89 and {"mm_interpolate_hex8", "mm_region_distance", "mm_convert_kernels"} <= set(declared)
    swept = S.swept_symbols()
    assert not swept - set(declared), sorted(swept - set(declared))                  # (no case names a symbol that is gone)
    assert not set(S.EXCLUDED) - set(declared), sorted(set(S.EXCLUDED) - set(declared))
    assert not swept & set(S.EXCLUDED), sorted(swept & set(S.EXCLUDED))
    assert all(reason.strip() for reason in S.EXCLUDED.values())
    missing = sorted(set(declared) - swept - set(S.EXCLUDED))
    assert not missing, f"no sweep case names {missing}: add one to scratch_fill_cases.GROUPS (or an exclusion with its reason)"


def test_the_completeness_check_sees_a_case_that_is_taken_out():
    declared = set(S.signature_tables())
    for group, case in (("streaming_tools", "order_statistics"), ("earth_models", "regions"), ("hex8_search", "interpolate_hex8_host")):
        groups = {g: {c: s for c, s in cases.items() if (g, c) != (group, case)} for g, cases in S.GROUPS.items()}
        assert declared - S.swept_symbols(groups) - set(S.EXCLUDED) == set(S.GROUPS[group][case]), (group, case)


def test_every_case_of_the_two_tables_is_in_a_group():
    """by name, from the tables' sources: importing them would import the oracle"""
    import re

    for path, table in (("test_caller_stream_gpu.py", "CASES"), ("test_caller_views_gpu.py", "OWN_CASES")):
        text = open(os.path.join(ROOT, "tests", path)).read()
        body = text[text.index(f"\n{table} = {{"):]
        names = re.findall(r'^    "(\w+)":', body[:body.index("\n}")], flags=re.M)
        assert len(names) >= 18
        grouped = {c for g, cases in S.GROUPS.items() if g != "pool_reuse" for c in cases}
        assert set(names) <= grouped, sorted(set(names) - grouped)


# ------------------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.gpu
@pytest.mark.parametrize("group", list(S.GROUPS))
def test_results_do_not_depend_on_what_unwritten_memory_holds(group):
    _child(f"S.run_group({group!r})\n")


# ------------------------------------------------------------------------------------------------- the positive controls
_CONTROLS = r"""
import ctypes as C
import numpy as np
from multimesh_amd import synth
from multimesh_amd.device import Context

print("fresh allocations hold the fill", flush=True)
ctx = S.context_with_fill("0x5A")
assert S.debug_scratch(ctx)[0] == 0x5A
for n in (1, 15, 16, 4099):
    a = ctx.empty(n, np.uint8)
    assert (a.numpy() == 0x5A).all(), n
assert S.debug_scratch(ctx)[3] >= 4

print("the reservation's last 4096 bytes hold the fill", flush=True)
pts = np.ascontiguousarray(synth.gll_mesh(4, 2, seed=3).reshape(-1, 3))     # a few hundred points, shared faces repeat
before = S.debug_scratch(ctx)[3]
uniq, inv = ctx.unique_points(pts)
assert np.array_equal(uniq.numpy(), np.unique(pts, axis=0)) and len(uniq.numpy()) < len(pts) < 1000
fill, base, reserved, fills = S.debug_scratch(ctx)
assert fill == 0x5A and base != 0 and reserved >= 4096 + 256 and reserved % 256 == 0 and fills > before
tail = np.zeros(4096, dtype=np.uint8)
ctx.lib.mm_copy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
assert ctx.lib.mm_copy_d2h(ctx.handle, tail.ctypes.data, base + reserved - 4096, 4096) == 0
assert (tail == 0x5A).all(), np.unique(tail)
ctx.close()

print("off by default", flush=True)
from test_caller_stream_gpu import _hex8
d = _hex8()
ctx = S.context_with_fill(None)
vals, enc, w, nf = ctx.interpolate_hex8(d.pa, d.ca, d.pb, d.fields, nelem_to_search=20, want_operator=True)
assert nf == d.nf and np.array_equal(vals.numpy(), d.vals)
fill, base, reserved, fills = S.debug_scratch(ctx)
assert fill == -1 and fills == 0 and base != 0 and reserved > 4096
ctx.close()
ctx = S.context_with_fill("")                                                # (empty: off)
assert S.debug_scratch(ctx)[0] == -1
ctx.close()

print("a value that is no byte is refused", flush=True)
for bad in ("zz", "256", "-1", "0x", "0x100", "5a", " 7", "0x5A "):
    try:
        S.context_with_fill(bad)
    except Exception as exc:
        assert "MM_SCRATCH_FILL" in str(exc) and "code -1" in str(exc), (bad, exc)
    else:
        raise AssertionError(f"MM_SCRATCH_FILL={bad!r} was accepted")
for good, byte in (("0", 0), ("255", 255), ("0xff", 255), ("0X5a", 0x5A), ("90", 90)):
    ctx = S.context_with_fill(good)
    assert S.debug_scratch(ctx)[0] == byte, good
    ctx.close()
print("ok")
"""

_GUARDED = r"""
import numpy as np
print("unique_points", flush=True)
ctx = S.context_with_fill("0xFF")
run, check = S.case_of("streaming_tools", "unique_points_ordered")
check(run(ctx))
fill, base, reserved, fills = S.debug_scratch(ctx)
assert fill == 0xFF and reserved == 0 and fills > 0, (fill, reserved, fills)
print("order_statistics", flush=True)
run, check = S.case_of("streaming_tools", "order_statistics")
check(run(ctx))
assert S.debug_scratch(ctx)[3] > fills
ctx.close()
print("ok")
"""


@pytest.mark.gpu
def test_the_switch_fills_is_off_by_default_and_refuses_what_is_no_byte():
    _child(_CONTROLS)


@pytest.mark.gpu
def test_guarded_pieces_are_filled_one_by_one():
    _child(_GUARDED, MM_GUARD_ALLOC="1")
