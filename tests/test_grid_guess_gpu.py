"""The fused pipeline's guessed search grid (mm_interpolate_hex8: the grid laid out from the PREVIOUS call's bounding
box, checked against this call's own box at the end, the call run again on a miss): a guessed call, a call whose
guess was wrong, and a call with the guess switched off all return what a fresh context returns, bit for bit, and the
debug counters show which path ran.  Reference flow: scripts/cli.py:62-100 (one source mesh, many calls: :183-195)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from multimesh_amd import synth

pytestmark = pytest.mark.gpu


def _guess_state(ctx):
    out = (C.c_longlong * 4)()
    fn = ctx.lib.mm_debug_grid_guess
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    assert fn(ctx.handle, out) == 0
    return {"valid": out[0], "misses": out[1], "guessed": out[2], "nsrc": out[3]}


def _fresh(pa, ca, pb, fields):
    from multimesh_amd.device import Context

    c = Context(0)
    try:
        v, enc, w, nf = c.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=20, want_operator=True)
        assert _guess_state(c)["guessed"] == 0           # a context's first call has nothing to guess from
        return v.numpy(), enc.numpy(), w.numpy(), nf
    finally:
        c.close()


def test_guessed_call_hit_miss_and_recovery():
    from multimesh_amd.device import Context

    n = 30
    pa, ca = synth.hex_mesh(n, seed=1, jitter=0.3)
    pb = np.random.default_rng(5).uniform(0.02, 0.98, size=(40_000, 3))
    fields = synth.vector_field(pa)[:2]
    ref = _fresh(pa, ca, pb, fields)
    # the same element count in another place and size: the guess left by mesh A is wrong for it
    pa2 = pa * 1.5 + np.array([3.0, -1.0, 0.25])
    pb2 = pb * 1.5 + np.array([3.0, -1.0, 0.25])
    fields2 = synth.vector_field(pa2)[:2]
    ref2 = _fresh(pa2, ca, pb2, fields2)

    c = Context(0)
    try:
        def run(p, q, f):
            v, enc, w, nf = c.interpolate_hex8(p, ca, q, f, nelem_to_search=20, want_operator=True)
            return v.numpy(), enc.numpy(), w.numpy(), nf

        def same(a, b):
            return a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))

        assert same(run(pa, pb, fields), ref)
        s = _guess_state(c)
        assert s == {"valid": 1, "misses": 0, "guessed": 0, "nsrc": len(ca)}
        assert same(run(pa, pb, fields), ref)            # guessed, confirmed
        sub = run(pa, pb[::3].copy(), fields)            # guessed, confirmed: other targets, same source mesh
        assert sub[3] == 0 and all(np.array_equal(x, y[::3]) for x, y in zip(sub[:3], ref[:3]))
        s = _guess_state(c)
        assert s["guessed"] == 2 and s["misses"] == 0 and s["valid"] == 1
        assert same(run(pa2, pb2, fields2), ref2)        # guessed from mesh A's box: wrong, run again
        s = _guess_state(c)
        assert s["guessed"] == 3 and s["misses"] == 1 and s["valid"] == 1   # (the second run left mesh B's box)
        assert same(run(pa2, pb2, fields2), ref2)        # guessed from mesh B's box: right
        s = _guess_state(c)
        assert s["guessed"] == 4 and s["misses"] == 1
        assert same(run(pa, pb, fields), ref)            # second miss: this context stops guessing
        s = _guess_state(c)
        assert s["guessed"] == 5 and s["misses"] == 2
        assert same(run(pa, pb, fields), ref)
        assert _guess_state(c)["guessed"] == 5
    finally:
        c.close()


def test_values_only_and_host_entry_after_a_guess():
    from multimesh_amd.device import Context

    pa, ca = synth.hex_mesh(24, seed=2, jitter=0.25)
    pb, _ = synth.hex_mesh(31, seed=7, jitter=0.2)
    fields = synth.vector_field(pa)[:1]
    c = Context(0)
    try:
        v0, nf0 = c.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=20)
        v1, nf1 = c.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=20)
        out = c.interpolate_hex8_host(pa, ca, pb, fields, nelem_to_search=20)
        assert _guess_state(c)["guessed"] == 2 and _guess_state(c)["misses"] == 0
        assert nf0 == nf1 == out[-1]
        assert np.array_equal(v0.numpy(), v1.numpy()) and np.array_equal(v0.numpy(), np.asarray(out[0]))
    finally:
        c.close()


def test_switch_off():
    code = (
        "import numpy as np, ctypes as C\n"
        "from multimesh_amd import synth\n"
        "from multimesh_amd.device import Context\n"
        "pa, ca = synth.hex_mesh(16, seed=1, jitter=0.3)\n"
        "pb = np.random.default_rng(5).uniform(0.05, 0.95, size=(5000, 3))\n"
        "f = synth.vector_field(pa)[:1]\n"
        "c = Context(0)\n"
        "a = c.interpolate_hex8(pa, ca, pb, f)[0].numpy(); b = c.interpolate_hex8(pa, ca, pb, f)[0].numpy()\n"
        "out = (C.c_longlong * 4)(); c.lib.mm_debug_grid_guess.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]\n"
        "c.lib.mm_debug_grid_guess(c.handle, out)\n"
        "assert np.array_equal(a, b) and out[2] == 0, list(out)\n"
        "print('ok')\n"
    )
    env = dict(os.environ, MM_GRID_GUESS="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.timeout(300)
def test_a_miss_at_a_realistic_size_is_cheap():
    # ADVICE (round 3): a guessed grid from a mesh of the same element count in ANOTHER place clamps every source and
    # target into a few boundary cells; without a device-side check the ring searches then scan nearly all sources for
    # every target (1M x 1M here: minutes, and it looks like a hang) before the host notices.  bbox_final_kernel now
    # compares this call's box with the guess on the device and the ring-search and locate kernels return at once: the
    # miss costs one cheap extra pass.  1M -> 1M, the second mesh shifted and scaled; bit-equal to a fresh context and
    # within a few times the time of an ordinary call.
    import time

    from multimesh_amd.device import Context

    pa, ca = synth.hex_mesh(101, seed=1)
    pb, _ = synth.hex_mesh(101, seed=7)
    f = synth.vector_field(pa)[:1]
    pa2, pb2 = pa * 3.0 + 10.0, pb * 3.0 + 10.0
    f2 = synth.vector_field(pa2)[:1]
    c = Context(0)
    try:
        d = [c.to_device(x) for x in (pa, ca, pb, f, pa2, pb2, f2)]
        c.interpolate_hex8(d[0], d[1], d[2], d[3])                      # leaves mesh A's box as the guess
        c.interpolate_hex8(d[0], d[1], d[2], d[3])                      # a guessed call that is confirmed
        c.synchronize()
        t0 = time.perf_counter()
        c.interpolate_hex8(d[0], d[1], d[2], d[3])
        c.synchronize()
        t_hit = time.perf_counter() - t0
        before = _guess_state(c)
        t0 = time.perf_counter()
        v2, nf2 = c.interpolate_hex8(d[4], d[1], d[5], d[6])            # same element count, another box: a miss
        c.synchronize()
        t_miss = time.perf_counter() - t0
        after = _guess_state(c)
        assert after["misses"] == before["misses"] + 1 and after["guessed"] == before["guessed"] + 1
        assert t_miss < max(30 * t_hit, 0.5), (t_hit, t_miss)           # (an unguarded miss: tens of seconds)
        fresh = Context(0)
        try:
            v_ref, nf_ref = fresh.interpolate_hex8(pa2, ca, pb2, f2)
            assert nf2 == nf_ref == 0 and np.array_equal(v2.numpy(), v_ref.numpy())
        finally:
            fresh.close()
    finally:
        c.close()


def _small_case():
    """Mesh A (3375 elements, 5000 targets, four field components) and the same connectivity scaled and shifted."""
    pa, ca = synth.hex_mesh(16, seed=1, jitter=0.3)
    pb = np.random.default_rng(5).uniform(0.05, 0.95, size=(5000, 3))
    shift = np.array([3.0, -1.0, 0.25])
    pa2, pb2 = pa * 1.5 + shift, pb * 1.5 + shift

    def four(p):
        f = synth.vector_field(p)
        return np.ascontiguousarray(np.concatenate([f, -f[:1] * 0.5]))

    return (pa, ca, pb, four(pa)), (pa2, ca, pb2, four(pa2))


def _device_call(c, mesh, ncomp, want_operator):
    pa, ca, pb, f = mesh
    out = c.interpolate_hex8(pa, ca, pb, np.ascontiguousarray(f[:ncomp]), nelem_to_search=20, want_operator=want_operator)
    return [x.numpy() for x in out[:-1]] + [out[-1]]


def _fresh_call(mesh, ncomp, want_operator):
    from multimesh_amd.device import Context

    c = Context(0)
    try:
        return _device_call(c, mesh, ncomp, want_operator)
    finally:
        c.close()


def _same(a, b):
    return len(a) == len(b) and a[-1] == b[-1] and all(np.array_equal(x, y) for x, y in zip(a[:-1], b[:-1]))


@pytest.mark.parametrize("ncomp,want_operator", [(4, False), (1, True)])
def test_missed_guess_through_the_host_entry(ncomp, want_operator):
    # The call that is run again after a wrong guess gets no host feed (the device copies are in place).  Four components
    # without the operator: more than the locate kernels gather themselves (kFuseGatherMaxComp = 3), so the rows live in
    # the context's private buffers and the separate gather runs after the second attempt; one component with the
    # operator: the rows are the caller's.
    from multimesh_amd.device import Context

    mesh_a, mesh_b = _small_case()
    ref_a, ref_b = _fresh_call(mesh_a, ncomp, want_operator), _fresh_call(mesh_b, ncomp, want_operator)
    c = Context(0)
    try:
        def host(mesh):
            pa, ca, pb, f = mesh
            out = c.interpolate_hex8_host(pa, ca, pb, np.ascontiguousarray(f[:ncomp]), nelem_to_search=20,
                                          want_operator=want_operator)
            return [np.asarray(x) for x in out[:-1]] + [out[-1]]

        assert _same(host(mesh_a), ref_a)
        assert _guess_state(c) == {"valid": 1, "misses": 0, "guessed": 0, "nsrc": len(mesh_a[1])}
        assert _same(host(mesh_a), ref_a)                 # guessed, confirmed
        s = _guess_state(c)
        assert s["guessed"] == 1 and s["misses"] == 0 and s["valid"] == 1
        assert _same(host(mesh_b), ref_b)                 # guessed from mesh A's box: wrong, run again without the feed
        s = _guess_state(c)
        assert s["guessed"] == 2 and s["misses"] == 1 and s["valid"] == 1   # (the second run left mesh B's box)
    finally:
        c.close()


def test_resident_source_between_guessed_calls():
    # A call on a resident source neither guesses nor disturbs the guess the context holds: the call after it is guessed
    # like the one before it.
    from multimesh_amd.device import Context

    mesh_a, _ = _small_case()
    pa, ca, pb, f = mesh_a
    f1 = np.ascontiguousarray(f[:1])
    ref = _fresh_call(mesh_a, 1, True)
    c = Context(0)
    try:
        assert _same(_device_call(c, mesh_a, 1, True), ref)
        src = c.source(pa, ca)
        assert _same(_device_call(c, mesh_a, 1, True), ref)          # guessed, confirmed
        assert _guess_state(c) == {"valid": 1, "misses": 0, "guessed": 1, "nsrc": len(ca)}
        out = src.interpolate(pb, f1, nelem_to_search=20, want_operator=True)
        assert _same([x.numpy() for x in out[:-1]] + [out[-1]], ref)
        assert _guess_state(c) == {"valid": 1, "misses": 0, "guessed": 1, "nsrc": len(ca)}
        assert _same(_device_call(c, mesh_a, 1, True), ref)          # guessed, confirmed
        assert _guess_state(c) == {"valid": 1, "misses": 0, "guessed": 2, "nsrc": len(ca)}
        src.free()
    finally:
        c.close()
