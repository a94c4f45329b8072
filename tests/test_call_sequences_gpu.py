"""Fused hex8 calls whose settings change on a warm context, every call against the oracle.

A context that has served a fused call holds a guessed grid, that grid's per-cell counts, the call's target sort
(mm_context::target_replay with MM_BUF_TPOS / _TSTART / _LANE_ITEMS), the lane probe's verdict, device copies of host
arrays and the miss counter.  tests/test_replay_sort_gpu.py and tests/test_grid_guess_gpu.py vary the geometry under one
set of settings and compare with a fresh context; here the SETTINGS of a call differ from those of the call that left
the state -- list length, lazy / eager lists, arithmetic, fields, operator, timers, entry point -- and every result is
compared with the oracle's (tests/sequence_cases.py; its CPU-side preconditions: tests/test_sequence_cases.py).  Which
path a call took is asserted from Context.last_knn_kernels() and the counters of mm_debug_grid_guess and
mm_debug_target_replay, so that the file cannot pass by a route that holds no state.

What keeps or replays a sort (mm_pipeline.hip run_stages, mm_knn.hip knn_query_typed): only a call with lazily evaluated
lists (lazy on and k > 8: the query is the 8-list and its rows go by sorted position).  k <= 8 and eager lists keep
nothing and leave the held sort as it is; the call after them replays a sort that is two calls old."""
import functools

import numpy as np
import pytest

import sequence_cases as Q
from multimesh_amd import synth
from oracle import oracle as O
from test_replay_sort_gpu import _state

pytestmark = pytest.mark.gpu

BASE = Q.BASE


class Session:
    """One context, and for the resident entry one Source over S made once."""

    def __init__(self, resident=False):
        from multimesh_amd.device import Context

        self.ctx = Context(0)
        self.src_handle = self.ctx.source(*Q.source("S")) if resident else None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.src_handle is not None:
            self.src_handle.free()
        self.ctx.close()


def run(ctx, src_handle, source, targets, s, arrays=None):
    """Applies the settings and calls the entry -> ((values, enc, w, nfailed) as NumPy, enc and w None without the
    operator; the kNN kernels of the call's last run; the counters after it).  arrays: the caller's own (nodes,
    connectivity, points, fields) in place of the scene's."""
    pa, ca, pts, f = arrays or (*Q.source(source), Q.targets(targets, source), Q.fields(s.fields, source))
    ctx.set_lazy_lists(s.lazy)
    ctx.set_fp_mode(s.fp)
    ctx.set_profiling(s.profiling)
    if s.entry == "device":
        out = ctx.interpolate_hex8(pa, ca, pts, f, nelem_to_search=s.k, want_operator=s.want_operator)
    elif s.entry == "host":
        out = ctx.interpolate_hex8_host(pa, ca, pts, f, nelem_to_search=s.k, want_operator=s.want_operator)
    else:
        assert source == "S"
        out = src_handle.interpolate(pts, f, nelem_to_search=s.k, want_operator=s.want_operator)
    kernels = ctx.last_knn_kernels()
    arrs = [a if isinstance(a, np.ndarray) else a.numpy() for a in out[:-1]]
    got = (arrs[0], arrs[1], arrs[2], out[-1]) if s.want_operator else (arrs[0], None, None, out[-1])
    return got, kernels, _state(ctx)


def call(sess, s, targets="T", source="S", arrays=None):
    """run, compared with the oracle -> (kernels, counters)."""
    got, kernels, state = run(sess.ctx, sess.src_handle, source, targets, s, arrays)
    Q.compare(got, Q.expected(source, targets, s), s, source)
    return kernels, state


def warm(sess, entry):
    """Two BASE calls on the entry: an ordinary one that records, then one that replays (and, with a mesh to process,
    is guessed and sorts the sources in one pass)."""
    s = BASE.but(entry=entry)
    kernels, state = call(sess, s)
    assert "target_replay" not in kernels and "lane" in kernels and "tree" not in kernels, kernels
    kernels, state = call(sess, s)
    assert ({"target_replay", "lane"} if entry == "resident" else {"target_replay", "one_pass", "lane"}) <= kernels, kernels
    assert (state["misses"], state["held"], state["replays"], state["records"]) == (0, 1, 1, 1), state
    assert state["guessed"] == (0 if entry == "resident" else 1), state
    return state


# ---- which path a call took, from the counters before and after it --------------------------------------------------
def replayed(before, kernels, after):
    return "target_replay" in kernels and after["misses"] == before["misses"] and \
        after["replays"] == before["replays"] + 1 and after["records"] == before["records"] and after["held"] == 1


def no_replay(before, kernels, after):
    return "target_replay" not in kernels and after["misses"] == before["misses"] and after["replays"] == before["replays"]


def kept_nothing(before, kernels, after):
    return no_replay(before, kernels, after) and after["records"] == before["records"] and after["held"] == 1


def recorded(before, kernels, after):
    return no_replay(before, kernels, after) and after["records"] == before["records"] + 1 and after["held"] == 1


def missed(before, kernels, after):
    """(the attempt that missed counts as a replay; the kernels are those of the call's last run, the ordinary one)"""
    return "target_replay" not in kernels and after["misses"] == before["misses"] + 1


def anything(before, kernels, after):
    return True


# change: (settings of the changed call, its targets, its source, its path, the path of BASE after it)
CHANGES = {
    **{f"k{k}": (dict(k=k), "T", "S", replayed, replayed) for k in (9, 21, 33, 64)},
    **{f"k{k}": (dict(k=k), "T", "S", kept_nothing, replayed) for k in (1, 8)},
    "eager_k20": (dict(lazy=False), "T", "S", kept_nothing, replayed),
    "eager_k21": (dict(lazy=False, k=21), "T", "S", no_replay, replayed),
    "eager_k33": (dict(lazy=False, k=33), "T", "S", no_replay, replayed),
    "fp_tol": (dict(fp="tol"), "T", "S", replayed, replayed),
    "three_components": (dict(fields="three"), "T", "S", replayed, replayed),
    "values_only": (dict(want_operator=False), "T", "S", replayed, replayed),
    "profiling_1": (dict(profiling=1), "T", "S", replayed, replayed),
    "profiling_2": (dict(profiling=2), "T", "S", replayed, replayed),
    "other_field_values": (dict(fields="other"), "T", "S", replayed, replayed),
    "T_fewer": (dict(), "T_fewer", "S", recorded, recorded),
    "T_nan": (dict(), "T_nan", "S", anything, anything),
    "T_swapped": (dict(), "T_swapped", "S", missed, missed),
    "T_moved": (dict(), "T_moved", "S", missed, missed),
    "S_shifted": (dict(), "T", "S_shifted", missed, missed),
    "S_small": (dict(), "T", "S_small", no_replay, anything),
}
CASES = [(name, entry) for name in CHANGES for entry in Q.ENTRIES if entry != "resident" or CHANGES[name][2] == "S"]


@pytest.mark.parametrize("change,entry", CASES)
def test_one_changed_setting_then_the_base_call(change, entry):
    settings, targets, source, changed_path, base_path = CHANGES[change]
    base = BASE.but(entry=entry)
    with Session(entry == "resident") as sess:
        before = warm(sess, entry)
        kernels, state = call(sess, base.but(**settings), targets, source)
        assert changed_path(before, kernels, state), (change, entry, sorted(kernels), before, state)
        if change == "eager_k20":
            assert "lane" in kernels, kernels
        if change == "profiling_1":
            t = sess.ctx.last_timings()
            assert t["knn_query"] > 0 and t["locate"] > 0, t
        if change == "T_nan":
            assert state["misses"] <= 1, state
        if change == "S_small":
            assert state["guessed"] == before["guessed"], (before, state)
        if change == "S_shifted":
            assert state["guessed"] == before["guessed"] + 1, (before, state)
        before = state
        kernels, state = call(sess, base)
        assert base_path(before, kernels, state), (change, entry, sorted(kernels), before, state)
        if base_path is missed:
            assert state["misses"] == 2, state
        if change == "T_fewer":                       # T's sort was recorded anew: the call after that replays it
            before = state
            kernels, state = call(sess, base)
            assert replayed(before, kernels, state), (sorted(kernels), before, state)


def test_entries_share_one_context():
    """Device, host and resident calls on one context.  The host calls hand over the SAME NumPy buffers with their
    contents changed in place: a device copy cached by address would show as stale targets or values."""
    pa, ca = Q.source("S")
    bufs = [pa.copy(), ca.copy(), Q.targets("T").copy(), Q.fields("one").copy()]
    addresses = [b.ctypes.data for b in bufs]
    with Session(resident=True) as sess:
        warm(sess, "device")
        call(sess, BASE.but(entry="host"), arrays=bufs)
        call(sess, BASE.but(entry="resident"))
        call(sess, BASE, "T_swapped")
        bufs[2][:] = Q.targets("T_swapped")
        bufs[3][:] = Q.fields("other")
        call(sess, BASE.but(entry="host", fields="other"), "T_swapped", arrays=bufs)
        call(sess, BASE.but(entry="resident"))
        bufs[2][:] = Q.targets("T")
        bufs[3][:] = Q.fields("one")
        kernels, state = call(sess, BASE.but(entry="host"), arrays=bufs)
        assert [b.ctypes.data for b in bufs] == addresses
        assert state["misses"] <= 2, state


def test_host_entry_miss_is_rerun_from_the_device_copies():
    """A guess miss on the host entry: the second attempt runs without the host feed, on the device copies the first
    attempt uploaded."""
    host = BASE.but(entry="host")
    with Session() as sess:
        call(sess, host)
        kernels, state = call(sess, host)
        assert {"target_replay", "one_pass", "lane"} <= kernels and (state["misses"], state["guessed"]) == (0, 1), (kernels, state)
        kernels, state = call(sess, host, "T", "S_shifted")
        assert "one_pass" not in kernels and "target_replay" not in kernels, kernels
        assert (state["misses"], state["guessed"]) == (1, 2), state
        kernels, state = call(sess, host, "T", "S_shifted")
        assert {"target_replay", "one_pass"} <= kernels and (state["misses"], state["guessed"]) == (1, 3), (kernels, state)


def test_staged_calls_leave_the_kept_sort_alone():
    pa, ca = Q.source("S")
    pts = Q.targets("T")
    nn = Q.oracle_lists("S", "T")
    with Session() as sess:
        ctx = sess.ctx
        before = warm(sess, "device")
        cen = ctx.centroid(ca, pa)
        assert cen.numpy().tobytes() == O.centroid(ca, pa).tobytes()
        index = ctx.knn_build(cen)
        for k in (8, 20):
            assert np.array_equal(index.query(pts, k).numpy(), nn[:, :k]), k
        index.free()
        enc_o, w_o, nf_o, _ = Q.located("S", "T", 20)
        enc, w, nf = ctx.locate_hex8(np.ascontiguousarray(nn[:, :20]), synth.reorder_hex8(ca), pa, pts)
        assert nf == nf_o and enc.numpy().tobytes() == enc_o.tobytes() and w.numpy().tobytes() == w_o.tobytes()
        f = Q.fields("three")
        assert ctx.gather(f, enc_o, w_o).numpy().tobytes() == np.ascontiguousarray(O.gather(f, enc_o, w_o)).tobytes()
        kernels, state = call(sess, BASE)
        assert replayed(before, kernels, state), (sorted(kernels), before, state)


def _repeat(sess, n, targets, until_guessed=None):
    """BASE over `targets` n times (or until `guessed` reaches until_guessed): every eighth call against the oracle, the
    rest against the first by bytes.  -> the counters after each call."""
    states, first = [], None
    while len(states) < n and not (states and states[-1]["guessed"] == until_guessed):
        got, kernels, state = run(sess.ctx, None, "S", targets, BASE)
        if len(states) % 8 == 0:
            Q.compare(got, Q.expected("S", targets, BASE), BASE)
        first = first or got
        assert got[3] == first[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], first[:3])), len(states)
        states.append(state)
    return states


def test_sixty_four_confirmed_guesses_forgive_one_miss():
    """settle_guess: a guessed call that is confirmed takes one miss back when the context's count of guessed calls (the
    missed ones among them) is a multiple of 64.  A context with two misses guesses no more, so its count stands still
    and it is never forgiven."""
    with Session() as sess:
        warm(sess, "device")
        kernels, state = call(sess, BASE, "T_swapped")
        assert (state["misses"], state["guessed"]) == (1, 2), state
        states = _repeat(sess, 100, "T_swapped", until_guessed=64)
        assert [s["guessed"] for s in states] == list(range(3, 65))
        assert [s["misses"] for s in states] == [1] * 61 + [0], states[-2:]
        # two more misses are needed again to stop the guessing
        kernels, state = call(sess, BASE, "T")
        assert (state["misses"], state["guessed"]) == (1, 65), state
        kernels, state = call(sess, BASE, "T_swapped")
        assert (state["misses"], state["guessed"]) == (2, 66), state
        kernels, state = call(sess, BASE, "T")
        assert kernels.isdisjoint({"target_replay", "one_pass"}) and (state["misses"], state["guessed"]) == (2, 66), (kernels, state)
    with Session() as sess:
        warm(sess, "device")
        call(sess, BASE, "T_swapped")
        kernels, state = call(sess, BASE, "T")
        assert (state["misses"], state["guessed"]) == (2, 3), state
        states = _repeat(sess, 70, "T")
        assert all((s["misses"], s["guessed"], s["replays"]) == (2, 3, state["replays"]) for s in states), states[-1]


@functools.lru_cache(maxsize=None)
def walked(seed):
    """One walk of Q.walk behind warm(entry), every step against the oracle -> (misses at the end, steps that replayed)."""
    steps = Q.walk(seed)
    entry = steps[0][0].entry
    replays = 0
    with Session(entry == "resident") as sess:
        state = warm(sess, entry)
        for i, (s, targets) in enumerate(steps):
            before = state
            kernels, state = call(sess, s, targets)
            replays += replayed(before, kernels, state)
            if i and steps[i - 1] == (s, targets) and s.keeps_sort:
                assert replayed(before, kernels, state), (seed, i, s, targets, sorted(kernels), before, state)
    return state["misses"], replays


@pytest.mark.parametrize("seed", Q.WALK_SEEDS)
def test_random_walks(seed):
    misses, replays = walked(seed)
    print(f"walk {seed}: {replays} replays, {misses} miss")
    assert misses == 1


def test_random_walks_replay_often_enough():
    total = sum(walked(seed)[1] for seed in Q.WALK_SEEDS)
    print(f"{total} replays over {len(Q.WALK_SEEDS)} walks")
    assert total >= Q.WALK_MIN_REPLAYS
