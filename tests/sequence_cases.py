"""Scenes, call settings and the oracle's answers of the call-sequence tests (tests/test_call_sequences_gpu.py).

The fused hex8 entries (Context.interpolate_hex8, .interpolate_hex8_host, Source.interpolate) keep state from one call to
the next: the guessed grid, its per-cell counts, the previous call's target sort, the lane probe's verdict, device copies
of host arrays, the miss counter.  The tests drive one context through calls whose SETTINGS differ from the call that
left the state and compare every call with the oracle (oracle/oracle.py: cKDTree lists over the C restatement's centroids,
the C restatement of the reference's locate, its NumPy-order gather), never with the library itself.  Everything here is
plain NumPy; tests/test_sequence_cases.py checks on the CPU that the scenes are what the GPU tests need.

Scene S: a 24-node-per-side jittered mesh folded along x (x += 0.08 tri(6 y), a zig-zag of slope +-1.92: 12 167
elements), the nodes of a second mesh mapped the same way as targets (13 824) and 200 targets far outside (every one
fails).  A mesh sheared as a whole fills less than half of its bounding box, the grid statistic of the build
(mm_knn.hip stat_verdict) then asks for density levels and the pipeline takes the kNN tree, which keeps no state; the
folded mesh fills its box, passes the statistic (grid_statistic below) and takes the lane kernel over a single-level
grid, AND has targets that accept none of their first 8, 20 and 32 candidates, so that k = 9 .. 64 with lazy lists
fetch full lists on demand and k = 20, 33 and 64 give different answers.
"""
import dataclasses
import functools

import numpy as np

import dispatch_cases as D
import test_replay_sort_gpu as R          # the grid's arithmetic and the target constructions (not copied)
from multimesh_amd import synth
from oracle import oracle as O

N = 24
NFAR = 200
KS = (1, 8, 9, 20, 21, 33, 64)
ENTRIES = ("device", "resident", "host")
SHIFT = (1.5, np.array([3.0, -1.0, 0.25]))      # S_shifted = S * 1.5 + (3, -1, 0.25)
NAN_ROW = 1234
WALK_STEPS = 14
WALK_SEEDS = tuple(range(8))
WALK_MIN_REPLAYS = 24


@dataclasses.dataclass(frozen=True)
class Settings:
    """One call: the entry, the list length, lazy / eager lists, the locate stage's arithmetic, the fields ("one", "three"
    or "other": one component with other values), whether the operator is asked for, the stage timers (0, 1, 2)."""
    entry: str = "device"
    k: int = 20
    lazy: bool = True
    fp: str = "exact"
    fields: str = "one"
    want_operator: bool = True
    profiling: int = 0

    def but(self, **changes):
        return dataclasses.replace(self, **changes)

    @property
    def keeps_sort(self):
        """The call keeps (or replays) its target sort: only a lazily evaluated list (kq = 8 < k) sorts the rows."""
        return self.lazy and self.k > D.LAZY_K


BASE = Settings()


def _fold(p):
    """x += 0.08 tri(6 y), tri the triangle wave of period 1 and range [-1, 1]."""
    p = p.copy()
    t = 6.0 * p[:, 1]
    p[:, 0] += 0.08 * (2.0 * np.abs(2.0 * (t - np.floor(t + 0.5))) - 1.0)
    return p


def _moved_by(source, p):
    return np.ascontiguousarray(p * SHIFT[0] + SHIFT[1]) if source == "S_shifted" else p


@functools.lru_cache(maxsize=None)
def source(name):
    """(nodes, exodus connectivity) of S, S_shifted (same element count, another box) or S_small (another count)."""
    if name == "S_small":
        return synth.hex_mesh(20, seed=2)
    pa, ca = synth.hex_mesh(N, seed=1, jitter=0.3)
    return _moved_by(name, _fold(pa)), ca


@functools.lru_cache(maxsize=None)
def far_targets():
    """NFAR targets far outside every mesh here, as dispatch_cases.outside_mesh makes them (its rows beyond |x| = 1.5)."""
    pb = D.outside_mesh(NFAR)[2]
    far = pb[(np.abs(pb) > 1.5).all(axis=1)]
    assert len(far) == NFAR
    return far


def _replay_case(pts):
    """A case as tests/test_replay_sort_gpu.py's constructions take it, always on S's grid."""
    pa, ca = source("S")
    return pa, ca, np.ascontiguousarray(pts), None


@functools.lru_cache(maxsize=None)
def targets(name, src="S"):
    """T: the sheared target mesh's nodes and the far targets behind them.  T_swapped (two rows in different cells
    exchanged), T_moved (one target one cell further), T_permuted, T_fewer (the last five rows dropped), T_nan (one NaN
    row), T_fewer_swapped (T_fewer with two rows exchanged).  For S_shifted the targets are mapped as the mesh is."""
    if src == "S_shifted":
        return _moved_by(src, targets(name))
    if name == "T":
        pb, _ = synth.hex_mesh(N, seed=7, jitter=0.2)
        pts = np.concatenate([_fold(0.01 + 0.98 * pb), far_targets()])
    elif name == "T_fewer":
        pts = targets("T")[:-5]
    elif name == "T_nan":
        pts = targets("T").copy()
        pts[NAN_ROW] = np.nan
    else:
        base, change = {"T_swapped": ("T", R._swapped), "T_moved": ("T", R._moved), "T_permuted": ("T", R._permuted),
                        "T_fewer_swapped": ("T_fewer", R._swapped)}[name]
        pts = change(_replay_case(targets(base)))[2]
    pts = np.ascontiguousarray(pts)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def fields(name, src="S"):
    pa = source(src)[0]
    f = synth.vector_field(pa)
    return np.ascontiguousarray({"one": f[:1], "three": f[:3], "other": -2.0 * f[:1] + 1.0}[name])


def grid(src="S"):
    """(lo, dims, 1 / h) of the search grid over a source's centroids (R._grid restates grid_layout)."""
    return R._grid(*source(src))


def grid_statistic(src="S"):
    """(largest share of the sources in one band of level-0 cell counts, share of the sources in cells of at most 5): what
    mm_knn.hip's stat_verdict reads.  A band above 0.02 asks for a density level (and the fused pipeline then takes the
    tree), a sparse share above 0.25 for a coarser grid: either way the grid is not guessed and no sort is kept."""
    pa, ca = source(src)
    counts = np.bincount(cells(O.centroid(ca, pa), src), minlength=int(grid(src)[1].prod()))
    above = [counts[counts > c].sum() for c in (15, 19, 38, 77, 154, 307, 614, 1229)] + [0]
    return max(a - b for a, b in zip(above, above[1:])) / len(ca), counts[counts <= 5].sum() / len(ca)


def cells(pts, src="S"):
    return R._cells(pts, *grid(src))


# ---------------------------------------------------------------------------------------------------------- oracle
@functools.lru_cache(maxsize=None)
def oracle_lists(src, tgt):
    """cKDTree's 64 nearest centroids of every target.  A non-finite target is nearest to nothing: its row is given the
    first 64 elements, and the oracle's locate decides (no element accepts it)."""
    pa, ca = source(src)
    pts = targets(tgt, src)
    finite = np.isfinite(pts).all(axis=1)
    nn = np.tile(np.arange(D.KMAX, dtype=np.int64), (len(pts), 1))
    nn[finite] = O.knn_ckdtree(O.centroid(ca, pa), pts[finite], D.KMAX, workers=D.WORKERS)[0]
    return nn


@functools.lru_cache(maxsize=None)
def located(src, tgt, k):
    """(enc, w, nfailed, status) of the oracle's locate over the first k candidates."""
    pa, ca = source(src)
    enc, w, nf, status = O.locate_hex8(oracle_lists(src, tgt)[:, :k], synth.reorder_hex8(ca), pa, targets(tgt, src),
                                       want_status=True)
    assert nf == (status < 0).sum() and not enc[status < 0].any() and not w[status < 0].any()
    return enc, w, nf, status


@functools.lru_cache(maxsize=None)
def _expected(src, tgt, k, fname):
    enc, w, nf, status = located(src, tgt, k)
    vals = np.ascontiguousarray(O.gather(fields(fname, src), enc, w))
    assert not vals[status < 0].any()
    for a in (vals, enc, w):
        a.setflags(write=False)
    return vals, enc, w, nf


def expected(src, tgt, settings):
    """(values f64[N, C], enc int64[N, 8], w f64[N, 8], nfailed); rows of failed targets are zero in all three."""
    return _expected(src, tgt, settings.k, settings.fields)


def compare(got, want, settings, src="S"):
    """got = (values, enc, w, nfailed), enc and w None when the operator was not asked for.  exact: every byte; tol: ids
    and the failed count equal, weights within the header's bound (D.fp_tol), values within it times max|field|."""
    vals, enc, w, nf = got
    vals_o, enc_o, w_o, nf_o = want
    assert nf == nf_o, (settings, nf, nf_o)
    assert vals.shape == vals_o.shape and (enc is None) == (not settings.want_operator), settings
    if settings.want_operator:
        assert enc.tobytes() == enc_o.tobytes(), (settings, int((enc != enc_o).any(axis=1).sum()))
    if settings.fp == "exact":
        assert vals.tobytes() == vals_o.tobytes(), (settings, int((vals != vals_o).any(axis=1).sum()))
        if settings.want_operator:
            assert w.tobytes() == w_o.tobytes(), (settings, int((w != w_o).any(axis=1).sum()))
        return
    tol = D.fp_tol(*source(src))
    scale = np.abs(fields(settings.fields, src)).max()
    dv = np.abs(vals - vals_o).max()
    assert dv <= tol * scale, (settings, dv, tol * scale)
    if settings.want_operator:
        dw = np.abs(w - w_o).max()
        assert dw <= tol, (settings, dw, tol)


# ---------------------------------------------------------------------------------------------------------- walks
def _draw_change(rng, s, tgt):
    """One setting of the pool that never misses, changed to another value."""
    what = rng.choice(["k", "lazy", "fp", "fields", "operator", "profiling", "targets"])
    if what == "k":
        return s.but(k=int(rng.choice([k for k in KS if k != s.k]))), tgt
    if what == "lazy":
        return s.but(lazy=not s.lazy), tgt
    if what == "fp":
        return s.but(fp="tol" if s.fp == "exact" else "exact"), tgt
    if what == "fields":
        return s.but(fields=str(rng.choice([f for f in ("one", "three", "other") if f != s.fields]))), tgt
    if what == "operator":
        return s.but(want_operator=not s.want_operator), tgt
    if what == "profiling":
        return s.but(profiling=int(rng.choice([p for p in (0, 1, 2) if p != s.profiling]))), tgt
    if tgt in ("T", "T_fewer"):                  # (behind the swap the targets stay)
        tgt = "T_fewer" if tgt == "T" else "T"
    return s, tgt


def walk(seed):
    """WALK_STEPS (settings, targets) pairs behind warm(entry), the entry drawn once.  A step changes one or two
    settings of the step before it or, with probability 1/2, repeats it.  One step, at a drawn position, takes the held
    sort's targets with two rows exchanged (T_swapped, or T_fewer_swapped when the last kept sort is T_fewer's) in a
    BASE-like call that replays: exactly one miss per walk; all later steps keep those targets."""
    rng = np.random.default_rng(seed)
    swap_at = int(rng.integers(1, WALK_STEPS))
    s, tgt, held = BASE.but(entry=ENTRIES[int(rng.integers(len(ENTRIES)))]), "T", "T"
    steps = []
    for i in range(WALK_STEPS):
        if i == swap_at:
            s, tgt = s.but(k=20, lazy=True), held + "_swapped"
        elif i == 0 or rng.random() >= 0.5:
            for _ in range(int(rng.integers(1, 3))):
                s, tgt = _draw_change(rng, s, tgt)
        if s.keeps_sort:
            held = tgt
        steps.append((s, tgt))
    return steps


def repeated_replays(steps):
    """Steps that repeat the step before them and keep their sort: each replays what that step recorded or replayed."""
    return sum(1 for a, b in zip(steps, steps[1:]) if a == b and b[0].keeps_sort)
