"""The generators and oracles of tests/fuzz_cases.py, on the CPU.

* draw_* at the "tool" budget still draw the cases the seeds quoted in test_parity_gpu.py and test_guarded_gpu.py name:
  tests/golden/fuzz_draws.json holds, for cases 0..19 of each tool's default seed and for the three cases those tests
  quote, every scalar of the case line and the shape and first row (at most 8 entries of it) of every drawn array, recorded from the tools' loop
  bodies before they moved into fuzz_cases.py.
* The corpus tests/test_fuzz_gpu.py runs (fuzz_cases.SUITE_CORPUS) draws every entry of every choice list, the follow-up
  case and the far clouds, and stays inside the suite's sizes.
* Two caps keep the GPU checks from going quiet: the fused-GLL comparison is skipped on at most 15 % of the GLL cases
  (jitter <= 0.02; expected 0.02 / 0.3 = 6.7 %), and at most 1 % of the kNN rows outside lattices and 1-D clouds hold an
  exact distance tie among their k nearest (the rows where an index may differ from the reference's).
* The oracles agree with each other on three small cases per generator: a wrong oracle cannot pass for a wrong kernel.
"""
import concurrent.futures
import functools
import json
import os

import numpy as np
import pytest

import fuzz_cases as F
from dispatch_cases import WORKERS, knn_distances
from multimesh_amd import synth
from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_draws.json")
FUSED_SKIP_CAP = 0.15
TIE_ROW_CAP = 0.01


# ------------------------------------------------------------------------------------------------------ the golden draws
def _golden_entries():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("entry", _golden_entries(), ids=lambda e: f"{e['tool']}-{e['seed']}")
def test_tool_budget_draws_the_recorded_cases(entry):
    want = entry["cases"]
    last = max(int(c) for c in want)
    seen = 0
    for c in F.cases(entry["tool"], entry["seed"], last + 1, entry["budget"]):
        rec = want.get(str(c["case"]))
        if rec is None:
            continue
        seen += 1
        got = {name: c[name] for name in rec["params"]}
        assert got == rec["params"], (c["case"], got, rec["params"])
        for name, a in rec["arrays"].items():
            arr = c[name]
            assert list(arr.shape) == a["shape"], (c["case"], name, arr.shape)
            first = arr.reshape(-1, arr.shape[-1])[0][:8]
            assert first.tobytes() == np.array(a["first"], np.float64).tobytes(), (c["case"], name, first, a["first"])
    assert seen == len(want)


def test_the_quoted_cases_are_the_ones_the_regressions_describe():
    by = {(e["tool"], e["seed"]): e["cases"] for e in _golden_entries()}
    # test_guarded_gpu.py: 17280 = 135 * 128 clustered sources, 83868 targets, k = 3
    p = by["knn", 31003]["1365"]["params"]
    assert (p["kind"], p["nsrc"], p["ntgt"], p["k"], p["dim"]) == ("clustered", 17280, 83868, 3, 3)
    # test_parity_gpu.py: a clustered cloud, k <= 8 / hex_mesh(29, seed=766496109, ...)
    assert by["knn", 501]["2017"]["params"]["kind"] == "clustered" and by["knn", 501]["2017"]["params"]["k"] <= 8
    assert by["pipeline", 424242]["615"]["params"]["n"] == 29
    c = list(F.cases("pipeline", 424242, 616, "tool"))[615]
    assert c["mesh_seed"] == 766496109 and abs(c["jitter"] - 0.104) < 1e-3


# ------------------------------------------------------------------------------------------------- the suite's corpus
@functools.lru_cache(maxsize=None)
def _params(name):
    """The scalars of every case of the corpus (arrays dropped)."""
    out = []
    for c in F.corpus(name):
        p = {key: v for key, v in c.items() if not isinstance(v, np.ndarray)}
        if name == "pipeline":
            p["nelem"] = len(c["ca"])
        if name == "gll":
            p["nelem"] = len(c["src"])
        out.append(p)
    return out


def _seen(name, key, where=lambda p: True):
    return {p[key] for p in _params(name) if where(p)}


def test_corpus_batches_are_what_the_issue_asks_for():
    for name, table in F.SUITE_CORPUS.items():
        assert len({seed for _, seed, _ in table}) == len(table), "every batch has a seed of its own"
        first = table[0][0]
        assert len(F.batches(name, first)) >= 4
        assert [n for _, n in F.batches(name, "guarded")] == [6]
    assert {r for r, _, _ in F.SUITE_CORPUS["knn"]} == {"default", "tree", "list", "strip", "lane", "guarded"}
    assert {r for r, _, _ in F.SUITE_CORPUS["pipeline"]} == {"exact", "tol", "guarded"}


def test_knn_corpus_draws_every_choice_and_stays_inside_the_caps():
    ps = _params("knn")
    assert _seen("knn", "k") >= set(F.KNN_KS)
    assert _seen("knn", "kind") == set(F.KNN_KINDS) | {"far"}
    assert _seen("knn", "dim") == set(F.KNN_DIMS)
    assert _seen("knn", "margin") == set(F.KNN_MARGINS)
    assert _seen("knn", "want_dist") == {True, False}
    assert _seen("knn", "far_ratio", lambda p: p["kind"] == "far") == set(F.FAR_RATIOS)
    assert _seen("knn", "far_cloud", lambda p: p["kind"] == "far") == set(F.FAR_CLOUDS)
    assert sum(p["follow_up"] for p in ps) >= 3
    brackets_src, brackets_tgt = set(), set()
    prev = None
    for p in ps:
        if p["case"] == 0:
            prev = None
        if p["follow_up"]:
            assert (p["nsrc"], p["ntgt"], p["dim"], p["k"]) == (prev["nsrc"], prev["ntgt"], prev["dim"], prev["k"])
            assert p["kind"] != prev["kind"]
        # (a lattice rounds its count to a power: at most (m + 1/2)^dim for m^dim asked)
        assert 1 <= p["nsrc"] < (40_000 if "lattice" not in (p["kind"], p["far_cloud"]) else 43_000) and 1 <= p["ntgt"] < 12_000
        assert 1 <= p["k"] <= min(64, p["nsrc"])
        brackets_src.add(int(np.searchsorted([200, 5000], p["nsrc"], side="right")))
        brackets_tgt.add(int(p["ntgt"] >= 300))
        prev = p
    assert brackets_src == {0, 1, 2} and brackets_tgt == {0, 1}
    # (KNN_KS lies on both sides of 8, 20 and 32, the list lengths at which the dispatch changes kernels)
    assert {7, 8, 13, 20, 24, 32, 33} <= set(F.KNN_KS)


def test_pipeline_corpus_draws_every_choice_and_stays_inside_the_caps():
    for route in ("exact", "tol"):
        assert len(F.batches("pipeline", route)) >= 4
    assert _seen("pipeline", "k") >= set(F.PIPELINE_KS)
    assert _seen("pipeline", "margin") == set(F.PIPELINE_MARGINS)
    assert _seen("pipeline", "ncomp") == set(F.PIPELINE_NCOMP)
    assert _seen("pipeline", "sheared") == {True, False}
    for route in ("exact", "tol"):
        assert _seen("pipeline", "lazy", lambda p: p["route"] == route) == {True, False}
    for p in _params("pipeline"):
        assert 4 <= p["n"] < 14 and 1 <= p["npts"] < 8000 and 1 <= p["k"] <= min(64, p["nelem"])


def test_gll_corpus_draws_every_choice_and_stays_inside_the_caps():
    ps = _params("gll")
    assert {(p["order"], p["dim"]) for p in ps} == {(o, d) for o in F.GLL_ORDERS for d in F.GLL_DIMS}
    assert _seen("gll", "k") >= set(F.GLL_KS)
    assert _seen("gll", "tol") == set(F.GLL_TOLS)
    assert _seen("gll", "margin") == set(F.GLL_MARGINS)
    assert _seen("gll", "snap") == {True, False} and _seen("gll", "ncomp") == set(F.GLL_NCOMP)
    assert _seen("gll", "lazy", lambda p: p["fused"]) == {True, False}
    assert _seen("gll", "want_operator", lambda p: p["fused"]) == {True, False}
    for p in ps:
        assert 3 <= p["n"] < (6 if p["dim"] == 3 else 12) and 1 <= p["npts"] < 2000 and 1 <= p["k"] <= min(27, p["nelem"])


def test_unique_corpus_draws_every_choice_and_stays_inside_the_caps():
    ps = _params("unique")
    assert _seen("unique", "kind") == set(F.UNIQUE_KINDS)
    assert _seen("unique", "dim") == {1, 2, 3}
    assert {int(np.searchsorted([50, 5000], p["n"], side="right")) for p in ps} == {0, 1, 2}
    assert all(1 <= p["n"] < 60_000 for p in ps)


# ---------------------------------------------------------------------------------------------------------- the two caps
def test_fused_gll_comparison_is_skipped_on_few_cases():
    ps = _params("gll")
    skipped = sum(not p["fused"] for p in ps)
    assert all(p["fused"] == (p["jitter"] > 0.02) for p in ps)
    print(f"fused GLL comparison skipped on {skipped} of {len(ps)} cases ({100.0 * skipped / len(ps):.1f} %)")
    assert skipped <= FUSED_SKIP_CAP * len(ps)


def _brute_tie_rows(c):
    """Rows of a case with two equal distances among the k nearest, or between the k-th and the next one (brute force)."""
    kk = min(c["k"] + 1, c["nsrc"])
    if kk < 2:
        return 0
    tgt = c["tgt"]
    parts = np.array_split(np.arange(len(tgt)), min(WORKERS, max(1, len(tgt) // 64)))
    with concurrent.futures.ThreadPoolExecutor(WORKERS) as pool:
        idx = np.concatenate(list(pool.map(lambda rows: O.knn_brute(c["src"], tgt[rows], kk), parts)))
    d = knn_distances(c["src"], tgt, idx)
    return int((d[:, 1:] == d[:, :-1]).any(axis=1).sum())


def test_knn_rows_with_an_exact_tie_are_few():
    rows = ties = 0
    for c in F.corpus("knn"):
        if c["kind"] == "lattice" or c["dim"] == 1:
            continue
        rows += c["ntgt"]
        ties += _brute_tie_rows(c)
    print(f"kNN rows with an exact tie among their k nearest (outside lattices and 1-D): {ties} of {rows} "
          f"({100.0 * ties / rows:.3f} %)")
    assert rows > 50_000 and ties <= TIE_ROW_CAP * rows


# ------------------------------------------------------------------------------------------------ oracle against oracle
def _small(name, count=3):
    """The first `count` small cases of the first default batch of a generator."""
    route, seed, _ = F.SUITE_CORPUS[name][0]
    out = []
    for c in F.cases(name, seed, 200, "suite"):
        size = {"knn": c.get("nsrc", 0) * c.get("ntgt", 0), "pipeline": c.get("npts", 0) * 2000,
                "gll": c.get("npts", 0) * 2000, "unique": c.get("n", 0) * 1000}[name]
        if size <= 6_000_000 and not (name == "knn" and (c["kind"] in ("lattice", "far") or c["dim"] == 1 or c["k"] < 2)):
            out.append(c)
        if len(out) == count:
            return out
    raise AssertionError("no small cases")


def test_knn_oracles_agree():
    for c in _small("knn"):
        i_ref, d_ref = F.knn_reference(c)
        brute = O.knn_brute(c["src"], c["tgt"], c["k"])
        d_brute = knn_distances(c["src"], c["tgt"], brute)
        # general position: the same lists; cKDTree's distances are the stated ones to rounding
        assert np.array_equal(knn_distances(c["src"], c["tgt"], i_ref), d_brute), F.line_knn(c)
        assert np.array_equal(i_ref, brute) or F.knn_judge(i_ref, None, c, brute) is None, F.line_knn(c)
        np.testing.assert_allclose(d_ref, d_brute, rtol=4e-16, atol=0)
        # and the judge refuses a neighbour that is not among the nearest, a repeated id and a wrong distance
        worse = brute.copy()
        far = np.argmax(((c["src"] - c["tgt"][0]) ** 2).sum(axis=1))
        worse[0, -1] = far
        assert F.knn_judge(worse, None, c, i_ref) is not None or c["nsrc"] <= c["k"]
        if c["k"] >= 2:
            twice = brute.copy()
            twice[0, 1] = twice[0, 0]
            assert F.knn_judge(twice, None, c, i_ref) is not None
        assert F.knn_judge(brute, np.nextafter(d_brute, np.inf), c, i_ref) is not None


def test_pipeline_oracles_agree():
    for c in _small("pipeline"):
        cen = O.centroid(c["ca"], c["pa"])
        assert np.allclose(cen, c["pa"][c["ca"]].mean(axis=1), rtol=1e-13, atol=0)
        nn, enc_o, w_o, nf_o, status, vals = F.pipeline_oracle(c)
        assert np.array_equal(nn, O.knn_brute(cen, c["pb"], c["k"])), F.line_pipeline(c)
        ok = status >= 0
        assert nf_o == (~ok).sum()
        # a located target: its weights sum to one and reproduce its coordinates from the element's corners
        assert np.allclose(w_o[ok].sum(axis=1), 1.0, atol=1e-9)
        back = np.einsum("np,npj->nj", w_o[ok], c["pa"][enc_o[ok]])
        scale = np.abs(c["pa"]).max()
        inside = ok & (status < c["k"])
        assert np.abs(back - c["pb"][ok])[inside[ok]].max(initial=0.0) <= 1e-6 * scale
        assert np.allclose(vals[ok], np.einsum("np,cnp->nc", w_o[ok], c["fields"][:, enc_o[ok]]), rtol=1e-12, atol=1e-12)
        assert not vals[~ok].any()


def test_gll_oracles_agree():
    for c in _small("gll"):
        nn = O.knn_ckdtree(c["cen"], c["pts"], c["k"], workers=WORKERS)[0].reshape(c["npts"], c["k"])
        assert np.array_equal(nn, O.knn_brute(c["cen"], c["pts"], c["k"])), F.line_gll(c)
        elem, co, miss = O.locate_gll(c["order"], nn, c["src"], c["pts"], c["tol"], c["snap"])
        found = elem >= 0
        assert miss == (~found).sum() or c["snap"]
        # the coefficients of a located target sum to one and reproduce its coordinates (within the tolerance loop's reach)
        assert np.allclose(co[found].sum(axis=1), 1.0, atol=1e-9)
        vals = O.gather_elem(c["fields"], elem, co)
        want = np.einsum("np,cnp->nc", co[found], c["fields"][:, elem[found]])
        assert np.allclose(vals[found], want, rtol=1e-12, atol=1e-12)


def test_unique_oracles_agree():
    for c in _small("unique"):
        ru, rinv = np.unique(c["pts"], axis=0, return_inverse=True)
        su, sinv = F.unique_by_sort(c["pts"])
        assert np.array_equal(ru, su) and np.array_equal(rinv.reshape(-1), sinv), F.line_unique(c)
        assert np.array_equal(su[sinv], c["pts"])
