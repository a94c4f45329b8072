"""One context's scratch pool and buffers serve calls of different shape one after the other: every entry point lays its
scratch out anew (csrc/mm_scratch_layout.h), over whatever the call before left there.  A sequence of calls with very
different layouts on ONE context -- a kNN query on a uniform cloud, a GLL locate with snap-to-nearest, unique_points, a kNN
query through the tree of a graded cloud (its second pass lays the pool out once more in mid-call), the fused hex8
pipeline with lazy lists (the on-demand list query does the same), then the first call again -- must give, bit for bit,
what each call gives on a context of its own.  The kNN kernels each call launched are compared too, and checked against the
path the scenario is meant for, so that the test cannot pass by another route.  Shapes: tests/dispatch_cases.py."""
import numpy as np
import pytest

import dispatch_cases as D

pytestmark = pytest.mark.gpu


def knn_uniform(c, env):
    env.setenv("MM_KNN_TREE", "0")                                            # (read per build) the grid kernels
    src, tgt, _ = D.knn_cloud("uniform", 3)
    tree = c.knn_build(src)
    idx, dist = tree.query(tgt, 8, want_dist=True)
    out = (idx.numpy(), dist.numpy())
    kernels = c.last_knn_kernels()
    tree.free()
    assert kernels & {"lane", "strip", "cell"} and "tree" not in kernels, kernels
    return out, kernels


def gll_snap(c, env):
    gp, pts, _, nn = D.gll_case(2, 3)
    elem, co, miss = c.locate_gll(2, np.ascontiguousarray(nn[:, :9]), gp, pts, tolerance=1.05, snap_to_nearest=True)
    return (elem.numpy(), co.numpy(), np.int64(miss)), set()


def unique(c, env):
    gp = D.gll_case(2, 3)[0]
    uniq, inv = c.unique_points(np.ascontiguousarray(gp.reshape(-1, 3)))      # element-nodal points: shared faces repeat
    assert len(uniq.numpy()) < gp.shape[0] * gp.shape[1]
    return (uniq.numpy(), inv.numpy()), set()


def knn_graded_tree(c, env):
    env.setenv("MM_KNN_TREE", "1")
    src, tgt = D.graded_cloud()[:2]
    tree = c.knn_build(src)
    idx, dist = tree.query(tgt, 20, want_dist=True)
    out = (idx.numpy(), dist.numpy())
    kernels = c.last_knn_kernels()
    tree.free()
    assert "tree" in kernels, kernels
    return out, kernels


def hex8_lazy(c, env):
    env.delenv("MM_KNN_TREE", raising=False)                                  # the pipeline's own choice of index
    pa, ca, pb, fields, _ = D.sheared_mesh()
    c.set_lazy_lists(True)
    vals, enc, w, nf = c.interpolate_hex8(pa, ca, pb, fields, nelem_to_search=25, want_operator=True)
    kernels = c.last_knn_kernels()
    assert c.last_locate_stats()["reference_order"] > 0 and "list" in kernels, kernels   # full lists were fetched on demand
    return (vals.numpy(), enc.numpy(), w.numpy(), np.int64(nf)), kernels


SEQUENCE = (knn_uniform, gll_snap, unique, knn_graded_tree, hex8_lazy, knn_uniform)


def test_one_context_serves_calls_of_different_shape_like_fresh_contexts(monkeypatch):
    from multimesh_amd.device import Context

    monkeypatch.delenv("MM_KNN_FORCE_LIST", raising=False)
    fresh = {}
    for call in set(SEQUENCE):
        with Context(0) as c:
            fresh[call] = call(c, monkeypatch)
    with Context(0) as c:
        for step, call in enumerate(SEQUENCE):
            out, kernels = call(c, monkeypatch)
            want, want_kernels = fresh[call]
            assert kernels == want_kernels, (step, call.__name__, kernels, want_kernels)
            for i, (a, b) in enumerate(zip(out, want)):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (step, call.__name__, i)
