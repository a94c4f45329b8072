"""The scenes of tests/sequence_cases.py are what tests/test_call_sequences_gpu.py needs them to be, checked on the CPU with
the oracle and the grid's own arithmetic before anything runs on a GPU."""
import numpy as np

import dispatch_cases as D
import sequence_cases as Q

LANE_MIN_Z = 6                       # mm_knn.hip choose_lane: dims[2] >= 6 and npts >= 2 * ncells


def test_scene_takes_the_lane_kernel_on_a_single_level_grid():
    lo, dims, inv_h = Q.grid()
    ncells = int(dims.prod())
    assert dims[2] >= LANE_MIN_Z
    for src in ("S", "S_shifted"):                 # no density level, no coarser grid: the grid can be guessed
        band, sparse = Q.grid_statistic(src)
        print(src, tuple(Q.grid(src)[1]), band, sparse)
        assert band <= 0.01 and sparse <= 0.20     # (the build's thresholds are 0.02 and 0.25)
    for name in ("T", "T_fewer", "T_nan", "T_swapped"):
        assert len(Q.targets(name)) >= 2 * ncells
    assert len(Q.source("S")[1]) == 12_167 and len(Q.targets("T")) == 13_824 + Q.NFAR


def test_targets_run_out_of_candidates_at_8_20_and_32():
    status = Q.located("S", "T", D.KMAX)[3]
    inside = np.arange(len(status)) < len(status) - Q.NFAR
    beyond = {m: int(D.no_accept_within(status, m)[inside].sum()) for m in (8, 20, 32)}
    print(beyond)
    assert beyond[8] >= 500 and beyond[20] >= 50 and beyond[32] >= 4


def test_far_targets_fail_for_every_k_and_no_other_target_does():
    n = len(Q.targets("T"))
    for src in ("S", "S_shifted"):
        for k in Q.KS:
            enc, w, nf, status = Q.located(src, "T", k)
            failed = status < 0
            assert failed[n - Q.NFAR:].all(), (src, k)
            if k >= 20:                    # (shorter lists leave a few targets of the mesh without an accepting candidate)
                assert nf == Q.NFAR and not failed[:n - Q.NFAR].any(), (src, k, nf)
            vals = Q.expected(src, "T", Q.BASE.but(k=k))[0]
            assert not enc[failed].any() and not w[failed].any() and not vals[failed].any()
    assert Q.located("S", "T_nan", 20)[3][Q.NAN_ROW] < 0 and Q.located("S", "T_nan", 20)[2] == Q.NFAR + 1
    assert Q.located("S", "T_fewer", 20)[2] == Q.NFAR - 5


def test_swapped_keeps_every_count_and_moved_changes_one_cell():
    ncells = int(Q.grid()[1].prod())
    for base, swapped in (("T", "T_swapped"), ("T_fewer", "T_fewer_swapped")):
        a, b = Q.cells(Q.targets(base)), Q.cells(Q.targets(swapped))
        assert np.array_equal(np.bincount(a, minlength=ncells), np.bincount(b, minlength=ncells))
        assert (a != b).sum() == 2 and (Q.targets(base) != Q.targets(swapped)).any(axis=1).sum() == 2
    assert (Q.cells(Q.targets("T")) != Q.cells(Q.targets("T_moved"))).sum() == 1
    perm = Q.targets("T_permuted")
    assert np.array_equal(np.sort(perm, axis=0), np.sort(Q.targets("T"), axis=0)) and (perm != Q.targets("T")).any()
    assert np.isnan(Q.targets("T_nan")).any(axis=1).sum() == 1 and len(Q.targets("T_fewer")) == len(Q.targets("T")) - 5


def test_other_sources():
    (pa, ca), (pa2, ca2), (pa3, ca3) = Q.source("S"), Q.source("S_shifted"), Q.source("S_small")
    assert len(ca2) == len(ca) and np.array_equal(ca2, ca) and len(ca3) != len(ca)
    assert ((pa2.min(axis=0) > pa.max(axis=0)) | (pa2.max(axis=0) < pa.min(axis=0))).any()      # disjoint boxes
    assert not np.array_equal(Q.grid("S_shifted")[0], Q.grid("S")[0])


def test_k_20_33_and_64_give_different_answers():
    enc = {k: Q.located("S", "T", k)[0] for k in (20, 33, 64)}
    assert (enc[20] != enc[33]).any(axis=1).sum() >= 1 and (enc[33] != enc[64]).any(axis=1).sum() >= 1


def test_fields():
    one, other, three = Q.fields("one"), Q.fields("other"), Q.fields("three")
    assert one.shape == other.shape == (1, len(Q.source("S")[0])) and three.shape[0] == 3
    assert (one != other).all()


def test_walks_miss_once_and_replay_often_enough():
    total = 0
    entries = set()
    for seed in Q.WALK_SEEDS:
        steps = Q.walk(seed)
        assert len(steps) == Q.WALK_STEPS and steps == Q.walk(seed)
        names = [t for _, t in steps]
        first = next(i for i, t in enumerate(names) if t.endswith("_swapped"))
        assert first >= 1 and all(t in ("T", "T_fewer") for t in names[:first]) and len(set(names[first:])) == 1
        # the swap step replays the sort the walk's model says is held: that is the one miss
        held = [t for s, t in [(Q.BASE, "T")] + steps[:first] if s.keeps_sort][-1]
        assert names[first] == held + "_swapped" and steps[first][0].keeps_sort
        assert len({s.entry for s, _ in steps}) == 1
        entries.add(steps[0][0].entry)
        total += Q.repeated_replays(steps)
    print(total, entries)
    assert total >= Q.WALK_MIN_REPLAYS and entries == set(Q.ENTRIES)
