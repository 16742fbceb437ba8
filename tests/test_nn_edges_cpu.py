"""The inputs of tests/test_gpu_nn_edges.py on the CPU: the numpy restatement of the correspondence search equals the CPU
oracle (orc_nn) on every case, and every case is what it says it is (exact visible counts, real ties, the stop rule's equality,
run lengths)."""
import numpy as np
import pytest

import nn_cases
import nn_restatement as nr


def _ref(model, case):
    name, pm, npart, cloud, vis, data, labels = case
    return nr.nn_ref(nn_cases.part_of_vertex(model, pm), npart, cloud, vis, data, labels)


@pytest.mark.parametrize("group", list(nn_cases.GROUPS))
def test_restatement_equals_the_oracle_on_every_case(smpl, omodel, group):
    assert np.array_equal(nn_cases.main_joint(smpl), omodel.main_joint())
    for case in nn_cases.cases(smpl, group):
        name, pm, npart, cloud, vis, data, labels = case
        ref = _ref(smpl, case)
        got = omodel.nn(pm, npart, cloud, vis, data, labels)
        assert np.array_equal(got, ref), (name, int((got != ref).sum()))
        assert np.isfinite(cloud).all() and np.isfinite(data).all(), name


def test_case_names_are_unique_and_every_group_has_cases(smpl):
    names = [c[0] for c in nn_cases.all_cases(smpl)]
    assert len(set(names)) == len(names)
    assert all(len(nn_cases.cases(smpl, g)) > 0 for g in nn_cases.GROUPS)
    for mapname in ("identity", "merged", "single", "sparse64"):
        pm, npart = nn_cases.part_map(mapname)
        assert len(pm) == nn_cases.J and pm.min() >= 0 and pm.max() < npart <= 64
    pov = nn_cases.part_of_vertex(smpl, nn_cases.part_map("merged")[0])
    assert int((pov == 0).sum()) == 1983
    pm, _ = nn_cases.part_map("sparse64")
    assert np.diff(np.sort(pm)).min() >= 2 and pm.min() >= 2 and pm.max() <= 61      # empty parts in between and at both ends


def test_visible_count_sweep_sets_exactly_n(smpl):
    seen = []
    for case in nn_cases.cases(smpl, "sweep"):
        name, pm, npart, cloud, vis, data, labels = case
        pr = nn_cases.PROMISES[name]
        pov = nn_cases.part_of_vertex(smpl, pm)
        assert int(vis[pov == pr["part"]].sum()) == pr["visible"], name
        assert int((labels == pr["part"]).sum()) >= 300 and (labels == -1).any() and (labels == npart).any(), name
        ref = _ref(smpl, case)
        assert ((ref[labels == pr["part"]] >= 0).all() if pr["visible"] else (ref[labels == pr["part"]] == -1).all()), name
        seen.append((npart, pr["visible"]))
    assert [n for p, n in seen if p == 22] == list(nn_cases.SWEEP_N) and [n for p, n in seen if p == 24] == [511, 512, 513]


def test_tile_cases_put_answers_on_both_sides_of_the_boundary(smpl):
    for case in nn_cases.cases(smpl, "tiles"):
        name, pm, npart, cloud, vis, data, labels = case
        pr = nn_cases.PROMISES[name]
        pov = nn_cases.part_of_vertex(smpl, pm)
        ids1 = np.nonzero(pov == 1)[0]
        assert int((pov == 0).sum()) + pr["split"] == 1024
        ref = _ref(smpl, case)[pr["first"]:]
        assert np.array_equal(ref, pr["targets"]), name
        rank = np.searchsorted(ids1, ref)                       # position of the answer inside part 1
        behind = int((rank >= pr["split"]).sum())
        if name.endswith("first-tile-empty"):
            assert behind == len(ref) and not vis[ids1[:pr["split"]]].any()
        else:
            assert behind == len(ref) // 2, name


def test_tie_cases_tie(smpl):
    for group in ("ties", "magnitudes"):
        for case in nn_cases.cases(smpl, group):
            name, pm, npart, cloud, vis, data, labels = case
            pr = nn_cases.PROMISES.get(name, {})
            if "tie_queries" not in pr:
                continue
            tc = nr.tie_counts(nn_cases.part_of_vertex(smpl, pm), npart, cloud, vis, data, labels)[pr["tie_queries"]]
            if pr.get("subnormal"):                              # the two distances are distinct subnormals: no tie at all
                assert (tc[tc > 0] >= 1).all()
                r = nr.dist2(np.zeros((1, 3)), np.array([[1e-155, 0, 0], [2e-155, 0, 0]]))[0]
                assert 0.0 < r[0] < r[1] < 2.3e-308, name
                continue
            assert (tc >= 2).mean() >= 0.5, (name, float((tc >= 2).mean()))


def test_stop_rule_cases_hit_the_equality(smpl):
    t = np.array([0.25, -0.5, 2.5])
    n = 0
    for case in nn_cases.cases(smpl, "ties"):
        name, pm, npart, cloud, vis, data, labels = case
        pr = nn_cases.PROMISES.get(name, {})
        if not pr.get("gap_tie"):
            continue
        n += 1
        pov = nn_cases.part_of_vertex(smpl, pm)
        ref = _ref(smpl, case)
        for q in range(npart):
            ids = np.nonzero(pov == q)[0]
            A, B = cloud[ids[0]], cloud[ids[1]]
            r = nr.dist2(t[None], np.stack([A, B]))[0]
            assert r[0] == r[1] == 1.5625
            gap = abs(A[1] - t[1])
            assert gap * gap == 1.5625 and abs(B[1] - t[1]) < gap                 # A's y gap alone equals the best distance
            others = np.delete(cloud[ids], [0, 1], axis=0)
            assert nr.dist2(t[None], others).min() > 1.5625
            assert (ref[labels == q] == ids[0]).all() and pr["answers"][q] == ids[0]
    assert n == 6


def test_zero_distance_and_run_cases(smpl):
    case = [c for c in nn_cases.cases(smpl, "slabs") if c[0] == "slab-zero-distance"][0]
    name, pm, npart, cloud, vis, data, labels = case
    ref = _ref(smpl, case)
    assert (ref >= 0).all() and np.array_equal(cloud[ref], data)                  # every query IS a candidate
    for case in nn_cases.cases(smpl, "runs"):
        name, pm, npart, cloud, vis, data, labels = case
        seq = nn_cases.PROMISES[name]["sequence"]
        ref = _ref(smpl, case)
        assert np.array_equal(ref[1:], seq), name
        edges = np.nonzero(np.diff(ref[1:]))[0] + 1
        lengths = np.diff(np.concatenate([[0], edges, [len(seq)]]))
        assert list(lengths[:len(nn_cases.RUNS)]) == list(nn_cases.RUNS) and (lengths[len(nn_cases.RUNS):] == 1).all(), name
        assert np.abs(data[1:] - data[0]).max(axis=1).min() > 1.4                   # the centre lies far from the rest
        pov = nn_cases.part_of_vertex(smpl, pm)
        assert int(vis[pov == labels[1]].sum()) == int(name.split("-")[2])


def test_sums_restatement_equals_a_plain_integer_loop(smpl):
    picked = [c for c in nn_cases.all_cases(smpl) if c[0] in ("runs-identity-400-first-1", "sweep-merged-513", "queries-sparse64")]
    assert len(picked) == 3
    for case in picked:
        name, pm, npart, cloud, vis, data, labels = case
        corr = _ref(smpl, case)
        cnt, fsum, centre = nr.nn_sums_ref(corr, data, nn_cases.V)
        assert np.array_equal(centre, data[0])
        c2 = [0] * nn_cases.V
        f2 = [[0] * nn_cases.V for _ in range(3)]
        for i, v in enumerate(corr.tolist()):
            if v < 0:
                continue
            c2[v] += 1
            for k in range(3):
                f2[k][v] += int(round(float((data[i, k] - data[0, k]) * 2.0 ** 40)))   # round(): half to even, as rint
        assert cnt.tolist() == c2 and fsum.tolist() == f2, name
        assert cnt.sum() == (corr >= 0).sum() > 0
