"""The inputs of tests/test_gpu_head_edges.py on the CPU: every model of tests/head_models.py is what it says it is (PROMISES), is accepted
by the CPU oracle and by avt_model_create, and the plain restatements of tests/head_restatement.py equal the oracle on it: skinning in
long double against the oracle's double within 1e-14, visibility exactly."""
import ctypes

import numpy as np
import pytest

import head_models as hm
import head_restatement as hr
import nn_restatement as nr
from avatar_amd import capi

# The oracle in double against the long-double restatement: at most 2.8e-15 on clouds of a few metres, measured over procedural models up
# to the 58-level chain and V = 9036; 1e-14 is that with a margin of about 4x for seeds not tried.  The GPU tests' bar of 1e-12 then has a
# factor of 100 over legitimate rounding at every shape.  If this fails, the restatement or the case is wrong: fix that, not the bound.
ORACLE_BOUND = 1e-14
_SEEN = {"skin": 0.0}


def _names():
    return [hm.procedural_name(row) for row, _ in hm.PROCEDURAL] + [hm.resized_name(V, F) for V, F in hm.RESIZED]


@pytest.fixture(scope="module")
def models(smpl):
    return dict(hm.procedural_cases() + hm.resized_cases(smpl))


@pytest.fixture(scope="module")
def oracles(models):
    from oracle import oracle as orc
    made = {}

    def get(name):
        if name not in made:
            made[name] = orc.OracleModel(models[name])
        return made[name]
    return get


def _dims(model):
    return (np.asarray(model["v_template"]).shape[0], np.asarray(model["f"]).shape[0], np.asarray(model["kintree_table"]).shape[1],
            np.asarray(model["shapedirs"]).shape[2])


def test_tables_are_complete():
    names = _names()
    assert len(set(names)) == len(names) == 15 + 10
    assert [r[0][2] for r in hm.PROCEDURAL if r[0][4] == "random"] == [21, 22, 28, 29, 42, 43, 56, 57]
    assert set(hm.SKINNED_RESIZED) <= set(hm.RESIZED)


@pytest.mark.parametrize("name", _names())
def test_every_promise_holds(smpl, models, name):
    m, pr = models[name], hm.PROMISES[name]
    V, F, J, K = _dims(m)
    got = hm.shape_promises(V, F, J)
    for k in ("v256", "f256", "passes9", "passes12", "chunk", "finalize", "vis_frame", "vis_lds"):
        if k in pr:
            assert got[k] == pr[k], (name, k, got[k], pr[k])
    anc = hm.ancestor_counts(m)
    assert anc.min() >= 1 and anc.max() <= pr["anc_le"] <= 16, (name, int(anc.max()))
    if pr["anc_max"] is not None:
        assert anc.max() == pr["anc_max"], (name, int(anc.max()))
    W = hm.dense_weights(m)
    assert ((W > 1e-12).sum(1) >= 1).all()
    a = capi.ModelArrays(m)
    assert (a.V, a.F, a.J, a.K, a.P) == (V, F, J, K, 3 + 3 * J + K) and a.P <= 179
    stored = np.diff(a.w_colptr)
    assert stored.min() >= 1 and stored.max() <= 4
    faces = np.asarray(m["f"])
    assert faces.shape == (F, 3) and faces.min() >= 0 and faces.max() < V
    if name.startswith("procedural"):
        tree = name.rsplit("-", 1)[1]
        lv = hm.levels(hm.parents(m))
        if pr["levels"] is not None:
            assert lv.max() + 1 == pr["levels"]
        if tree == "random":
            par = hm.parents(m)
            assert all(max(0, j - 3) <= par[j] < j for j in range(1, J))
        assert lv[np.nonzero((W > 1e-12).any(0))[0]].max() <= hm.MAX_LEVEL
        assert np.abs(np.asarray(m["v_template"])).max() <= 1.0                       # a 2 m box
        assert "prior_weight" not in m and a.ncomps == 0
        Jr = np.asarray(m["J_regressor"])
        assert np.abs(Jr.sum(1) - 1.0).max() < 1e-12 and ((Jr != 0).sum(1) <= 5).all() and (Jr >= 0).all()
        sp_ = m["_special"]
        if V >= 8 and J >= 2:
            assert len(sp_["stored_zero"]) == 3 and len(sp_["low_sum"]) == 3
            for v in sp_["stored_zero"]:                                              # the 0.0 is a stored entry of the vertex's column
                col = a.w_val[a.w_colptr[v]:a.w_colptr[v + 1]]
                assert (col == 0.0).sum() == 1 and abs(col.sum() - 1.0) < 1e-12
            v = sp_["first_slot_zero"]
            assert a.w_val[a.w_colptr[v]] == 0.0 and a.w_colptr[v + 1] - a.w_colptr[v] >= 2
            assert np.abs(W[sp_["low_sum"]].sum(1) - 0.7).max() < 1e-12
            rest = np.setdiff1d(np.arange(V), sp_["low_sum"])
            assert np.abs(W[rest].sum(1) - 1.0).max() < 1e-12
            assert set(stored.tolist()) >= {1, 2} and stored.max() == min(4, min(int(lv.max()), hm.MAX_LEVEL) + 1)     # 1 to 4 weights
        if F >= 8:
            used = np.bincount(faces.reshape(-1), minlength=V)
            assert (used == 0).any() and (used >= 2).any()                            # vertices without a face; faces that share vertices
            assert ((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])).any()     # a degenerate face
            at = hm.threshold_faces(F)
            assert len(at) == 4 and set(at) >= {i for i in (0, 255, 256, F - 1) if i < F}
            tv = faces[at].reshape(-1)
            assert len(set(tv.tolist())) == 12 and (used[tv] == 1).all()              # the threshold faces' vertices are theirs alone
        elif V >= 3:
            assert len(set(faces[0].tolist())) == 3
    else:
        assert J == 24 and K == 10 and a.ncomps > 0                                   # skeleton, shape keys and prior are SMPL's
        assert all(m[k] is smpl[k] for k in ("kintree_table", "prior_weight", "prior_mean", "prior_cov"))
        assert np.abs(W.sum(1) - 1.0).max() < 1e-9
        assert np.bincount(hm.synth.main_joint(m), minlength=24).min() >= 4
        Jr = np.asarray(m["J_regressor"])
        assert ((Jr != 0).sum(1) == 8).all() and set(np.unique(Jr).tolist()) == {0.0, 0.125}
        assert len(np.unique(np.asarray(m["v_template"]), axis=0)) == V
        if V > 6890:
            used = np.bincount(faces.reshape(-1), minlength=V)
            assert (used[6890:] == 0).sum() > 0                                       # added vertices that no face references


@pytest.mark.parametrize("name", _names())
def test_model_is_accepted_and_restatements_equal_the_oracle(models, oracles, name):
    from avatar_amd import api
    m = models[name]
    V, F, J, K = _dims(m)
    om = oracles(name)
    assert (om.V, om.F, om.J, om.K) == (V, F, J, K)
    lib = capi.load_library()
    desc = capi.ModelArrays(m)
    d = desc.desc()
    h = ctypes.c_void_p()
    assert lib.avt_model_create(ctypes.byref(d), ctypes.byref(h)) == 0, lib.avt_last_error()
    mj = np.empty(V, np.int32)
    assert lib.avt_model_main_joint(h, capi.iptr(mj)) == 0 and np.array_equal(mj, om.main_joint())
    lib.avt_model_destroy(h)
    assert max(len(om.ancestors(v)) for v in range(0, V, max(1, V // 300))) <= 16
    w, p, R = hm.poses(m, 4)
    worst = 0.0
    for f in range(4):
        rc, rj, rt = hr.update(m, w[f], p[f], R[f])
        oc, oj, ot = om.update(w[f], p[f], R[f])
        e = max(float(np.abs(oc - rc).max()), float(np.abs(oj - rj).max()), float(np.abs(ot - rt).max()))
        q = api.rot_to_quat(R[f]) * (1.01 if f == 1 else 1.0)                         # (one pose with quaternions off the unit sphere)
        qc = hr.update_q(m, p[f], q, w[f])[0]
        e = max(e, float(np.abs(om.points(p[f], q, w[f]) - qc).max()))
        worst = max(worst, e)
    _SEEN["skin"] = max(_SEEN["skin"], worst)
    print(f"{name}: oracle against the long-double restatement {worst:.2e} (largest so far {_SEEN['skin']:.2e})")
    assert worst <= ORACLE_BOUND, (name, worst)


@pytest.mark.parametrize("name", _names())
def test_visibility_restatement_equals_the_oracle(models, oracles, name):
    m = models[name]
    V, F, J, K = _dims(m)
    om = oracles(name)
    mesh = np.asarray(m["f"])
    rng = np.random.default_rng([5, V, F])
    w, p, R = hm.poses(m, 2)
    clouds = [rng.uniform(-1, 1, (V, 3)), rng.uniform(-1, 1, (V, 3)) * 1e-2] + [om.update(w[f], p[f], R[f])[0] for f in range(2)]
    for c in clouds:
        for en in (1, 0):
            assert np.array_equal(hr.visibility(mesh, c, en), om.visibility(c, en)), name
        if F:
            used = np.bincount(mesh.reshape(-1), minlength=V)
            assert not hr.visibility(mesh, c, 1)[used == 0].any()
    if F >= 4:
        seen = set()
        for c, placed in hm.threshold_clouds(m):
            vis = hr.visibility(mesh, c, 1)
            assert np.array_equal(vis, om.visibility(c, 1)), name
            for fidx, (kind, verts) in placed.items():
                i1, i2, i3 = verts
                ax, ay, bx, by = c[i2, 0] - c[i1, 0], c[i2, 1] - c[i1, 1], c[i1, 0] - c[i3, 0], c[i1, 1] - c[i3, 1]
                z = ax * by - ay * bx
                want = [1e-4, np.nextafter(1e-4, 1.0), -1e-4, -np.nextafter(1e-4, 1.0)][kind]
                assert z == want, (name, fidx, kind, z)
                if kind != 3 or name.startswith("procedural"):       # (a real mesh has the neighbour across the long edge: the reversed face's z = -c is its +c)
                    assert vis[list(verts)].all() == (kind == 1) and vis[list(verts)].any() == (kind == 1), (name, fidx, kind)
                seen.add((fidx, kind))
            if name.startswith("procedural"):
                assert int(vis.sum()) == 3                           # the one visible face's vertices and nothing else
            elif all(k in (0, 2) for k, _ in placed.values()):
                assert not vis.any()
        assert seen == {(f, k) for f in hm.threshold_faces(F) for k in range(4)}      # every threshold face through every kind


@pytest.mark.parametrize("size", hm.RESIZED)
def test_probe_frames_hold_what_the_gpu_test_needs(smpl, models, oracles, size):
    """The frames of test_head_of_an_icp_iteration (here from the oracle's start cloud): invisible vertices, dropped labels, every visible
    vertex matched to itself, every invisible one to another vertex; T and M differ, and some vertex has several matches."""
    name = hm.resized_name(*size)
    m = models[name]
    V = size[0]
    p0, q0, w0 = hm.starts(smpl, 3)
    pov = hm.synth.main_joint(m)
    assert np.array_equal(pov, oracles(name).main_joint())
    for f in range(3):
        d, l = hm.probe(m, oracles(name).points(p0[f], q0[f], w0[f]), f)
        vis = hr.visibility(np.asarray(m["f"]), d, True)
        corr = nr.nn_ref(pov, 24, d, vis, d, l)
        assert np.array_equal(corr, oracles(name).nn(np.arange(24, dtype=np.int32), 24, d, vis, d, l))
        assert (vis == 0).any() and (vis != 0).any() and 3 <= (l == -1).sum() <= max(3, V // 100)
        keep = (vis != 0) & (l >= 0)
        assert np.array_equal(corr[keep], np.nonzero(keep)[0]) and (corr[l == -1] == -1).all()
        moved = (vis == 0) & (l >= 0) & (corr >= 0)
        assert moved.any() and (corr[moved] != np.nonzero(moved)[0]).all()
        cnt, M, T = hr.finalise(corr, V)
        assert T == (corr >= 0).sum() == cnt.sum() and M == len(np.unique(corr[corr >= 0])) < T and cnt.max() >= 2
