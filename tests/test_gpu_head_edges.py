"""The kernels at the head of every ICP iteration (avatar_amd/csrc/avt_kernels.hip: k_lbs, k_lbs_multi<2|4>, k_visibility, k_visibility_frame,
k_finalize, k_budget_hold) away from SMPL's mesh size, at their internal boundaries: 256 vertices / faces per workgroup, the 9 J and 12 J
loops on both sides of 256 and 512, K = 10 against every other K, frame counts that leave the last k_lbs_multi group partial with the grid
remap on, k_visibility_frame's LDS limit (V = 9035 / 9036), k_finalize's register path (ceil(V / 1024) <= 8) against its loop path.

The models are tests/head_models.py's, the yardsticks tests/head_restatement.py's (long double skinning, exact visibility) and
tests/nn_restatement.py's; tests/test_head_edges_cpu.py ties them to the CPU oracle.  Skinning is held to 1e-12 absolute, the project's
bar for this kernel (the oracle itself stays within 2.6e-15 of the long-double restatement on these models); everything else is exact.
The procedural models are never fitted: the fitting kernels run at SMPL's (J, K, P) only."""
import numpy as np
import pytest

import head_models as hm
import head_restatement as hr
import nn_restatement as nr
import test_gpu_icp_budgets as budgets
from avatar_amd import synth
from avatar_amd.capi import Options

pytestmark = pytest.mark.gpu

SKIN_BOUND = 1e-12
PROCEDURAL_NAMES = [hm.procedural_name(row) for row, _ in hm.PROCEDURAL]
SKINNED = PROCEDURAL_NAMES + [hm.resized_name(V, F) for V, F in hm.SKINNED_RESIZED]
RESIZED_NAMES = [hm.resized_name(V, F) for V, F in hm.RESIZED]
LBS_FRAMES = (1, 7, 8, 9)                 # avt_lbs_update: 8 is where the grid remap starts
STATE_FRAMES = (1, 3, 5, 29)              # icp_iters = 0: with lbs_frames = 4, 29 frames are eight groups (remap on), the last with one live frame
COPIES = [(lf, xf) for lf in (1, 2, 4) for xf in (1, 0)]      # (lbs_frames, xcd_frames); the first is the baseline


def _dims(model):
    return (np.asarray(model["v_template"]).shape[0], np.asarray(model["f"]).shape[0], np.asarray(model["kintree_table"]).shape[1],
            np.asarray(model["shapedirs"]).shape[2])


@pytest.fixture(scope="module")
def models(smpl):
    return dict(hm.procedural_cases() + hm.resized_cases(smpl))


@pytest.fixture(scope="module")
def gmodels(models):
    from avatar_amd import api
    made = {}

    def get(name):
        if name not in made:
            made[name] = api.AvatarModel(models[name])
        return made[name]
    return get


def _ctx(gm, max_points, max_frames, **tuning):
    from avatar_amd import api
    J = gm.numJoints()
    ctx = api.Context(gm, J, np.arange(J, dtype=np.int32), max_points, max_frames, device=0)
    return ctx.set_tuning(**tuning) if tuning else ctx


def _worst(got, ref):
    """largest absolute difference of (cloud, joint positions, joint transforms) against the long-double restatement"""
    return max(float(np.abs(g - r).max()) for g, r in zip(got, ref))


def _quats(R, scale_frame=1):
    from avatar_amd import api
    q = np.array([api.rot_to_quat(r) for r in R])
    if len(q) > scale_frame:
        q[scale_frame] *= 1.01             # one frame off the unit sphere: the forward model does not normalise
    return q


# ---- skinning ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SKINNED)
def test_lbs_update_matches_the_long_double_restatement(models, gmodels, name):
    """avt_lbs_update (k_lbs from rotation matrices) with 1, 7, 8 and 9 frames of different poses: cloud, joint positions and joint
    transforms within 1e-12 of the restatement; the grid remap (xcd_frames, from 8 frames on) and lbs_frames change no bit."""
    m = models[name]
    n = max(LBS_FRAMES)
    w, p, R = hm.poses(m, n, seed=1)
    ref = [hr.update(m, w[f], p[f], R[f]) for f in range(n)]
    ctx = _ctx(gmodels(name), 8, n)
    worst = 0.0
    for nf in LBS_FRAMES:
        base = None
        for lf, xf in COPIES:               # (avt_lbs_update always runs k_lbs: lbs_frames must not matter, xcd_frames remaps its grid)
            ctx.set_tuning(lbs_frames=lf, xcd_frames=xf)
            got = ctx.lbs_update(w[:nf], p[:nf], R[:nf])
            if base is None:
                base = got
                for f in range(nf):
                    worst = max(worst, _worst((got[0][f], got[1][f], got[2][f]), ref[f]))
            else:
                assert all(np.array_equal(a, b) for a, b in zip(got, base)), (name, nf, f"lbs_frames {lf} xcd_frames {xf} changes bits")
    print(f"{name}: k_lbs against the restatement {worst:.2e}")
    assert worst <= SKIN_BOUND, (name, worst)


def _state_run(ctx, nf, p, q, w):
    """icp_iters = 0 over nf frames of one dummy labelled point each: bucketing plus one skinning launch from the quaternion state"""
    ctx.frames_upload([np.zeros((1, 3))] * nf, [np.zeros(1, np.int32)] * nf)
    ctx.state_upload(p[:nf], q[:nf], w[:nf])
    ctx.optimize_resident(Options.demo(icp_iters=0))
    return [ctx.posed(f) for f in range(nf)]


@pytest.mark.parametrize("name", SKINNED)
def test_skinning_from_the_quaternion_state(models, gmodels, name):
    """optimize() with icp_iters = 0 (k_lbs / k_lbs_multi<2|4> with from_state = 1) over 1, 3, 5 and 29 frames: every frame within 1e-12
    of the restatement from the same quaternions; lbs_frames = 1, 2, 4 and xcd_frames = 0, 1 give the same bits for every frame."""
    m = models[name]
    n = max(STATE_FRAMES)
    w, p, R = hm.poses(m, n, seed=2)
    q = _quats(R)
    ref = [hr.update_q(m, p[f], q[f], w[f]) for f in range(n)]
    ctx = _ctx(gmodels(name), 8, n)
    worst = 0.0
    for nf in STATE_FRAMES:
        base = None
        for lf, xf in COPIES:
            ctx.set_tuning(lbs_frames=lf, xcd_frames=xf)
            got = _state_run(ctx, nf, p, q, w)
            if base is None:
                base = got
                for f in range(nf):
                    worst = max(worst, _worst(got[f], ref[f]))
            else:
                bad = [f for f in range(nf) if not all(np.array_equal(a, b) for a, b in zip(got[f], base[f]))]
                assert not bad, (name, nf, f"lbs_frames {lf} xcd_frames {xf} differs from lbs_frames 1 on frames {bad}")
    print(f"{name}: skinning from the state against the restatement {worst:.2e}")
    assert worst <= SKIN_BOUND, (name, worst)


_probe, _starts = hm.probe, hm.starts


@pytest.mark.parametrize("name", [hm.resized_name(V, F) for V, F in hm.SKINNED_RESIZED])
def test_skinning_from_the_skeleton_tables(smpl, models, gmodels, name):
    """After a fit (moment form, 5 frames, icp_iters = 2, max_iters_per_icp = 3) the closing launch skins from the skeleton tables k_solve
    made (from_state = 2; k_lbs_multi with lbs_frames = 2, 4: the last group partial): posed(f) within 1e-12 of the restatement at the
    state the call returned, and the same bits for lbs_frames = 1, 2, 4."""
    from avatar_amd import api
    m = models[name]
    nf = 5
    p0, q0, w0 = _starts(smpl, nf)
    pt, qt, wt = _starts(smpl, nf, first=60)
    datas, labs = [], []
    for f in range(nf):          # data: the model posed a little away from the start state
        qb = 0.9 * q0[f] + 0.1 * qt[f]
        target = hr.update_q(m, p0[f] + 0.02, qb / np.linalg.norm(qb, axis=1, keepdims=True), w0[f] + 0.3)[0].astype(np.float64)
        d, l = _probe(m, target, f)
        datas.append(d); labs.append(l)
    ctx = _ctx(gmodels(name), len(labs[0]), nf)
    ctx.set_data_term(api.Context.DATA_TERM_MOMENTS)
    opt = Options.demo(icp_iters=2, max_iters_per_icp=3)
    base, worst = None, 0.0
    for lf in (1, 2, 4):
        ctx.set_tuning(lbs_frames=lf)
        ctx.frames_upload(datas, labs)
        ctx.state_upload(p0, q0, w0)
        ctx.optimize_resident(opt)
        p, q, w, st = ctx.state_download()
        got = [ctx.posed(f) for f in range(nf)]
        if base is None:
            base = (p, q, w, got)
            assert not np.array_equal(p, p0)            # the fit moved
            for f in range(nf):
                worst = max(worst, _worst(got[f], hr.update_q(m, p[f], q[f], w[f])))
        else:
            assert np.array_equal(p, base[0]) and np.array_equal(q, base[1]) and np.array_equal(w, base[2]), (name, lf)
            assert all(np.array_equal(a, b) for f in range(nf) for a, b in zip(got[f], base[3][f])), (name, lf)
    print(f"{name}: skinning from the skeleton tables against the restatement {worst:.2e}")
    assert worst <= SKIN_BOUND, (name, worst)


# ---- stand-alone visibility -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROCEDURAL_NAMES + [hm.resized_name(9036, 2049)])
def test_visibility_equals_the_restatement(models, gmodels, name):
    """avt_visibility (k_visibility, 256 faces per workgroup) on random clouds, posed clouds and clouds with faces exactly at the threshold
    (z = 1e-4 is not visible, the next double is; a reversed winding; faces 0, 255, 256 and F - 1): equal to the restatement, a vertex no
    face references stays 0, enable = 0 gives all 1."""
    m = models[name]
    V, F, J, K = _dims(m)
    mesh = np.asarray(m["f"])
    rng = np.random.default_rng([6, V, F])
    w, p, R = hm.poses(m, 2, seed=3)
    clouds = [rng.uniform(-1, 1, (V, 3)), rng.uniform(-1, 1, (V, 3)) * 1e-2] + [hr.update(m, w[f], p[f], R[f])[0].astype(np.float64) for f in range(2)]
    if F >= 4:
        clouds += [c for c, _ in hm.threshold_clouds(m)]
    ctx = _ctx(gmodels(name), 8, 1)
    used = np.bincount(mesh.reshape(-1), minlength=V)
    for i, c in enumerate(clouds):
        got = ctx.visibility(c, True)
        assert np.array_equal(got, hr.visibility(mesh, c, True)), (name, i, int((got != hr.visibility(mesh, c, True)).sum()))
        assert not got[used == 0].any()
        assert np.array_equal(ctx.visibility(c, False), np.ones(V, np.uint8)), (name, i)


def test_visibility_of_a_model_without_faces():
    """F = 0: no face, no launch; the cleared flags stand (enable = 1: all 0, enable = 0: all 1)."""
    from avatar_amd import api
    m = hm.procedural(8, 0, 2, 1, "chain")
    gm = api.AvatarModel(m)
    assert gm.numFaces() == 0
    ctx = _ctx(gm, 8, 1)
    cloud = np.random.default_rng(8).uniform(-1, 1, (8, 3))
    assert np.array_equal(ctx.visibility(cloud, True), np.zeros(8, np.uint8))
    assert np.array_equal(ctx.visibility(cloud, False), np.ones(8, np.uint8))
    assert np.array_equal(ctx.visibility(cloud, True), np.zeros(8, np.uint8))


# ---- the head of an ICP iteration through optimize() -----------------------------------------------------------------------------------
TUNINGS = {"default": {}, "frame": dict(nn_force_part=1, vis_frame_min=1, groups=1)}
BOTH_FORMS = {hm.resized_name(V, F) for V, F in ((1025, 1023), (8192, 13776), (8193, 13777), (9036, 2049))}
NINE_FRAMES = {hm.resized_name(1025, 1023), hm.resized_name(8193, 13777)}


@pytest.fixture(scope="module")
def oracles(models):
    from oracle import oracle as orc
    made = {}

    def get(name):
        if name not in made:
            made[name] = orc.OracleModel(models[name])
        return made[name]
    return get


def _head_run(ctx, datas, labs, p0, q0, w0, opt):
    ctx.frames_upload(datas, labs)
    ctx.state_upload(p0, q0, w0)
    ctx.optimize_resident(opt)
    p, q, w, st = ctx.state_download()
    return p, q, w, st, [ctx.correspondences(f, len(labs[f])) for f in range(len(labs))]


@pytest.mark.parametrize("name", RESIZED_NAMES)
def test_head_of_an_icp_iteration(smpl, models, gmodels, oracles, name):
    """One ICP iteration (icp_iters = 1, max_iters_per_icp = 1) on frames whose data are the start cloud's own vertices: a visible vertex is
    matched to itself, an invisible one to what the restatement finds among the visible vertices of its part.  Default tuning (k_visibility +
    k_nn_vis) and nn_force_part = 1, vis_frame_min = 1 (k_visibility_frame + k_compact + k_nn_part; at V = 9036 the frame kernel's LDS does
    not fit and k_visibility runs inside the batch): correspondences, per-vertex counts, T and M exact; the normal equations at the returned
    state - built from k_finalize's matched list, by its loop path from V = 8193 on - within 1e-9 of the oracle's on both data-term forms;
    the second run of each shape (the cached graph) repeats the first bit for bit."""
    from avatar_amd import api
    m = models[name]
    V, F, J, K = _dims(m)
    nf = 9 if name in NINE_FRAMES else 3
    p0, q0, w0 = _starts(smpl, nf)
    pm = synth.identity_part_map()
    pov = synth.main_joint(m)
    mesh = np.asarray(m["f"])
    ctx = _ctx(gmodels(name), V, nf)
    start = [c[0] for c in _state_run(ctx, nf, p0, q0, w0)]          # the GPU's own start clouds
    datas, labs, want = [], [], []
    for f in range(nf):
        d, l = _probe(m, start[f], f)
        vis = hr.visibility(mesh, d, True)
        corr = nr.nn_ref(pov, 24, d, vis, d, l)
        # conditions of the test: invisible vertices, dropped labels, and visible vertices matched to themselves
        assert (vis == 0).any() and (vis != 0).any() and (l == -1).any(), (name, f)
        keep = (vis != 0) & (l >= 0)
        assert np.array_equal(corr[keep], np.nonzero(keep)[0]) and (corr[l == -1] == -1).all()
        moved = (vis == 0) & (l >= 0) & (corr >= 0)
        assert moved.any() and (corr[moved] != np.nonzero(moved)[0]).all()
        datas.append(d); labs.append(l); want.append((corr,) + hr.finalise(corr, V))
    opt = Options.demo(icp_iters=1, max_iters_per_icp=1)
    forms = (("rows", api.Context.DATA_TERM_ROWS), ("moments", api.Context.DATA_TERM_MOMENTS)) if name in BOTH_FORMS else (("auto", None),)
    failures = []
    for tname, tun in TUNINGS.items():
        for fname, form in forms:
            ctx = _ctx(gmodels(name), V, nf, **tun)
            t = ctx.tuning()
            assert all(getattr(t, k) == v for k, v in tun.items())
            if form is not None:
                ctx.set_data_term(form)
            p, q, w, st, corr = _head_run(ctx, datas, labs, p0, q0, w0, opt)
            for f in range(nf):
                rc, cnt, M, T = want[f]
                gc = ctx.nn_sums(f)[0]
                if not (np.array_equal(corr[f], rc) and np.array_equal(gc, cnt) and st[f].num_correspondences == T and st[f].matched_model_points == M):
                    failures.append(f"{tname}/{fname} frame {f}: {int((corr[f] != rc).sum())} indices, {int((gc != cnt).sum())} counts, "
                                    f"T {st[f].num_correspondences} for {T}, M {st[f].matched_model_points} for {M}")
            if name in BOTH_FORMS:
                om = oracles(name)
                for f in range(nf):
                    H, g, cost = ctx.normal_equations(f)
                    oc, og, oH, _ = om.evaluate(p[f], q[f], w[f], corr[f], datas[f], 0.0, 0.0, aggregate=0)
                    eh, eg = float(np.abs(H - oH).max() / np.abs(oH).max()), float(np.abs(g - og).max() / max(1.0, np.abs(og).max()))
                    if not (eh < 1e-9 and eg < 1e-9):
                        failures.append(f"{tname}/{fname} frame {f}: normal equations off by {eh:.2e} (H), {eg:.2e} (g)")
            p2, q2, w2, st2, corr2 = _head_run(ctx, datas, labs, p0, q0, w0, opt)      # the cached graph replayed
            if not (np.array_equal(p, p2) and np.array_equal(q, q2) and np.array_equal(w, w2) and all(np.array_equal(a, b) for a, b in zip(corr, corr2))):
                failures.append(f"{tname}/{fname}: the second run differs from the first")
    assert not failures, f"{name}: " + "; ".join(failures[:12])


# ---- per-frame budgets at other hold-block sizes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(255, 257), (1025, 1023)])
def test_budgets_at_other_hold_block_sizes(smpl, models, gmodels, size):
    """k_budget_hold copies nctl + 2 xsize + 3 V + 15 J doubles per frame in 2048-element pieces: the budgets test of
    tests/test_gpu_icp_budgets.py on meshes whose hold block ends elsewhere (V = 255: one piece; V = 1025: two)."""
    from avatar_amd import api
    name = hm.resized_name(*size)
    m = models[name]
    pm = synth.identity_part_map()
    frames = []
    for seed in (30, 31, 32, 33, 34):
        w, p, R = synth.sample_ground_truth(smpl, seed)
        data, labels = synth.render_cloud(m, synth.pose_vertices(m, w, p, R), pm)
        assert len(labels) > 200
        sel = np.arange(0, len(labels), max(1, len(labels) // 4000))
        w0, p0, R0 = synth.perturb_start(w, p, R, seed)
        frames.append((data[sel], labels[sel], p0, api.rot_to_quat(R0), w0))
    budgets._check_budgets(gmodels(name), frames, 5, dict(max_iters_per_icp=3))
