"""Self-occlusion visibility from a face-id render (include/avt.h: avt_set_occlusion_render, avt_get_visibility; avt_render.hip:
k_occ_faces, k_occ_mark and the renderer's own kernels on the context's clouds).

Expected flags are tests/occlusion_restatement.py's (the CPU restatement of renderFaces plus the back-face test in numpy doubles) or,
for the six small scenes, written out by hand (tests/occlusion_cases.py).  Every comparison is byte equality: the face image is pixel
for pixel and the back-face test is bit-defined."""
import os
import subprocess

import numpy as np
import pytest

import avatar_render_cases as rc
import head_models as hm
import occlusion_cases as oc
import occlusion_restatement as occ
from avatar_amd import synth
from avatar_amd.capi import AvtError, Options

pytestmark = pytest.mark.gpu

SCENES = oc.scenes()
HERE = os.path.dirname(os.path.abspath(__file__))


def _ctx(gm, max_points=8, max_frames=1, **tuning):
    from avatar_amd import api
    J = gm.numJoints()
    ctx = api.Context(gm, J, np.arange(J, dtype=np.int32), max_points, max_frames, device=0)
    return ctx.set_tuning(**tuning) if tuning else ctx


# ---- stand-alone avt_visibility on hand-made meshes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_hand_made_scene(name):
    """The six scenes: the flags written by hand with the mode on, the back-face flags with it off (near-covers-far is the test that
    fails without the feature: there the far quad stays visible), all 1 with enable_occlusion = 0 either way."""
    s = SCENES[name]
    V = len(s["cloud"])
    ctx = _ctx(rc.tiny_model(s["cloud"], s["mesh"]))
    assert np.array_equal(ctx.visibility(s["cloud"], True), s["backface"]), (name, "mode off")
    ctx.set_occlusion_render(oc.S32, oc.K32)
    got = ctx.visibility(s["cloud"], True)
    assert np.array_equal(got, s["visible"]), (name, s["why"], got.tolist())
    assert np.array_equal(ctx.visibility(s["cloud"], False), np.ones(V, np.uint8)), (name, "enable_occlusion = 0")


def test_face_image_is_followed_behind_the_camera():
    """renderFaces culls nothing by depth: a front-facing face with a vertex at z < 0 whose mirrored projection owns pixels is seen."""
    s = oc.behind_but_painted()
    ctx = _ctx(rc.tiny_model(s["cloud"], s["mesh"]))
    ctx.set_occlusion_render(oc.S32, oc.K32)
    assert np.array_equal(ctx.visibility(s["cloud"], True), s["visible"])


def test_switching_modes():
    """width = 0 restores the back-face result; enable_occlusion = 0 gives all 1 with the mode on; a refused setter call leaves the old
    setting in force (on stays on with its camera, off stays off)."""
    from avatar_amd import capi
    s = SCENES["near-covers-far"]
    ctx = _ctx(rc.tiny_model(s["cloud"], s["mesh"]))
    lib = capi.load_library()
    bad = [(-1, 24), (32, 0), (32, -5), (65536, 1), (40000, 60000)]

    def refused():
        for w, h in bad:
            rc_ = lib.avt_set_occlusion_render(ctx.h, w, h, 128.0, 128.0, 16.0, 12.0)
            assert rc_ != 0 and b"avt_set_occlusion_render" in lib.avt_last_error(), (w, h)
    refused()
    assert np.array_equal(ctx.visibility(s["cloud"], True), s["backface"])          # still off
    ctx.set_occlusion_render(oc.S32, oc.K32)
    assert np.array_equal(ctx.visibility(s["cloud"], True), s["visible"])
    refused()
    assert np.array_equal(ctx.visibility(s["cloud"], True), s["visible"])           # still on, same camera
    assert np.array_equal(ctx.visibility(s["cloud"], False), np.ones(8, np.uint8))
    ctx.set_occlusion_render(None)
    assert np.array_equal(ctx.visibility(s["cloud"], True), s["backface"])
    with pytest.raises(AvtError):
        ctx.get_visibility(0)                                                       # no optimize call has run


SOUPS = [(85, (32, 24)), (256, (32, 24)), (257, (32, 24)), (255, (32, 24)), (16385, (32, 24)), (85, (1, 1)), (85, (257, 1)), (85, (33, 17))]


@pytest.mark.parametrize("F,size", SOUPS, ids=[f"F{F}-{w}x{h}" for F, (w, h) in SOUPS])
def test_triangle_soup_equals_the_helper(F, size):
    """Random triangles of both windings, many outside the image: 255 / 256 / 257 faces (a workgroup of k_occ_faces / k_rend_cover),
    16 385 faces (above REND_SORT_CAP: k_paint_rank + k_rend_scatter), images 1 x 1, 257 x 1 and 33 x 17; V = 3 F is no multiple
    of 4 for the odd face counts."""
    k, sz = rc.cam(*size, f=64.0)
    cloud = np.array(rc._soup(k, sz, F, 5))
    mesh = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    want = occ.visible(cloud, mesh, k, *sz)
    bf = occ.backface(cloud, mesh)
    assert (want <= bf).all()
    if size != (1, 1):
        assert want.any() and (want < bf).any()          # the input shows the rule: seen faces, and front-facing faces without a pixel
    ctx = _ctx(rc.tiny_model(cloud, mesh))
    ctx.set_occlusion_render(sz, k)
    got = ctx.visibility(cloud, True)
    assert np.array_equal(got, want), (F, size, int((got != want).sum()))
    ctx.set_occlusion_render(None)
    assert np.array_equal(ctx.visibility(cloud, True), bf)


# ---- inside optimize() ------------------------------------------------------------------------------------------------------------------------
CAM = dict(fx=100.0, fy=100.0, cx=80.0, cy=60.0, width=160, height=120)      # the avatar at 2.3 - 2.5 m is about 70 of the 120 rows tall
SIZES = [(255, 257), (1025, 1023), (9036, 2049)]
# frames per call, tuning: one frame; two frames (one frame per group: the second launch has fb.f0 = 1); 33 frames in one launch (past
# vis_frame_min = 32, still the few-frame nearest neighbour: the scatter rides in k_occ_faces); 33 frames as two groups (fb.f0 = 17) with
# the throughput nearest neighbour (k_compact takes the scatter and reads fb.visible)
SHAPES = {"1": (1, {}), "2": (2, {}), "33": (33, {}), "33-split": (33, dict(groups=2, nn_force_part=1))}


@pytest.fixture(scope="module")
def gmodels(smpl):
    from avatar_amd import api
    made = {}

    def get(V, F):
        if (V, F) not in made:
            m = hm.resized(smpl, V, F)
            made[(V, F)] = (m, api.AvatarModel(m))
        return made[(V, F)]
    return get


def _frames(smpl, nf, first=40):
    gt = [synth.sample_ground_truth(smpl, first + f) for f in range(nf)]
    st = [synth.perturb_start(*gt[f], first + f) for f in range(nf)]
    from avatar_amd import api
    w = np.array([g[0] for g in gt]); p = np.array([g[1] for g in gt]); R = np.array([g[2] for g in gt])
    return (w, p, R), (np.array([s[1] for s in st]), np.array([api.rot_to_quat(s[2]) for s in st]), np.array([s[0] for s in st]))


def _expected(model, nn_ctx, cloud, data, labels):
    vis = occ.visible(cloud, np.asarray(model["f"]), CAM, CAM["width"], CAM["height"])
    return vis, nn_ctx.nn(cloud, vis, data, labels)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("size", SIZES, ids=[hm.resized_name(*s) for s in SIZES])
def test_first_icp_iteration(smpl, gmodels, size, shape):
    """icp_iters = 1, max_iters_per_icp = 0 on frames of different poses rendered by avt_synth_render_frames at 160 x 120: for every frame
    avt_get_visibility equals the helper on the cloud avt_get_posed returns, and avt_get_correspondences equals avt_nn on that cloud with
    the helper's flags; once per data-term form; the same call issued again (the cached graph) gives identical flags."""
    from avatar_amd import api
    m, gm = gmodels(*size)
    nf, tun = SHAPES[shape]
    (w, p, R), (p0, q0, w0) = _frames(smpl, nf)
    ctx = _ctx(gm, CAM["width"] * CAM["height"], nf, **tun)
    nn_ctx = _ctx(gm, CAM["width"] * CAM["height"], 1)
    ctx.set_occlusion_render((CAM["width"], CAM["height"]), CAM)
    opt = Options.demo(icp_iters=1, max_iters_per_icp=0)
    want = None
    for form in (api.Context.DATA_TERM_ROWS, api.Context.DATA_TERM_MOMENTS):
        ctx.set_data_term(form)
        n = ctx.render_frames(w, p, R, CAM)
        assert (n > 100).all()                       # (the 2049 faces of the largest model are a seventh of its surface)
        frames = [ctx.frame_download(f) for f in range(nf)]
        ctx.state_upload(p0, q0, w0)
        ctx.optimize_resident(opt)
        vis = [ctx.get_visibility(f) for f in range(nf)]
        corr = [ctx.correspondences(f, int(n[f])) for f in range(nf)]
        clouds = [ctx.posed(f)[0] for f in range(nf)]
        if want is None:          # the head of the ICP iteration does not depend on the form: one reference for both
            want = [_expected(m, nn_ctx, clouds[f], *frames[f]) for f in range(nf)]
            hidden = sum(int((occ.backface(clouds[f], np.asarray(m["f"])) != want[f][0]).sum()) for f in range(nf))
            print(f"{hm.resized_name(*size)} x {shape}: {hidden} vertices hidden by the render over {nf} frames")
        bad = [f for f in range(nf) if not np.array_equal(vis[f], want[f][0])]
        assert not bad, (size, shape, form, "flags differ on frames", bad, int((vis[bad[0]] != want[bad[0]][0]).sum()))
        bad = [f for f in range(nf) if not np.array_equal(corr[f], want[f][1])]
        assert not bad, (size, shape, form, "correspondences differ on frames", bad)
        ctx.state_upload(p0, q0, w0)
        ctx.optimize_resident(opt)
        assert all(np.array_equal(ctx.get_visibility(f), vis[f]) for f in range(nf)), (size, shape, form, "replay")


@pytest.mark.parametrize("size", SIZES[:2], ids=[hm.resized_name(*s) for s in SIZES[:2]])
def test_second_icp_iteration(smpl, gmodels, size):
    """One resident call with icp_iters = 2 on two copies of one frame, budgets [1, 2]: frame 0 is left as ICP iteration 0 left it, so its
    posed cloud is the cloud ICP iteration 1 of frame 1 started from - frame 1's flags and correspondences equal the helper's and avt_nn's
    on it (k_lbs cleared the flags between the iterations: nothing of iteration 0 survives)."""
    m, gm = gmodels(*size)
    (w, p, R), (p0, q0, w0) = _frames(smpl, 1, first=47)
    two = lambda a: np.concatenate([a, a])
    ctx = _ctx(gm, CAM["width"] * CAM["height"], 2)
    nn_ctx = _ctx(gm, CAM["width"] * CAM["height"], 1)
    ctx.set_occlusion_render((CAM["width"], CAM["height"]), CAM)
    n = ctx.render_frames(two(w), two(p), two(R), CAM)
    data, labels = ctx.frame_download(1)
    ctx.state_upload(two(p0), two(q0), two(w0))
    ctx.optimize_resident_budgets(Options.demo(icp_iters=2, max_iters_per_icp=3), [1, 2])
    cloud0, cloud1 = ctx.posed(0)[0], ctx.posed(1)[0]
    assert not np.array_equal(cloud0, cloud1)                      # frame 1 went on
    vis, corr = _expected(m, nn_ctx, cloud0, data, labels)
    assert np.array_equal(ctx.get_visibility(1), vis)
    assert np.array_equal(ctx.correspondences(1, int(n[1])), corr)


# ---- full size ------------------------------------------------------------------------------------------------------------------------------
K4A = synth.K4A_INTRIN
ARM_POSE = {16: (0.0, 1.8, 0.0), 18: (0.0, 0.0, -1.5), 17: (0.0, -1.8, 0.0), 19: (0.0, 0.0, 1.5)}     # both forearms in front of the torso


def _arm_pose():
    R = np.tile(np.eye(3), (24, 1, 1))
    R[0] = synth.rodrigues(np.array([0.0, np.pi, 0.0]))
    for j, aa in ARM_POSE.items():
        R[j] = synth.rodrigues(np.array(aa))
    return np.zeros(10), np.array([0.0, 0.0, 2.4]), R


@pytest.fixture(scope="module")
def arm(smpl):
    """the arm pose, checked on the CPU first: the render hides front-facing vertices (at least 100 of them)"""
    w, p, R = _arm_pose()
    verts = synth.pose_vertices(smpl, w, p, R)
    mesh = np.asarray(smpl["f"])
    vis, bf = occ.visible(verts, mesh, K4A, K4A["width"], K4A["height"]), occ.backface(verts, mesh)
    assert (vis <= bf).all() and int(bf.sum()) - int(vis.sum()) >= 100
    return w, p, R, verts


def test_full_size_arm_in_front_of_the_torso(smpl, gmodel, arm):
    """The synthetic SMPL model, one frame, 1280 x 720, K4A intrinsics, the pose as the start state: the flags equal the helper's on the
    posed cloud, are a subset of the back-face flags and strictly fewer."""
    from avatar_amd import api
    w, p, R, verts = arm
    mesh = np.asarray(smpl["f"])
    ctx = _ctx(gmodel, K4A["width"] * K4A["height"] // 4, 1)
    n = ctx.render_frames(w, p, R, K4A)
    q = api.rot_to_quat(R)
    opt = Options.demo(icp_iters=1, max_iters_per_icp=0)
    ctx.state_upload(p[None], q[None], w[None])
    ctx.optimize_resident(opt)
    bf = ctx.get_visibility(0)
    ctx.set_occlusion_render((K4A["width"], K4A["height"]), K4A)
    ctx.state_upload(p[None], q[None], w[None])
    ctx.optimize_resident(opt)
    vis = ctx.get_visibility(0)
    cloud = ctx.posed(0)[0]
    assert np.array_equal(bf, occ.backface(cloud, mesh))
    assert np.array_equal(vis, occ.visible(cloud, mesh, K4A, K4A["width"], K4A["height"]))
    assert (vis <= bf).all() and int(vis.sum()) < int(bf.sum())
    print(f"arm pose: {int(bf.sum())} front-facing vertices, {int(bf.sum()) - int(vis.sum())} of them hidden by the render")


# ---- facades --------------------------------------------------------------------------------------------------------------------------------
def test_python_facades_reach_the_context(smpl, gmodel, arm):
    """renderOcclusion of api.AvatarOptimizer and render_occlusion of the trackers: avt_get_visibility differs from the back-face flags
    on the arm pose (and is a subset of them)."""
    from avatar_amd import api, tracker
    w, p, R, verts = arm
    pm = synth.identity_part_map()
    size = (K4A["width"], K4A["height"])
    xyz, mask, _ = synth.render_images(smpl, verts, pm)
    data, labels = tracker.subsample(xyz, mask, None, 6, 24)
    flags = {}
    for on in (False, True):
        ava = api.Avatar(gmodel)
        ava.w, ava.p, ava.r = w.copy(), p.copy(), R.copy()
        ava.update()
        opt = api.AvatarOptimizer(ava, K4A, size, 24, pm, max_points=len(labels))
        opt.renderOcclusion = on
        opt.maxItersPerICP = 0
        opt.optimize(data, labels, 1)
        flags[on] = opt.ctx.get_visibility(0)
    assert (flags[True] <= flags[False]).all() and int(flags[True].sum()) < int(flags[False].sum())
    tr = tracker.MultiFrameTracker.create(gmodel, 1, 24, pm, max_points=len(labels), interval=6, frame_icp_iters=1, max_iters_per_icp=0,
                                          render_occlusion=(K4A, size))
    assert tr.renderOcclusion is not None
    tr.p[0], tr.q[0], tr.w[0] = p, api.rot_to_quat(R), w
    tr.streams[0].reinit = tr.streams[0].firstTime = False        # a warm stream: the fit starts from the arm pose
    assert tr.process([(xyz, mask, None)]) == [True]
    on = tr.ctx.get_visibility(0)
    tr.set_render_occlusion(None)
    assert tr.renderOcclusion is None and tr.process([(xyz, mask, None)]) == [True]
    off = tr.ctx.get_visibility(0)
    assert (on <= off).all() and int(on.sum()) < int(off.sum())
    ft = tracker.FrameTracker(opt, render_occlusion=False)
    assert opt.renderOcclusion is False and ft.opt is opt


def test_cpp_facade_reaches_the_context(smpl, arm, tmp_path):
    """tests/cpp/occlusion_demo.cpp: ark::AvatarOptimizer::renderOcclusion on the arm pose - fewer visible vertices than with the
    back-face test alone, none that the back-face test hides."""
    import struct
    from avatar_amd import tracker
    from test_gpu_facade import write_model_dir
    exe = os.path.join(HERE, "cpp", "occlusion_demo")
    assert os.path.exists(exe), "tests/cpp/occlusion_demo is not built (make -C avatar_amd/csrc facade)"
    w, p, R, verts = arm
    xyz, mask, _ = synth.render_images(smpl, verts, synth.identity_part_map())
    data, labels = tracker.subsample(xyz, mask, None, 6, 24)
    mdir, fpath = str(tmp_path / "model"), str(tmp_path / "frame.bin")
    write_model_dir(smpl, mdir)
    with open(fpath, "wb") as f:
        f.write(struct.pack("i", len(labels)))
        f.write(np.ascontiguousarray(data, np.float64).tobytes()); f.write(np.ascontiguousarray(labels, np.int32).tobytes())
        f.write(w.astype(np.float64).tobytes()); f.write(p.astype(np.float64).tobytes())
        f.write(np.ascontiguousarray(np.transpose(R, (0, 2, 1))).tobytes())      # column-major 3x3 blocks
    out = subprocess.run([exe, mdir, fpath], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "occlusion_demo ok" in out.stdout, out.stdout
