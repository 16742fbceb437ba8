"""ark::AvatarRenderer on the GPU (include/avt_render.h, avatar_amd/render.py) against the CPU restatement of the reference's renderer
(tests/cpp/avatar_renderer_restatement.cpp): depth, part mask, Lambert overlay, face ids, projections and the painter order, all
array_equal."""
import os
import struct
import subprocess

import numpy as np
import pytest

from avatar_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K4A = synth.K4A_INTRIN


def _rst():
    import avatar_render_restatement as rst
    return rst


@pytest.fixture(scope="module")
def posed(smpl, gmodel):
    """posed clouds and joints of seeds 0..63 (the first four are the painter test's poses)"""
    from avatar_amd import api
    gts = [synth.sample_ground_truth(smpl, s) for s in range(64)]
    W = np.array([g[0] for g in gts]); P = np.array([g[1] for g in gts]); R = np.array([g[2] for g in gts])
    ctx = api.Context(gmodel, 24, synth.identity_part_map(), 1000, 64, device=0)
    cloud, jp, _ = ctx.lbs_update(W, P, R)
    return cloud, jp


def _vp(smpl, part_map=None):
    mj = synth.main_joint(smpl)
    return mj if part_map is None else np.asarray(part_map)[mj]


def _check_image(got, ref, proj, name, pm_vp, intrin, size):
    rst = _rst()
    W, H = size
    for i, (cl, jp) in enumerate(ref):
        o = rst.render(cl, smpl_faces[0], intrin, W, H, vertex_part=pm_vp, joints=jp)
        g = got[i]
        for k in ("depth", "mask", "lambert", "faces"):
            assert np.array_equal(g[k], o[k]), f"{name} image {i}: {k} differs at {(g[k] != o[k]).sum()} pixels"
        p = proj[i]
        assert np.array_equal(p["points"], o["points"]) and np.array_equal(p["joints"], o["joints"]), f"{name} image {i}: projections"
        assert np.array_equal(p["keys"], o["keys"]) and np.array_equal(p["ordered"], o["ordered"]), f"{name} image {i}: ordered faces"
    return o


smpl_faces = [None]


@pytest.fixture(autouse=True, scope="module")
def _faces(smpl):
    smpl_faces[0] = np.ascontiguousarray(smpl["f"], np.int32)


def _render_all(rend, n):
    from avatar_amd import render
    rend.run(render.ALL)
    return [rend.download(i) for i in range(n)], [rend.projection(i) for i in range(n)]


def test_seeded_poses_all_outputs_match_the_restatement(smpl, gmodel, posed):
    from avatar_amd import render
    cloud, jp = posed
    n = 4
    rend = render.Renderer(gmodel, K4A["width"], K4A["height"], K4A, n)
    rend.upload(cloud[:n], jp[:n])
    got, proj = _render_all(rend, n)
    last = _check_image(got, list(zip(cloud[:n], jp[:n])), proj, "seeded", _vp(smpl), K4A, (K4A["width"], K4A["height"]))
    assert (last["lambert"] > 0).sum() > 15000 and (last["faces"] >= 0).sum() > 15000
    # tie insensitivity: the fixtures do not depend on how std::sort orders equal keys
    rst = _rst()
    for i in range(n):
        a = rst.render(cloud[i], smpl_faces[0], K4A, K4A["width"], K4A["height"], vertex_part=_vp(smpl), stable=False)
        for k in ("depth", "mask", "lambert"):
            assert np.array_equal(a[k], got[i][k]), f"seed {i}: {k} depends on the order of tied keys"


def test_part_map_and_rank_ordering(smpl, gmodel, posed):
    """renderPartMask's part_map, and the O(F^2) rank count giving the same positions and images as the sort"""
    from avatar_amd import render
    cloud, jp = posed
    pm = (np.arange(24) * 7) % 5
    rend = render.Renderer(gmodel, 641, 479, K4A, 3)
    rend.set_part_map(pm)
    rend.upload(cloud[4:7], jp[4:7])
    got, proj = _render_all(rend, 3)
    _check_image(got, list(zip(cloud[4:7], jp[4:7])), proj, "part map", _vp(smpl, pm), K4A, (641, 479))
    rend.set_ordering(render.ORDER_RANK)
    got2, proj2 = _render_all(rend, 3)
    for i in range(3):
        assert np.array_equal(proj[i]["pos"], proj2[i]["pos"])
        for k in got[i]:
            assert np.array_equal(got[i][k], got2[i][k])


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (641, 479)])
def test_odd_sizes_and_partly_off_screen(smpl, gmodel, posed, size):
    from avatar_amd import render
    cloud, jp = posed
    intr = dict(fx=K4A["fx"] * size[0] / 1280.0 * 1.7, fy=K4A["fy"] * size[1] / 720.0 * 1.7, cx=size[0] * 0.5 - 0.25, cy=size[1] * 0.5 + 0.125)
    shifted = cloud[8:10].copy()
    shifted[1, :, 0] += 0.45                                   # the second avatar is partly off the right edge
    shifted[1, :, 1] -= 0.35                                   # ... and the bottom edge
    jps = jp[8:10].copy()
    jps[1, :, 0] += 0.45; jps[1, :, 1] -= 0.35
    rend = render.Renderer(gmodel, size[0], size[1], intr, 2)
    rend.upload(shifted, jps)
    got, proj = _render_all(rend, 2)
    _check_image(got, list(zip(shifted, jps)), proj, f"{size}", _vp(smpl), intr, size)
    if size == (641, 479):
        f = got[1]["faces"]
        assert (f[:, -1] >= 0).any() or (f[-1, :] >= 0).any(), "the shifted avatar should cross the border"


def test_batch_of_64_equals_64_single_calls(smpl, gmodel, posed):
    from avatar_amd import render
    cloud, jp = posed
    W, H = K4A["width"], K4A["height"]
    rend = render.Renderer(gmodel, W, H, K4A, 64)
    rend.upload(cloud, jp)
    got, proj = _render_all(rend, 64)
    one = render.Renderer(gmodel, W, H, K4A, 1)
    for i in range(64):
        one.upload(cloud[i], jp[i])
        g1, p1 = _render_all(one, 1)
        for k in got[i]:
            assert np.array_equal(got[i][k], g1[0][k]), f"image {i}: batched {k} differs from the single call"
        for k in proj[i]:
            assert np.array_equal(proj[i][k], p1[0][k]), f"image {i}: batched {k} differs from the single call"
    # and a few of them against the restatement
    _check_image([got[i] for i in (13, 40, 63)], [(cloud[i], jp[i]) for i in (13, 40, 63)], [proj[i] for i in (13, 40, 63)], "batch",
                 _vp(smpl), K4A, (W, H))


def _frames(smpl, seeds):
    from avatar_amd import api
    datas, labels, p0, q0, w0 = [], [], [], [], []
    for s in seeds:
        fr = synth.make_frame(smpl, s)
        sel = np.arange(0, len(fr["labels"]), 4)
        datas.append(fr["data"][sel]); labels.append(fr["labels"][sel])
        w, p, R = fr["start"]
        p0.append(p); q0.append(api.rot_to_quat(R)); w0.append(w)
    return datas, labels, np.array(p0), np.array(q0), np.array(w0)


def test_render_from_context_after_optimize(smpl, gmodel):
    """Rendering a context's frames on the device equals rendering avt_get_posed's clouds, and leaves the context as it was: the
    next optimize is bit-identical to one run without rendering."""
    from avatar_amd import api, render
    from avatar_amd.capi import Options
    opt = Options.demo(max_iters_per_icp=4)
    datas, labels, p0, q0, w0 = _frames(smpl, (0, 3, 5))
    outs = []
    for with_render in (False, True):
        ctx = api.Context(gmodel, 24, synth.identity_part_map(), 40000, 3, device=0)
        p1, q1, w1, _ = ctx.optimize_batch(datas, labels, opt, p0, q0, w0)
        if with_render:
            rend = render.Renderer(gmodel, K4A["width"], K4A["height"], K4A, 3)
            rend.from_context(ctx, [2, 0, 1])
            got, proj = _render_all(rend, 3)
            host = render.Renderer(gmodel, K4A["width"], K4A["height"], K4A, 3)
            posed = [ctx.posed(f) for f in (2, 0, 1)]
            host.upload(np.array([c for c, _, _ in posed]), np.array([j for _, j, _ in posed]))
            ref, rproj = _render_all(host, 3)
            for i in range(3):
                for k in got[i]:
                    assert np.array_equal(got[i][k], ref[i][k]), f"frame image {i}: {k} from the context differs from the posed cloud's"
                for k in proj[i]:
                    assert np.array_equal(proj[i][k], rproj[i][k])
                assert (got[i]["lambert"] > 0).sum() > 15000
            _check_image(got[:1], [(posed[0][0], posed[0][1])], proj[:1], "context", _vp(smpl), K4A, (K4A["width"], K4A["height"]))
        p2, q2, w2, st = ctx.optimize_batch(datas, labels, opt, p1, q1, w1)
        outs.append((p2, q2, w2, [s.final_cost for s in st], [ctx.cloud(f) for f in range(3)]))
    a, b = outs
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)), "rendering changed a later optimize"


def test_multi_tracker_render_streams(smpl, gmodel):
    """MultiFrameTracker.render: the selected streams' last fits rendered from the context equal the posed clouds' render"""
    from avatar_amd import render, tracker
    mt = tracker.MultiFrameTracker.create(gmodel, 3, max_points=60000)
    frames = []
    for s in (1, 2, 4):
        w, p, R = synth.sample_ground_truth(smpl, s, use_gmm=False)
        xyz, mask, _ = synth.render_images(smpl, synth.pose_vertices(smpl, 0.5 * w, p, R), synth.identity_part_map())
        ys, xs = np.nonzero(mask != 255)
        frames.append((xyz, mask, (ys.min(), xs.min(), ys.max(), xs.max())))
    assert all(mt.process(frames))
    intr = dict(fx=300.0, fy=300.0, cx=160.0, cy=120.0)
    imgs = mt.render([2, 0], (320, 240), intr, render.LAMBERT | render.PART_MASK)
    host = render.Renderer(gmodel, 320, 240, intr, 1)
    for i, s in enumerate((2, 0)):
        c, j, _ = mt.posed(s)
        host.upload(c, j)
        host.run(render.LAMBERT | render.PART_MASK)
        ref = host.download(0, render.LAMBERT | render.PART_MASK)
        assert np.array_equal(imgs[i]["lambert"], ref["lambert"]) and np.array_equal(imgs[i]["mask"], ref["mask"])
        assert (ref["lambert"] > 0).sum() > 500


def test_render_demo_equals_python(smpl, gmodel, tmp_path):
    """tests/cpp/render_demo (the facade, ark::AvatarRenderer) writes the images the Python mirror renders"""
    from avatar_amd import api, render
    from tests.test_gpu_facade import write_model_dir
    exe = os.path.join(HERE, "cpp", "render_demo")
    assert os.path.exists(exe), "tests/cpp/render_demo not built (make -C avatar_amd/csrc facade)"
    mdir = str(tmp_path / "model")
    write_model_dir(smpl, mdir)
    w, p, R = synth.sample_ground_truth(smpl, 9)
    W, H = 643, 481
    intr = dict(fx=400.5, fy=401.25, cx=321.5, cy=240.75)
    spath, opath = str(tmp_path / "state.bin"), str(tmp_path / "out.bin")
    with open(spath, "wb") as f:
        f.write(np.asarray(w, np.float64).tobytes()); f.write(np.asarray(p, np.float64).tobytes())
        f.write(np.ascontiguousarray(np.asarray(R, np.float64).transpose(0, 2, 1)).tobytes())     # column-major 3x3 per joint
        f.write(struct.pack("2i", W, H)); f.write(np.array([intr["fx"], intr["fy"], intr["cx"], intr["cy"]], np.float32).tobytes())
    r = subprocess.run([exe, mdir, spath, opath], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "the avatar has no posed cloud yet" in r.stderr
    V, J, F = gmodel.numPoints(), gmodel.numJoints(), gmodel.numFaces()
    buf = open(opath, "rb").read()
    off = 0

    def take(dt, n):
        nonlocal off
        a = np.frombuffer(buf, dt, n, off)
        off += a.nbytes
        return a
    cloud = take(np.float64, 3 * V).reshape(V, 3)
    depth = take(np.float32, W * H).reshape(H, W); mask = take(np.uint8, W * H).reshape(H, W)
    lam = take(np.uint8, W * H).reshape(H, W); faces = take(np.int32, W * H).reshape(H, W)
    pts = take(np.float32, 2 * V).reshape(V, 2); jts = take(np.float32, 2 * J).reshape(J, 2)
    keys = take(np.float32, F); ordered = take(np.int32, 3 * F).reshape(F, 3)
    assert off == len(buf)
    ava = api.Avatar(gmodel)
    ava.w, ava.p, ava.r = np.asarray(w, np.float64), np.asarray(p, np.float64), np.asarray(R, np.float64)
    ava.update()
    assert np.array_equal(ava.cloud, cloud)
    ar = render.AvatarRenderer(ava, intr)
    assert np.array_equal(ar.renderLambert((W, H)), lam)
    assert np.array_equal(ar.renderDepth((W, H)), depth)
    assert np.array_equal(ar.renderPartMask((W, H)), mask)
    assert np.array_equal(ar.renderFaces((W, H)), faces)
    assert np.array_equal(ar.getProjectedPoints(), pts) and np.array_equal(ar.getProjectedJoints(), jts)
    k2, o2 = ar.getOrderedFaces()
    assert np.array_equal(k2, keys) and np.array_equal(o2, ordered)
    assert (lam > 0).sum() > 1000


# ---- hand-built meshes (the CPU known answers of tests/test_avatar_render_cpu.py) on the device, with the per-vertex shading
HAND_INTR = dict(fx=100.0, fy=100.0, cx=10.0, cy=40.0)
_T = 0.005 / np.sqrt(1 - 0.005 ** 2)
HAND_MESHES = {
    "one triangle": ([[0, 0, 2.0], [0.5, 0, 2.0], [0, 0.5, 2.0]], [[0, 1, 2]], (40, 48)),
    "two overlapping": ([[0, 0, 3.0], [0.9, 0, 3.0], [0, 0.9, 3.0], [0, 0, 2.0], [0.3, 0, 2.0], [0, 0.3, 2.0]], [[3, 4, 5], [0, 1, 2]], (48, 48)),
    "shared-vertex quad": ([[0, 0, 2.0], [0.4, 0, 2.0], [0, 0.4, 2.0], [0.4, 0.4, 2.3]], [[0, 1, 2], [1, 3, 2]], (64, 64)),
    "almost edge-on": ([[1.0, 0, 2.0], [1.0, 0.5, 2.0], [1.0 + _T, 0, 3.0]], [[0, 1, 2]], (70, 48)),
    "coincident, opposite winding": ([[0, 0, 2.0], [0.5, 0, 2.0], [0, 0.5, 2.0], [0.6, 0, 2.0], [0.9, 0, 2.0], [0.9, 0.3, 2.0]],
                                     [[0, 1, 2], [0, 2, 1], [3, 4, 5]], (64, 48)),
    "crossing the border": ([[-0.3, 0, 2.0], [0.5, 0.1, 2.2], [0.1, 0.9, 2.1]], [[0, 1, 2]], (30, 40)),
}


from avatar_render_cases import tiny_model as _tiny_model      # the one-joint model recipe, shared with the edge cases


@pytest.mark.parametrize("name", list(HAND_MESHES))
def test_hand_built_meshes_on_the_device(name):
    from avatar_amd import render
    cloud, mesh, (W, H) = HAND_MESHES[name]
    cloud = np.asarray(cloud, np.float64)
    rend = render.Renderer(_tiny_model(cloud, mesh), W, H, HAND_INTR, 1)
    rend.upload(cloud)
    rend.run(render.ALL)
    g, p = rend.download(0), rend.projection(0, joints=False)
    normals, lam_v = rend.vertex_shading(0)
    o = _rst().render(cloud, mesh, HAND_INTR, W, H)
    for k in ("depth", "mask", "lambert", "faces"):
        assert np.array_equal(g[k], o[k]), f"{name}: {k} differs at {(g[k] != o[k]).sum()} pixels"
    for k in ("points", "keys", "ordered"):
        assert np.array_equal(p[k], o[k]), f"{name}: {k}"
    assert np.array_equal(normals, o["vnormal"], equal_nan=True) and np.array_equal(lam_v, o["lambert_v"], equal_nan=True), name
    if name == "coincident, opposite winding":
        assert np.isnan(normals[:3]).all() and np.isnan(lam_v[:3]).all()   # zero sums divided by a zero norm ...
        assert (g["faces"][25:39, 11:20] >= 0).all() and (g["lambert"][:, :37] == 0).all()   # ... painted, and NaN gives 0
        assert (g["lambert"][:, 38:] > 0).sum() > 20
    if name == "almost edge-on":
        assert (g["faces"] >= 0).sum() > 50 and (g["lambert"] == 0).all() and (g["depth"] == 0).all()
    if name == "crossing the border":
        assert g["lambert"][:, 0].any() and g["lambert"][:, -1].any() and g["lambert"][0, :].any()


def test_vertex_shading_of_seeded_poses(smpl, gmodel, posed):
    """the per-vertex normals (summed in painter order) and Lambert values of SMPL poses, bit for bit"""
    from avatar_amd import render
    cloud, jp = posed
    rend = render.Renderer(gmodel, 64, 48, K4A, 4)
    rend.upload(cloud[20:24])
    rend.run(render.LAMBERT)
    for i in range(4):
        n, lam = rend.vertex_shading(i)
        o = _rst().render(cloud[20 + i], smpl_faces[0], K4A, 64, 48)
        assert np.array_equal(n, o["vnormal"], equal_nan=True), f"image {i}: {(n != o['vnormal']).any(1).sum()} vertex normals differ"
        assert np.array_equal(lam, o["lambert_v"], equal_nan=True), f"image {i}: per-vertex Lambert values differ"


def test_cpp_multi_tracker_render_matches_python(smpl, gmodel, tmp_path):
    """tests/cpp/multi_render_demo: ark::MultiFrameTracker::render and renderedDepth / PartMask / Lambert / Faces of two streams
    equal the Python renderer on the posed clouds the C++ tracker reports"""
    from avatar_amd import render
    from tests.test_gpu_facade import write_model_dir
    from tests.test_gpu_tracker import write_sequence
    exe = os.path.join(HERE, "cpp", "multi_render_demo")
    assert os.path.exists(exe), "tests/cpp/multi_render_demo not built (make -C avatar_amd/csrc facade)"
    mdir = str(tmp_path / "model")
    write_model_dir(smpl, mdir)
    seqs = []
    for s in (1, 2, 4):
        w, p, R = synth.sample_ground_truth(smpl, s, use_gmm=False)
        xyz, mask, _ = synth.render_images(smpl, synth.pose_vertices(smpl, 0.5 * w, p, R), synth.identity_part_map())
        ys, xs = np.nonzero(mask != 255)
        path = str(tmp_path / f"seq{s}.bin")
        write_sequence(path, [(xyz, mask, (ys.min(), xs.min(), ys.max(), xs.max()))], 12, 3, 6, 1000)
        seqs.append(path)
    W, H = 321, 243
    out = str(tmp_path / "out.bin")
    r = subprocess.run([exe, mdir, out, str(W), str(H), "2,0"] + seqs, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    V, J = gmodel.numPoints(), gmodel.numJoints()
    buf = open(out, "rb").read()
    intr = dict(fx=np.float32(0.5 * W), fy=np.float32(0.5 * W), cx=np.float32(0.5 * W - 0.5), cy=np.float32(0.5 * H + 0.25))
    host = render.Renderer(gmodel, W, H, intr, 1)
    off = 0
    for _ in range(2):
        def take(dt, n):
            nonlocal off
            a = np.frombuffer(buf, dt, n, off)
            off += a.nbytes
            return a
        cloud = take(np.float64, 3 * V).reshape(V, 3); joints = take(np.float64, 3 * J).reshape(J, 3)
        depth = take(np.float32, W * H).reshape(H, W); parts = take(np.uint8, W * H).reshape(H, W)
        lam = take(np.uint8, W * H).reshape(H, W); faces = take(np.int32, W * H).reshape(H, W)
        host.upload(cloud, joints)
        host.run(render.ALL)
        ref = host.download(0)
        assert np.array_equal(depth, ref["depth"]) and np.array_equal(parts, ref["mask"])
        assert np.array_equal(lam, ref["lambert"]) and np.array_equal(faces, ref["faces"])
        assert (lam > 0).sum() > 500
    assert off == len(buf)
