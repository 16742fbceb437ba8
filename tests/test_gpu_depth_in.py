"""Depth images in, on the GPU (include/avt_bgsub.h's depth entries, k_bgs_backproject in avatar_amd/csrc/avt_bgsub.hip): the
back-projection against avatar_amd.depth.depth_to_xyz, the background subtraction from depth against the one from the XYZ map
and against tests/bgsub_restatement.py, the batch form and its hand-over to the forest, the error paths, and the trackers from
depth images end to end.  Every comparison is exact (uint8, int, float bit patterns); where both sides hold a NaN only NaN-ness
is compared (0 * inf has no agreed sign or payload across x86 and the GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bgsub_restatement as R
import bgsub_scenes as S
from avatar_amd import api, bgsub, capi, rtree, synth
from avatar_amd.depth import CameraIntrin, depth_to_xyz
from avatar_amd.tracker import FrameTracker, MultiFrameTracker
from test_depth_in_cpu import SPECIAL, same_bits
from test_gpu_bgsub import LIVE, check, run_one
from test_gpu_label_batch import _policy, tracker_inputs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "forest_small.srtr")
F = np.float32
CAMS = np.array([(60.0, 60.5, 4.0, 2.5), (525.25, 524.75, 31.5, 17.0), (606.438, 606.351, 637.294, 366.992)], F)
# fewer than four pixels (scalar form only); exactly one vector; a tail and an odd N, so images 1 and 2 start unaligned;
# exactly 1024 pixels (one workgroup's worth); 1025; the suite's small image; the widest column index with N % 4 == 2
SHAPES = [(1, 1), (1, 3), (3, 1), (2, 2), (1, 5), (7, 9), (16, 64), (5, 205), (37, 53), (2, 65535)]


def depth_images(n, rows, cols, seed):
    """uniform 0.3-6 m with the special values of the CPU test scattered by seed (each at about one pixel in fifty)"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.3, 6.0, (n, rows * cols)).astype(F)
    for i in range(n):
        for v in SPECIAL:
            z[i, rng.integers(0, rows * cols, max(1, rows * cols // 50))] = v
    return z.reshape(n, rows, cols)


def check_backprojection(rows, cols, n, seed):
    z = depth_images(n, rows, cols, seed)
    cams = CAMS[:n]
    if cols > 4:                                                # c - cx == 0 meets inf
        z[:, 0, 4] = np.inf
    b = bgsub.BGSubtractor(np.zeros((n, rows, cols, 3), F))
    b.upload_depth(z, cams)
    for i in range(n):
        assert same_bits(b.xyz(i), depth_to_xyz(z[i], cams[i])), (rows, cols, i)
    # the same into the backgrounds (a background past the first starts unaligned when rows * cols is odd): against its own
    # background every valid pixel is at distance 0, the few NaN ones form components too small to keep
    for i in range(n):
        b.set_background_depth(z[i], cams[i], i)
    b.upload_depth(z, cams)
    b.run_resident()
    for i in range(n):
        assert (b.download(i).mask == 255).all(), (rows, cols, i)
        assert same_bits(b.background[i] if n > 1 else b.background, depth_to_xyz(z[i], cams[i]))
    # ... and they are what a run sees: one pixel moved away from the background is the only candidate
    if rows * cols >= 4:
        z2 = np.full((n, rows, cols), 2.0, F)
        for i in range(n):
            b.set_background_depth(z2[i], cams[i], i)
        ref = bgsub.BGSubtractor(np.stack([depth_to_xyz(z2[i], cams[i]) for i in range(n)]))
        z2[:, rows // 2, cols // 2] = 1.0
        b.upload_depth(z2, cams)
        b.run_resident()
        want = ref.run_batch(np.stack([depth_to_xyz(z2[i], cams[i]) for i in range(n)]))
        for i in range(n):
            res = b.download(i)
            assert np.array_equal(res.mask, want[i].mask) and res.fg_count == want[i].fg_count
            assert same_bits(res.masked_depth, want[i].masked_depth)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_backprojection_bit_for_bit(shape):
    check_backprojection(shape[0], shape[1], 3, 1000 + shape[0] * 7 + shape[1])


def test_backprojection_at_720p():
    check_backprojection(720, 1280, 1, 5)


SCENES = [("blocky_100x130", lambda: S.blocky_scene(100, 130, 7), 36, 1465), ("blocky_37x53", lambda: S.blocky_scene(37, 53, 3), 3, 484),
          ("u", S.u_scene, 2, 12450), ("checker", lambda: S.checker_scene(block=11), 50, 6950), ("staircase", S.staircase_scene, 27, 8433)]


@pytest.mark.parametrize("name,make,n_comps,n_255", SCENES, ids=[s[0] for s in SCENES])
def test_bgsub_from_depth_equals_xyz_and_the_restatement(name, make, n_comps, n_255):
    bg, im, nn, nb, prev = make()
    cam = CameraIntrin(60.0, 60.5, 64.5, 49.5)
    bgz, imz = np.ascontiguousarray(bg[:, :, 2]), np.ascontiguousarray(im[:, :, 2])
    bg_xyz, im_xyz = depth_to_xyz(bgz, cam), depth_to_xyz(imz, cam)
    ref = R.fast(bg_xyz, im_xyz, nn, nb, prev)
    assert len(ref["comps"]) == n_comps and int((ref["mask"] == 255).sum()) == n_255      # the scene has teeth
    from_xyz = run_one(bgsub.BGSubtractor(bg_xyz), im_xyz, (nn, nb), prev)
    b = bgsub.BGSubtractor(np.zeros_like(bg_xyz))
    b.set_background_depth(bgz, cam)
    b.nnDistThreshRel, b.neighbThreshRel = nn, nb
    b.topLeft, b.botRight = prev
    mask, comps = b.run_depth(imz, cam, comps_by_size=True)
    got = bgsub.Result(mask, b.maskedDepth, bgsub.Frame())
    got.topLeft, got.botRight, got.capped, got.fg_count, got.comps_by_size = b.topLeft, b.botRight, b.capped, b.fgCount, comps
    same_result(got, from_xyz)
    check(got, ref)
    assert same_bits(b.xyz(0), im_xyz)


CAM176 = np.array([(200.0, 201.0, 88.0, 87.5), (190.5, 190.0, 90.25, 80.0), (210.0, 209.5, 85.0, 91.0)], F)


def handover_depths():
    """three 176 x 176 streams: walls at three depths as backgrounds; two blocks, nothing, and one block in front of them"""
    bgz = np.stack([np.full((176, 176), d, F) for d in (3.0, 3.5, 4.0)])
    a = bgz.copy()
    a[0, 20:70, 30:75] = 1.0
    a[0, 90:150, 100:160] = 2.0
    a[2, 40:120, 60:130] = 1.5
    b = bgz.copy()
    b[0, 100:160, 20:80] = 1.25
    b[1, 30:90, 90:150] = 2.25
    return bgz, a, b


@pytest.fixture(scope="module")
def trees():
    return rtree.RTree(GOLD), rtree.RTree(GOLD)


def same_result(a, b):
    assert np.array_equal(a.mask, b.mask) and (a.topLeft, a.botRight) == (b.topLeft, b.botRight)
    assert a.capped == b.capped and a.fg_count == b.fg_count and a.comps_by_size == b.comps_by_size
    assert np.array_equal(a.masked_depth.view(np.uint32), b.masked_depth.view(np.uint32))


def check_labels(got, results, single, interval, usable):
    for i, res in enumerate(results):
        if usable[i]:
            ref = single.predictBest(res.masked_depth, 0, interval, res.topLeft, res.botRight)
            assert np.array_equal(got[i], ref), i
            assert (ref != 255).sum() > 50, i
        else:
            assert (got[i] == 255).all(), i


def test_batch_and_hand_over(trees):
    g, single = trees
    bgz, za, zb = handover_depths()
    bg_xyz = np.stack([depth_to_xyz(bgz[i], CAM176[i]) for i in range(3)])
    order = np.array([2, 0, 1], np.int32)
    prev = np.array([(1, 2, 3, 4), (8, 6, 120, 140), (5, 5, 9, 9)], np.int32)
    b, x = bgsub.BGSubtractor(bg_xyz), bgsub.BGSubtractor(bg_xyz)
    # permuted backgrounds and given boxes: the depth upload against the XYZ upload of the same
    dz, dc = za[order], CAM176[order]
    b.upload_depth(dz, dc, bg_index=order, prev_boxes=prev)
    b.run_resident()
    want_p = x.run_batch(np.stack([depth_to_xyz(dz[i], dc[i]) for i in range(3)]), order, prev)
    for i in range(3):
        same_result(b.download(i), want_p[i])
        assert same_bits(b.xyz(i), depth_to_xyz(dz[i], dc[i]))
    assert want_p[0].fg_count > 1000 and want_p[1].fg_count > 1000 and want_p[2].topLeft == (175, 175)
    # what A and B give on their own
    want_a = x.run_batch(np.stack([depth_to_xyz(za[i], CAM176[i]) for i in range(3)]), None, prev)
    want_b = x.run_batch(np.stack([depth_to_xyz(zb[i], CAM176[i]) for i in range(3)]), None, prev)
    # the hazard of staging in the masked-depth buffer: B's staging is queued behind the forest's read of A's masked depth
    b.upload_depth(za, CAM176, prev_boxes=prev)
    b.run_resident()
    g.predict_from_bgsub(b, 1)
    b.upload_depth(zb, CAM176, prev_boxes=prev)
    b.run_resident()
    labels_a = g.download_all_labels().copy()
    check_labels(labels_a, want_a, single, 1, (True, False, True))
    g.predict_from_bgsub(b, 1)
    labels_b = g.download_all_labels()
    for i in range(3):
        same_result(b.download(i), want_b[i])
    check_labels(labels_b, want_b, single, 1, (True, True, False))
    assert not np.array_equal(labels_a[0], labels_b[0])
    # an XYZ batch after a depth batch on the same handle, and the reverse: nothing of the other is left
    xyz_a = np.stack([depth_to_xyz(za[i], CAM176[i]) for i in range(3)])
    b.upload(xyz_a, prev_boxes=prev)
    b.run_resident()
    for i in range(3):
        same_result(b.download(i), want_a[i])
        assert same_bits(b.xyz(i), xyz_a[i])
    b.upload_depth(zb[:2], CAM176[:2], prev_boxes=prev[:2])
    b.run_resident()
    for i in range(2):
        same_result(b.download(i), want_b[i])
        assert same_bits(b.xyz(i), depth_to_xyz(zb[i], CAM176[i]))
    # one camera for all images
    b.upload_depth(za, CAM176[0])
    assert same_bits(b.xyz(2), depth_to_xyz(za[2], CAM176[0]))


def test_errors_queue_nothing():
    bgz, za, _ = handover_depths()
    b = bgsub.BGSubtractor(np.stack([depth_to_xyz(bgz[i], CAM176[i]) for i in range(2)]))
    before = b.run_batch(np.stack([depth_to_xyz(za[i], CAM176[i]) for i in range(2)]))
    lib, h = b._lib, b._h
    z, k = np.ascontiguousarray(za[:2]), np.ascontiguousarray(CAM176[:2])
    zp, kp = capi.ptr(z, C.c_float), capi.ptr(k, C.c_float)
    mask, out = np.empty((176, 176), np.uint8), np.empty((176, 176, 3), F)
    mp, fr = capi.ptr(mask, C.c_ubyte), bgsub.Frame()
    rel = (C.c_float(0.005), C.c_float(0.005))
    bad = np.array([0, 2], np.int32)
    calls = {
        "upload: null depth": lambda: lib.avt_bgsub_depth_upload(h, 2, None, kp, None, None),
        "upload: null intrinsics": lambda: lib.avt_bgsub_depth_upload(h, 2, zp, None, None, None),
        "upload: n == 0": lambda: lib.avt_bgsub_depth_upload(h, 0, zp, kp, None, None),
        "upload: n < 0": lambda: lib.avt_bgsub_depth_upload(h, -1, zp, kp, None, None),
        "upload: background out of range": lambda: lib.avt_bgsub_depth_upload(h, 2, zp, kp, capi.ptr(bad, C.c_int), None),
        "upload: null handle": lambda: lib.avt_bgsub_depth_upload(None, 2, zp, kp, None, None),
        "run: null depth": lambda: lib.avt_bgsub_run_depth(h, 0, None, kp, *rel, mp, None, C.byref(fr)),
        "run: null intrinsics": lambda: lib.avt_bgsub_run_depth(h, 0, zp, None, *rel, mp, None, C.byref(fr)),
        "run: background out of range": lambda: lib.avt_bgsub_run_depth(h, 2, zp, kp, *rel, mp, None, C.byref(fr)),
        "background: null depth": lambda: lib.avt_bgsub_set_background_depth(h, 0, None, kp),
        "background: null intrinsics": lambda: lib.avt_bgsub_set_background_depth(h, 0, zp, None),
        "background: out of range": lambda: lib.avt_bgsub_set_background_depth(h, 2, zp, kp),
        "xyz: not resident": lambda: lib.avt_bgsub_xyz_download(h, 2, capi.ptr(out, C.c_float)),
        "xyz: negative": lambda: lib.avt_bgsub_xyz_download(h, -1, capi.ptr(out, C.c_float)),
        "xyz: null output": lambda: lib.avt_bgsub_xyz_download(h, 0, None),
    }
    for what, call in calls.items():
        assert call() != 0, what
        assert len(lib.avt_last_error() or b"") > 10, what
        for i in range(2):                                      # the previous result is still there
            same_result(b.download(i), before[i])
    with pytest.raises(ValueError):
        b.upload_depth(za[:, :, :100], CAM176)
    with pytest.raises(ValueError):
        b.upload_depth(za[:2], CAM176)                          # three cameras for two images
    with pytest.raises(capi.AvtError):
        b.xyz(2)


@pytest.fixture(scope="module")
def depth_inputs(smpl):
    """tracker_inputs of the label-batch test as depth images: their z channel, the K4A camera shifted by the crop"""
    bgs, steps = tracker_inputs(smpl)
    rows, cols = bgs.shape[1:3]
    k = synth.K4A_INTRIN
    cam = CameraIntrin(k["fx"], k["fy"], k["cx"] - (k["width"] - cols) // 2, k["cy"] - (k["height"] - rows) // 2)
    return np.ascontiguousarray(bgs[..., 2]), [np.ascontiguousarray(s[..., 2]) for s in steps], cam


def depth_front_end(bgz, cam):
    """a BGSubtractor whose backgrounds arrive as depth images"""
    front = bgsub.BGSubtractor(np.zeros(bgz.shape + (3,), F))
    for i in range(len(bgz)):
        front.set_background_depth(bgz[i], cam, i)
    front.nnDistThreshRel, front.neighbThreshRel = LIVE
    return front


def test_multi_tracker_from_depth_images_equals_the_xyz_path(smpl, gmodel, depth_inputs):
    bgz, steps, cam = depth_inputs
    rows, cols = bgz.shape[1:]
    pm = synth.identity_part_map()

    def make():
        return MultiFrameTracker.create(gmodel, 2, 24, pm, max_points=rows * cols // 16 + 1, beta_pose=0.05, beta_shape=0.12, **_policy())

    A, B = make(), make()
    A.attach_front_end(depth_front_end(bgz, cam), rtree.RTree(GOLD), rtree_interval=2, dist_to_pre_weight=0.001)
    from_xyz = bgsub.BGSubtractor(np.stack([depth_to_xyz(z, cam) for z in bgz]))
    from_xyz.nnDistThreshRel, from_xyz.neighbThreshRel = LIVE
    B.attach_front_end(from_xyz, rtree.RTree(GOLD), rtree_interval=2, dist_to_pre_weight=0.001)
    fitted_any = False
    for t, depths in enumerate(steps):
        fa = A.process_depth_images(depths, cam)
        fb = B.process_depth(np.stack([depth_to_xyz(z, cam) for z in depths]))
        assert fa == fb, t
        fitted_any |= any(fa)
        assert np.array_equal(A.p, B.p) and np.array_equal(A.q, B.q) and np.array_equal(A.w, B.w), t
        assert np.array_equal(A.labels, B.labels) and A.boxes == B.boxes, t
        for s in range(2):
            assert np.array_equal(A.comPre[s], B.comPre[s]), (t, s)
    assert fitted_any and max(st.num_correspondences for st in A.stats if st is not None) > 200
    assert (A.labels[0] != 255).sum() > 1000


def test_frame_tracker_from_a_depth_image_equals_the_xyz_path(smpl, gmodel, depth_inputs):
    bgz, steps, cam = depth_inputs
    rows, cols = bgz.shape[1:]
    front = depth_front_end(bgz[:1], cam)

    def tracker():
        tree = rtree.RTree(GOLD)
        opt = api.AvatarOptimizer(api.Avatar(gmodel), None, (cols, rows), tree.numParts, tree.partMap, max_points=rows * cols // 9 + 1)
        opt.betaPose, opt.betaShape = 0.05, 0.12
        return FrameTracker(opt, interval=3, rtree=tree)

    ta, tb = tracker(), tracker()
    for t in range(2):
        front.run_depth(steps[t][0], cam)
        tl, br = front.topLeft, front.botRight
        bbox = (tl[1], tl[0], br[1], br[0])
        fa = ta.process_depth_image(front.maskedDepth, cam, bbox)
        fb = tb.process_depth(depth_to_xyz(front.maskedDepth, cam), bbox)
        assert fa == fb and fa, t
        for a, c in ((ta.ava.p, tb.ava.p), (ta.ava.w, tb.ava.w), (ta.ava.r, tb.ava.r), (ta.comPre, tb.comPre)):
            assert np.array_equal(a, c), t
    assert ta.opt.last_stats.num_correspondences > 200


def test_cpp_multi_depth_demo_matches_python(smpl, gmodel, depth_inputs, tmp_path):
    """tests/cpp/multi_depth_demo (ark::MultiFrameTracker::processDepthImages over ark::BGSubtractor::runBatchDepth and
    ark::subsampleFrameDepth) on the inputs of the tracker test: labels, boxes, fitted flags and states of the Python path."""
    from tests.test_gpu_facade import write_model_dir
    exe = os.path.join(HERE, "cpp", "multi_depth_demo")
    assert os.path.exists(exe), "tests/cpp/multi_depth_demo not built (make -C avatar_amd/csrc facade)"
    bgz, steps, cam = depth_inputs
    rows, cols = bgz.shape[1:]
    pol = _policy()
    mdir, inp, outp = str(tmp_path / "model"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_model_dir(smpl, mdir)
    with open(inp, "wb") as fh:
        np.array([2, len(steps), rows, cols, pol["interval"], pol["frame_icp_iters"], pol["reinit_icp_iters"], pol["reinit_cnz"], 2], np.int32).tofile(fh)
        np.array(LIVE, F).tofile(fh)
        np.tile(cam.as_array(), 2).tofile(fh)
        bgz.tofile(fh)
        for depths in steps:
            depths.tofile(fh)
    r = subprocess.run([exe, mdir, GOLD, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    A = MultiFrameTracker.create(gmodel, 2, 24, synth.identity_part_map(), max_points=rows * cols // 16 + 1, beta_pose=0.05, beta_shape=0.12, **pol)
    front = depth_front_end(bgz, cam)
    A.attach_front_end(front, rtree.RTree(GOLD), rtree_interval=2)
    J, K, off = 24, 10, 0
    for t, depths in enumerate(steps):
        fitted = A.process_depth_images(depths, cam)
        labels = np.frombuffer(raw, np.uint8, 2 * rows * cols, off).reshape(2, rows, cols); off += 2 * rows * cols
        boxes = np.frombuffer(raw, np.int32, 8, off).reshape(2, 4); off += 32
        fit = np.frombuffer(raw, np.int32, 2, off); off += 8
        p = np.frombuffer(raw, np.float64, 6, off).reshape(2, 3); off += 48
        q = np.frombuffer(raw, np.float64, 8 * J, off).reshape(2, J, 4); off += 64 * J
        w = np.frombuffer(raw, np.float64, 2 * K, off).reshape(2, K); off += 16 * K
        assert np.array_equal(labels, A.labels), t
        assert [tuple(int(v) for v in b) for b in boxes] == [tl + br for tl, br in A.boxes], t
        assert [bool(v) for v in fit] == fitted, t
        assert np.array_equal(p, A.p) and np.array_equal(q, A.q) and np.array_equal(w, A.w), t
    assert (A.labels[0] != 255).sum() > 1000
    # ark::BGSubtractor's setBackgroundDepth, runDepth and xyz on the live handle, against the Python forms of the same
    front.set_background_depth(bgz[1], cam, 0)
    front.topLeft, front.botRight = (0, 0), (0, 0)
    last = steps[-1][0]
    m = front.run_depth(last, cam)
    mask = np.frombuffer(raw, np.uint8, rows * cols, off).reshape(rows, cols); off += rows * cols
    rec = np.frombuffer(raw, np.int32, 5, off); off += 20
    xyz = np.frombuffer(raw, F, rows * cols * 3, off).reshape(rows, cols, 3); off += 12 * rows * cols
    assert off == len(raw)
    assert np.array_equal(mask, m) and tuple(int(v) for v in rec) == front.topLeft + front.botRight + (front.fgCount,)
    assert same_bits(xyz, front.xyz(0)) and same_bits(xyz, depth_to_xyz(last, cam))
    assert (m != 255).sum() > 10000                     # another room behind the avatar: most of the image is foreground
