"""The device subsampling into a context's resident frames (avatar_amd/csrc/avt_subsample.hip) against the plain-loop
restatement of its rule (tests/subsample_restatement.py, which tests/test_subsample_cpu.py ties to tracker.subsample bit for
bit).  Every expected value is an integer or a bit pattern: frames are compared as uint64 / int32, so NaN payloads and signed
zeros count.  The shapes are the smallest that stand on each boundary of the kernels: the chunk of one workgroup, the wave
inside it, one pass of the scan over the chunk counts, the last grid row and column of a box."""
import os

import numpy as np
import pytest

import bgsub_scenes as S
import subsample_restatement as sr
from avatar_amd import api, bgsub, capi, rforest, rtree, subsample, synth, tracker
from avatar_amd.depth import CameraIntrin
from avatar_amd.tracker import MultiFrameTracker

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "forest_small.srtr")
WHOLE = (0, 0, -1, -1)
PARTS = 24
_CTX, _TREE = {}, []


def ctx_for(gmodel, max_points, max_frames):
    key = (max_points, max_frames)
    if key not in _CTX:
        _CTX[key] = api.Context(gmodel, PARTS, synth.identity_part_map(), max_points, max_frames)
    return _CTX[key]


def stump(fresh=False):
    """a tree of PARTS parts: the stage reads only the labels behind the handle"""
    if fresh or not _TREE:
        f = np.array([[3, 0, 0, -2, 0.5], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.float32)
        l = np.array([[1, 2, -1], [-1, -1, 0], [-1, -1, 1]], np.int32)
        d = np.zeros((2, PARTS), np.float32); d[0, 0] = d[1, PARTS - 1] = 1.0
        t = rtree.RTree.from_arrays(f, l, d, PARTS, part_map=np.arange(PARTS), part_map_type=0)
        if fresh:
            return t
        _TREE.append(t)
    return _TREE[0]


def front(xyz):
    """a background subtractor that holds the XYZ maps (n, rows, cols, 3) resident; no run"""
    b = bgsub.BGSubtractor(np.zeros(xyz.shape[1:], np.float32))
    b.upload(xyz, bg_index=np.zeros(len(xyz), np.int32))
    return b


def random_xyz(rng, n, rows, cols):
    return rng.standard_normal((n, rows, cols, 3)).astype(np.float32)


def random_labels(rng, n, rows, cols, fill=0.4):
    return np.where(rng.random((n, rows, cols)) < fill, rng.integers(0, PARTS, (n, rows, cols)), 255).astype(np.uint8)


def check(ctx, xyz, labels, boxes, intervals, forest=None, centroid_of=None, keep=None):
    """uploads, runs the stage, commits, and compares counts, boxes, centroids and every frame with the restatement"""
    forest = forest or stump()
    labels = np.ascontiguousarray(labels, np.uint8)
    n, rows, cols = labels.shape
    boxes = [WHOLE] * n if boxes is None else boxes
    iv = np.broadcast_to(np.asarray(intervals), (n,))
    forest.upload_labels(labels)
    b = front(np.ascontiguousarray(xyz, np.float32))
    counts, cent, used = ctx.frames_subsample(b, forest, intervals, boxes, centroid_of)
    ctx.frames_commit(keep)
    asked = np.zeros(n, bool)
    if centroid_of is not None:
        asked[np.asarray(centroid_of)] = True
    total = 0
    for i in range(n):
        d, l = sr.subsample(xyz[i], labels[i], boxes[i], int(iv[i]), PARTS)
        assert np.array_equal(counts[i], sr.count_row(l, PARTS)), (i, boxes[i], int(iv[i]))
        assert counts[i, 0] == len(l) and np.array_equal(counts[i, 1:], np.bincount(l, minlength=PARTS))
        want_box = (0, 0, cols - 1, rows - 1) if boxes[i][2] == -1 else tuple(boxes[i])
        assert tuple(used[i]) == want_box, i
        if asked[i] and len(l):
            assert np.array_equal(sr.bits(cent[i]), sr.bits(sr.centroid(d))), i
        else:
            assert np.isnan(cent[i]).all(), i                  # not written: as the caller filled it
        gd, gl = ctx.frame_download(i)
        if keep is not None and not keep[i]:
            assert len(gl) == 0 and len(gd) == 0, i
            continue
        assert gd.shape == d.shape and np.array_equal(sr.bits(gd), sr.bits(d)), (i, boxes[i], int(iv[i]))
        assert np.array_equal(gl, l), i
        total += len(l)
    return counts, total


def test_constants_are_exposed():
    C, W = subsample.constants()
    assert C >= 64 and C % 64 == 0 and W >= 64


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1)])
def test_small_images(gmodel, shape):
    rng = np.random.default_rng(3)
    ctx = ctx_for(gmodel, 512, 8)
    rows, cols = shape
    lab = np.stack([np.full(shape, 255, np.uint8), np.full(shape, 7, np.uint8), random_labels(rng, 1, rows, cols, 0.6)[0]])
    for iv in (1, 2, 7):
        check(ctx, random_xyz(rng, 3, rows, cols), lab, None, iv, centroid_of=[0, 1, 2])


def test_chunk_boundary(gmodel):
    """grids of exactly C - 1, C and C + 1 pixels, as one-row images and as a box at interval 3 in a larger one"""
    C, _ = subsample.constants()
    rng = np.random.default_rng(4)
    ctx = ctx_for(gmodel, 512, 8)
    for g in (C - 1, C, C + 1):
        for fill in (1.0, 0.5):
            _, total = check(ctx, random_xyz(rng, 2, 1, g), random_labels(rng, 2, 1, g, fill), None, 1, centroid_of=[1])
            assert total > 0
        cols = 3 * g + 5                                       # the box (2, 1) .. (2 + 3 (g - 1), 1): g grid pixels in one row
        check(ctx, random_xyz(rng, 1, 4, cols), random_labels(rng, 1, 4, cols, 0.7), [(2, 1, 2 + 3 * (g - 1), 3)], 3)


@pytest.mark.parametrize("pattern", ["none", "all", "first", "last"])
def test_wave_boundary(gmodel, pattern):
    """grids of 63, 64 and 65 pixels: the last lane of a wave, the first of the next"""
    rng = np.random.default_rng(5)
    ctx = ctx_for(gmodel, 512, 8)
    for g in (63, 64, 65, 127, 128, 129):
        lab = np.full((1, 1, g), 255, np.uint8)
        if pattern == "all":
            lab[:] = rng.integers(0, PARTS, g).astype(np.uint8)
        elif pattern == "first":
            lab[0, 0, 0] = 3
        elif pattern == "last":
            lab[0, 0, g - 1] = 23
        counts, _ = check(ctx, random_xyz(rng, 1, 1, g), lab, None, 1, centroid_of=[0])
        assert counts[0, 0] == {"none": 0, "all": g, "first": 1, "last": 1}[pattern]


def test_scan_boundary(gmodel):
    """W C + C + 1 grid pixels at interval 1: more chunks than one pass of the scan takes, the last chunk one pixel wide"""
    C, W = subsample.constants()
    G = W * C + C + 1
    rows = next(r for r in range(int(G ** 0.5), 0, -1) if G % r == 0)
    cols = G // rows
    assert rows > 1 and cols < 32768, (rows, cols)
    rng = np.random.default_rng(6)
    ctx = ctx_for(gmodel, G // 2 + C, 2)
    xyz = random_xyz(rng, 2, rows, cols)
    flat = np.full((2, G), 255, np.uint8)
    flat[0, G - 1] = 5                                         # kept pixels only in the last chunk
    every = rng.integers(0, PARTS, G).astype(np.uint8)
    every[(np.arange(G) // C) % 2 == 1] = 255                  # every second chunk empty
    flat[1] = every
    counts, total = check(ctx, xyz, flat.reshape(2, rows, cols), None, 1, centroid_of=[0, 1])
    assert counts[0, 0] == 1 and counts[1, 0] == (every != 255).sum() > W * C // 2


@pytest.mark.parametrize("interval", [1, 2, 3, 12])
@pytest.mark.parametrize("shape", [(37, 53), (100, 130)])
def test_intervals_and_extents(gmodel, shape, interval):
    """box extents k interval - 1, k interval and k interval + 1 in both axes: the last grid row and column fall just inside,
    on and just outside the box"""
    rows, cols = shape
    rng = np.random.default_rng(7 + interval)
    k = 2
    boxes = []
    for ex in (k * interval - 1, k * interval, k * interval + 1):
        for ey in (k * interval - 1, k * interval, k * interval + 1):
            boxes.append((3, 2, 3 + ex - 1, 2 + ey - 1))
    e = k * interval + 1
    boxes += [(cols - e, rows - e, cols - 1, rows - 1), (cols - 1, rows - 1, cols - 1, rows - 1), (5, 7, 5, 7), WHOLE, (0, 0, cols - 1, rows - 1)]
    n = len(boxes)
    ctx = ctx_for(gmodel, 100 * 130, 16)
    _, total = check(ctx, random_xyz(rng, n, rows, cols), random_labels(rng, n, rows, cols, 0.6), boxes, interval, centroid_of=[0, n - 2])
    assert total > 20


def test_batch_of_five(gmodel):
    """five intervals, five boxes, one of them the empty box of a lost stream, one image all 255"""
    rng = np.random.default_rng(8)
    lab = random_labels(rng, 5, 100, 130, 0.5)
    lab[3] = 255
    boxes = [(4, 6, 120, 90), WHOLE, (129, 99, 0, 0), (0, 0, 129, 99), (17, 0, 18, 99)]
    ctx = ctx_for(gmodel, 100 * 130, 16)
    counts, _ = check(ctx, random_xyz(rng, 5, 100, 130), lab, boxes, [2, 1, 3, 12, 5], centroid_of=[0, 2, 3])
    assert counts[2, 0] == 0 and counts[3, 0] == 0 and counts[1, 0] == (lab[1] != 255).sum() and (counts[[0, 1, 4], 0] > 0).all()


def test_special_values_pass_bit_for_bit(gmodel):
    rng = np.random.default_rng(9)
    rows, cols = 9, 40
    u = np.zeros((rows, cols, 3), np.uint32)
    specials = np.array([0x7FC00001, 0xFFC12345, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF,
                         0x00800000, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)          # quiet NaNs with payloads, +-inf, +-0, denormals, extremes
    u[:] = rng.choice(specials, (rows, cols, 3))
    xyz = u.view(np.float32)[None]
    lab = np.full((1, rows, cols), 11, np.uint8)
    ctx = ctx_for(gmodel, 512, 8)
    counts, _ = check(ctx, xyz, lab, None, 1)
    assert counts[0, 0] == rows * cols
    gd, _ = ctx.frame_download(0)
    assert np.isnan(gd).any() and np.isinf(gd).any() and (np.signbit(gd) & (gd == 0)).any() and ((gd != 0) & (np.abs(gd) < 1e-38)).any()


def test_centroids_for_a_subset(gmodel):
    rng = np.random.default_rng(10)
    ctx = ctx_for(gmodel, 100 * 130, 16)
    lab = random_labels(rng, 6, 60, 70, 0.5)
    lab[4] = 255                                               # asked for, but empty: not written either
    xyz = random_xyz(rng, 6, 60, 70) * np.float32(1000.0)
    check(ctx, xyz, lab, None, [1, 2, 1, 3, 1, 1], centroid_of=[1, 2, 4])
    check(ctx, xyz, lab, None, 1, centroid_of=np.array([True, False, False, True, False, True]))


def test_capacity(gmodel):
    """count == max_points is accepted; one more is refused, nothing is pending, and the context goes on working"""
    M = 300
    ctx = ctx_for(gmodel, M, 2)
    rng = np.random.default_rng(11)
    lab = np.full((2, 16, 20), 255, np.uint8)
    lab.reshape(2, -1)[0, :M] = 2
    lab.reshape(2, -1)[1, :17] = 4
    xyz = random_xyz(rng, 2, 16, 20)
    counts, _ = check(ctx, xyz, lab, None, 1)
    assert counts[0, 0] == M
    lab.reshape(2, -1)[0, M] = 3
    t = stump()
    t.upload_labels(lab)
    b = front(xyz)
    with pytest.raises(capi.AvtError, match=r"image 0 keeps 301 points, more than max_points_per_frame"):
        ctx.frames_subsample(b, t, 1, [WHOLE, WHOLE])
    with pytest.raises(capi.AvtError, match="nothing pending"):
        ctx.frames_commit()
    with pytest.raises(capi.AvtError):
        ctx.optimize_resident(api.Options.counted(icp_iters=1))
    _fit_uploaded(ctx, rng)


def _fit_uploaded(ctx, rng):
    """the context's own frames_upload + fit after a refusal"""
    J, K = ctx.model.numJoints(), ctx.model.numShapeKeys()
    data = [rng.standard_normal((120, 3)) * 0.3, rng.standard_normal((90, 3)) * 0.3]
    labels = [rng.integers(0, PARTS, 120).astype(np.int32), rng.integers(0, PARTS, 90).astype(np.int32)]
    ctx.frames_upload(data, labels)
    q = np.zeros((2, J, 4)); q[:, :, 3] = 1.0
    ctx.state_upload(np.zeros((2, 3)), q, np.zeros((2, K)))
    ctx.optimize_resident(api.Options.counted(icp_iters=1, max_iters_per_icp=2))
    p, _, _, st = ctx.state_download()
    assert np.isfinite(p).all() and st[0].num_correspondences > 0
    for f in range(2):
        gd, gl = ctx.frame_download(f)
        assert np.array_equal(gd, data[f]) and np.array_equal(gl, labels[f])


def test_bad_label_names_the_image(gmodel):
    rng = np.random.default_rng(12)
    ctx = ctx_for(gmodel, 100 * 130, 16)
    lab = random_labels(rng, 5, 30, 40, 0.5)
    lab[3, 12, 20] = 200
    xyz = random_xyz(rng, 5, 30, 40)
    t = stump()
    t.upload_labels(lab)
    b = front(xyz)
    with pytest.raises(capi.AvtError, match=r"label out of range.*in image 3 "):
        ctx.frames_subsample(b, t, 2, [WHOLE] * 5)
    with pytest.raises(capi.AvtError, match="nothing pending"):
        ctx.frames_commit()
    ctx.frames_subsample(b, t, 3, [WHOLE] * 5)                 # (12, 20) is not on the grid of interval 3 ... so this one passes
    ctx.frames_commit()
    lab[3, 12, 20] = 255
    check(ctx, xyz, lab, None, 2)                              # the handle and the context are as good as new


def test_pending_commit_and_refusals(gmodel):
    rng = np.random.default_rng(13)
    ctx = ctx_for(gmodel, 100 * 130, 16)
    lab = random_labels(rng, 4, 30, 40, 0.5)
    xyz = random_xyz(rng, 4, 30, 40)
    check(ctx, xyz, lab, None, 1)                              # frames resident ...
    t = stump()
    t.upload_labels(lab)
    b = front(xyz)
    ctx.frames_subsample(b, t, 2, [WHOLE] * 4)                 # ... and pending again: nothing is resident
    with pytest.raises(capi.AvtError):
        ctx.optimize_resident(api.Options.counted(icp_iters=1))
    with pytest.raises(capi.AvtError):
        ctx.optimize_resident_budgets(api.Options.counted(icp_iters=1), np.ones(4, np.int32))
    with pytest.raises(capi.AvtError, match="keep flags"):
        ctx.frames_commit([True, False])
    check(ctx, xyz, lab, None, 2, keep=[True, False, False, True])
    with pytest.raises(capi.AvtError, match="nothing pending"):
        ctx.frames_commit()
    # refused before anything is queued: the resident frames stay
    for bad_call in (lambda: ctx.frames_subsample(b, t, 0, [WHOLE] * 4), lambda: ctx.frames_subsample(b, t, 1, [(0, 0, 40, 29)] * 4),
                     lambda: ctx.frames_subsample(b, t, 1, [(-1, 0, 5, 5)] * 4), lambda: ctx.frames_subsample(front(xyz[:3]), t, 1, [WHOLE] * 4)):
        with pytest.raises(capi.AvtError):
            bad_call()
        gd, gl = ctx.frame_download(0)
        assert len(gl) == sr.subsample(xyz[0], lab[0], WHOLE, 2, PARTS)[1].size
    other = bgsub.BGSubtractor(np.zeros((30, 40, 3), np.float32))
    with pytest.raises(capi.AvtError, match="no XYZ maps resident"):
        ctx.frames_subsample(other, t, 1, [WHOLE] * 4)
    with pytest.raises(capi.AvtError, match="no run behind"):
        ctx.frames_subsample(b, t, 1)                          # device boxes want a run


def test_one_frame_of_1280_x_720(gmodel):
    rng = np.random.default_rng(14)
    rows, cols = 720, 1280
    small = np.where(rng.random((rows // 8, cols // 8)) < 0.33, rng.integers(0, PARTS, (rows // 8, cols // 8)), 255).astype(np.uint8)
    lab = np.repeat(np.repeat(small, 8, 0), 8, 1)[None]
    kept = int((lab != 255).sum())
    assert rows * cols // 4 < kept < rows * cols // 2
    ctx = ctx_for(gmodel, kept, 1)
    counts, _ = check(ctx, random_xyz(rng, 1, rows, cols), lab, None, 1, centroid_of=[0])
    assert counts[0, 0] == kept


def test_rforest_batch(gmodel):
    rng = np.random.default_rng(15)
    f = rforest.RForest([stump(True), stump(True)])
    ctx = ctx_for(gmodel, 100 * 130, 16)
    check(ctx, random_xyz(rng, 3, 50, 70), random_labels(rng, 3, 50, 70), [(2, 3, 60, 44), WHOLE, (69, 49, 0, 0)], [2, 3, 1], forest=f, centroid_of=[0, 1])


def test_chain_from_bgsub(gmodel):
    """background subtraction, the forest, the device post-processing, the subsampling: nothing through the host but the table"""
    scenes = [S.checker_scene(100, 130, 11), S.spiral_scene(100, 130), S.checker_scene(100, 130, 11)]
    bgs = np.stack([s[0] for s in scenes])
    imgs = np.stack([s[1] for s in scenes])
    imgs[2] = 0
    b, g = bgsub.BGSubtractor(bgs), rtree.RTree(GOLD)
    b.nnDistThreshRel, b.neighbThreshRel = 0.005, 0.005
    ctx = ctx_for(gmodel, 100 * 130, 16)
    for frame, iv in enumerate((2, 2, 1)):
        b.upload(imgs)
        b.run_resident()
        g.predict_from_bgsub(b, iv)
        g.post_process_from_bgsub(b, iv, 0.001)
        counts, cent, boxes = ctx.frames_subsample(b, g, iv, None, [0, 1, 2])
        ctx.frames_commit()
        labels = g.download_all_labels()
        for i in range(3):
            res = b.info(i)
            tl, br = res.topLeft, res.botRight
            assert tuple(boxes[i]) == tl + br
            d, l = tracker.subsample(imgs[i], labels[i], (tl[1], tl[0], br[1], br[0]), iv, PARTS)
            gd, gl = ctx.frame_download(i)
            assert gd.shape == d.shape and np.array_equal(sr.bits(gd), sr.bits(d)) and np.array_equal(gl, l), (frame, i)
            assert counts[i, 0] == len(l) and np.array_equal(counts[i, 1:], np.bincount(l, minlength=PARTS))
            if len(l):
                assert np.array_equal(sr.bits(cent[i]), sr.bits(np.ascontiguousarray(tracker.reinit_state(d, 24, 10)[0])))
        assert counts[0, 0] > 20 and counts[1, 0] > 20 and counts[2, 0] == 0 and tuple(boxes[2]) == (129, 99, 0, 0)
    g.upload_images(np.ones((3, 100, 130), np.float32))
    g.upload_labels(np.full((2, 100, 130), 255, np.uint8))
    with pytest.raises(capi.AvtError, match="not those of"):
        ctx.frames_subsample(b, g, 2)


# ---- the tracker: with the flag the same frames, budgets and states as without it
@pytest.fixture(scope="module")
def tracker_inputs(smpl):
    from test_gpu_post_device import _tracker_inputs
    return _tracker_inputs(smpl)


def _make(gmodel, front_end, device_subsample):
    from test_gpu_bgsub import LIVE
    A = MultiFrameTracker.create(gmodel, 3, 24, synth.identity_part_map(), max_points=240 * 320 // 4 + 1, beta_pose=0.05, beta_shape=0.12,
                                 interval=2, frame_icp_iters=2, reinit_icp_iters=3, reinit_cnz=400)
    front_end.nnDistThreshRel, front_end.neighbThreshRel = LIVE
    A.attach_front_end(front_end, rtree.RTree(GOLD), rtree_interval=2, dist_to_pre_weight=0.001, device_post_process=True,
                       device_subsample=device_subsample)
    return A


def _same_step(A, B, fa, fb, t):
    assert fa == fb, t
    assert np.array_equal(A.last_budgets, B.last_budgets) and A.last_reinit == B.last_reinit, t
    assert np.array_equal(A.p, B.p) and np.array_equal(A.q, B.q) and np.array_equal(A.w, B.w), t
    assert A.labels is None and np.array_equal(A.download_labels(), B.labels), t
    assert A.boxes == B.boxes, t
    for s in range(3):
        assert np.array_equal(A.comPre[s], B.comPre[s]), (t, s)


def test_the_flag_needs_the_device_post_processing(gmodel, tracker_inputs):
    bgs, _ = tracker_inputs
    A = MultiFrameTracker.create(gmodel, 3, 24, synth.identity_part_map(), max_points=1000)
    with pytest.raises(ValueError, match="device_post_process"):
        A.attach_front_end(bgsub.BGSubtractor(bgs), rtree.RTree(GOLD), device_subsample=True)


def test_tracker_process_depth(gmodel, tracker_inputs):
    bgs, steps = tracker_inputs
    A, B = _make(gmodel, bgsub.BGSubtractor(bgs), True), _make(gmodel, bgsub.BGSubtractor(bgs), False)
    seen = []
    for t, images in enumerate(steps):
        fa, fb = A.process_depth(images), B.process_depth(images)
        _same_step(A, B, fa, fb, t)
        seen.append(fa)
    assert seen[0] == [True, True, True] and seen[-1] == [True, True, False]
    assert A.last_budgets[2] == 0 and A.last_budgets[:2].min() > 0 and A.streams[2].reinit


def test_tracker_process_depth_images_and_fit_score(gmodel, tracker_inputs):
    bgs, steps = tracker_inputs
    rows, cols = bgs.shape[1:3]
    k = synth.K4A_INTRIN
    cam = CameraIntrin(k["fx"], k["fy"], k["cx"] - (k["width"] - cols) // 2, k["cy"] - (k["height"] - rows) // 2)

    def depth_front():
        f = bgsub.BGSubtractor(np.zeros(bgs.shape, np.float32))
        for i in range(len(bgs)):
            f.set_background_depth(np.ascontiguousarray(bgs[i, :, :, 2]), cam, i)
        return f

    A, B = _make(gmodel, depth_front(), True), _make(gmodel, depth_front(), False)
    with pytest.raises(RuntimeError, match="no step"):
        A.fit_score([0], (cols, rows), cam)
    with pytest.raises(RuntimeError, match="no step"):
        A.download_labels()
    for t, images in enumerate(steps):
        depths = np.ascontiguousarray(images[..., 2])
        fa, fb = A.process_depth_images(depths, cam), B.process_depth_images(depths, cam)
        _same_step(A, B, fa, fb, t)
        if t in (0, 5):
            pm = synth.identity_part_map()
            assert np.array_equal(A.fit_score([2, 0, 1], (cols, rows), cam, 0.05, 1, pm), B.fit_score([2, 0, 1], (cols, rows), cam, 0.05, 1, pm)), t
    assert any(fa) and not fa[2]


def test_cpp_multi_subsample_demo_matches_python(smpl, gmodel, tracker_inputs, tmp_path):
    """tests/cpp/multi_subsample_demo (ark::MultiFrameTracker with deviceSubsample, ark::frameDecision on count rows) on the
    inputs of the tracker test: labels, boxes, fitted flags, budgets and states of the Python path."""
    import subprocess
    from test_gpu_bgsub import LIVE
    from tests.test_gpu_facade import write_model_dir
    exe = os.path.join(HERE, "cpp", "multi_subsample_demo")
    assert os.path.exists(exe), "tests/cpp/multi_subsample_demo not built (make -C avatar_amd/csrc facade)"
    bgs, steps = tracker_inputs
    rows, cols = bgs.shape[1:3]
    k = synth.K4A_INTRIN
    cam = CameraIntrin(k["fx"], k["fy"], k["cx"] - (k["width"] - cols) // 2, k["cy"] - (k["height"] - rows) // 2)
    mdir, inp, outp = str(tmp_path / "model"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_model_dir(smpl, mdir)
    with open(inp, "wb") as fh:
        np.array([3, len(steps), rows, cols, 2, 2, 3, 400, 2], np.int32).tofile(fh)
        np.array(LIVE, np.float32).tofile(fh)
        np.tile(cam.as_array(), 3).tofile(fh)
        np.ascontiguousarray(bgs[..., 2]).tofile(fh)
        for images in steps:
            np.ascontiguousarray(images[..., 2]).tofile(fh)
    r = subprocess.run([exe, mdir, GOLD, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    front_end = bgsub.BGSubtractor(np.zeros(bgs.shape, np.float32))
    for i in range(3):
        front_end.set_background_depth(np.ascontiguousarray(bgs[i, :, :, 2]), cam, i)
    A = MultiFrameTracker.create(gmodel, 3, 24, synth.identity_part_map(), max_points=rows * cols // 4 + 1, beta_pose=0.05, beta_shape=0.12,
                                 interval=2, frame_icp_iters=2, reinit_icp_iters=3, reinit_cnz=400)
    front_end.nnDistThreshRel, front_end.neighbThreshRel = LIVE
    A.attach_front_end(front_end, rtree.RTree(GOLD), rtree_interval=2, dist_to_pre_weight=0.001, device_post_process=True, device_subsample=True)
    J, K, off = 24, 10, 0
    for t, images in enumerate(steps):
        fitted = A.process_depth_images(np.ascontiguousarray(images[..., 2]), cam)
        labels = np.frombuffer(raw, np.uint8, 3 * rows * cols, off).reshape(3, rows, cols); off += 3 * rows * cols
        boxes = np.frombuffer(raw, np.int32, 12, off).reshape(3, 4); off += 48
        fit = np.frombuffer(raw, np.int32, 3, off); off += 12
        budgets = np.frombuffer(raw, np.int32, 3, off); off += 12
        p = np.frombuffer(raw, np.float64, 9, off).reshape(3, 3); off += 72
        q = np.frombuffer(raw, np.float64, 12 * J, off).reshape(3, J, 4); off += 96 * J
        w = np.frombuffer(raw, np.float64, 3 * K, off).reshape(3, K); off += 24 * K
        assert np.array_equal(labels, A.download_labels()), t
        assert [tuple(int(v) for v in b) for b in boxes] == [tl + br for tl, br in A.boxes], t
        assert [bool(v) for v in fit] == fitted and np.array_equal(budgets, A.last_budgets), t
        assert np.array_equal(p, A.p) and np.array_equal(q, A.q) and np.array_equal(w, A.w), t
    assert off == len(raw) and any(fitted)
