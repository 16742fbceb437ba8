"""Labelling a batch of streams on the device (include/avt_rtree.h): one box per image (k_rtree_predict_boxes), the hand-over
from the background subtraction without a host trip (avt_rtree_predict_best_from_bgsub) and MultiFrameTracker.process_depth on
top of both.  Labels are uint8 and the fitted states come from the same kernels on the same inputs: every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import bgsub_scenes as S
from avatar_amd import bgsub, capi, rtree, synth
from avatar_amd.tracker import MultiFrameTracker
from oracle import rtree_oracle as ro
from test_gpu_bgsub import LIVE, room, scene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "forest_small.srtr")
ROWS, COLS = 37, 53


@pytest.fixture(scope="module")
def trees():
    # `single` serves the one-image calls the batch is compared with: they replace a tree's resident images
    return rtree.RTree(GOLD), rtree.RTree(GOLD), ro.OracleRTree.load(GOLD)


def _noise(seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.3, 6.0, (ROWS, COLS)).astype(np.float32)
    d[rng.random((ROWS, COLS)) < 0.2] = 0
    return d


def _boxes(interval):
    return [((0, 0), (-1, -1)), ((3, 1), (52, 36)), ((10, 10), (10, 11)), ((5, 7), (40, 7 + interval - 1)), ((52, 36), (0, 0))]


@pytest.mark.parametrize("interval", [1, 2, 5])
@pytest.mark.parametrize("fill", [True, False])
def test_boxes_against_the_oracle(trees, interval, fill):
    g, single, o = trees
    depths = np.stack([_noise(100 + i) for i in range(5)])
    boxes = _boxes(interval)
    g.upload_images(depths)
    labelled = 0
    for shift in (0, 2):                            # the same call with the boxes permuted across the images
        bx = boxes[shift:] + boxes[:shift]
        g.predict_resident_boxes(interval, [tl + br for tl, br in bx], fill)
        got = g.download_all_labels()
        assert got.shape == depths.shape
        for i, (tl, br) in enumerate(bx):
            ref = o.predictBest(depths[i], interval=interval, top_left=tl, bot_right=br, fill_in_gaps=fill)
            assert np.array_equal(got[i], ref), (shift, i)
            assert np.array_equal(g.download_labels(i), ref), (shift, i)
            if tl[0] <= br[0] or br[0] == -1:       # the single-image call refuses an empty box
                assert np.array_equal(single.predictBest(depths[i], 0, interval, tl, br, fill), ref), (shift, i)
            if bx[i] in (boxes[3], boxes[4]):
                assert (got[i] == 255).all(), (shift, i)
            labelled += int((got[i] != 255).sum())
    assert labelled > 100
    # a refused call queues nothing: the labels of the previous call are still there
    with pytest.raises(capi.AvtError):
        g.predict_resident_boxes(interval, [(0, 0, -1, -1)] * 4 + [(0, 0, COLS, ROWS - 1)], fill)
    with pytest.raises(capi.AvtError):
        g.predict_resident_boxes(0, [(0, 0, -1, -1)] * 5, fill)
    assert np.array_equal(g.download_all_labels(), got)


def _handover_scene():
    """three 176 x 176 images: capped (keeps the supplied box), all background (empty box), two blocks at two depths"""
    bg0, capped = S.cap_scene()[:2]
    wall = np.zeros((176, 176, 3), np.float32)
    wall[:, :, 2] = 3.0
    blocks = np.zeros((176, 176, 3), np.float32)
    blocks[20:70, 30:75] = (0.1, 0.1, 1.0)
    blocks[90:150, 100:160] = (0.3, 0.3, 2.0)
    return np.stack([bg0, wall, np.zeros_like(wall)]), np.stack([capped, wall, blocks])


def _check_handover(b, g, single, usable, interval):
    """every image of the batch against the single-image call on what bgsub downloads for it"""
    got = g.download_all_labels()
    for i in range(len(usable)):
        res = b.download(i)
        if usable[i]:
            ref = single.predictBest(res.masked_depth, 0, interval, res.topLeft, res.botRight)
            assert np.array_equal(got[i], ref), i
            assert (ref != 255).sum() > 50, i
        else:
            assert (got[i] == 255).all(), i
    return got


def test_hand_over_from_bgsub(trees):
    g, single, _ = trees
    bgs, imgs = _handover_scene()
    b = bgsub.BGSubtractor(bgs)
    inside, outside = (8, 6, 120, 140), (8, 6, 176, 140)
    for prev0, usable0 in ((inside, True), (outside, False)):
        prev = np.array([prev0, (1, 2, 3, 4), (1, 2, 3, 4)], np.int32)
        for interval in (2, 1):
            b.upload(imgs, prev_boxes=prev)
            b.run_resident()
            g.predict_from_bgsub(b, interval)
            with pytest.raises(capi.AvtError, match="no images resident"):     # the tree has no resident depth of its own
                g.predict_resident(interval)
            with pytest.raises(capi.AvtError, match="no images resident"):
                g.predict_resident_boxes(interval, [(0, 0, -1, -1)] * 3)
            r0, r1 = b.download(0), b.download(1)
            assert r0.capped and r0.topLeft + r0.botRight == tuple(prev0)
            assert r1.topLeft == (175, 175) and r1.botRight == (0, 0)
            first = _check_handover(b, g, single, (usable0, False, True), interval)
    # the next batch on the same two handles, other images in the slots: nothing of the previous one is left, and neither
    # stage overwrote what the other was still reading
    order = [2, 0, 1]
    b.upload(imgs[order], bg_index=np.array(order, np.int32), prev_boxes=np.array([(1, 2, 3, 4), inside, (1, 2, 3, 4)], np.int32))
    b.run_resident()
    g.predict_from_bgsub(b, 1)
    b.upload(imgs, prev_boxes=np.array([inside, (1, 2, 3, 4), (1, 2, 3, 4)], np.int32))    # queued behind the labelling
    b.run_resident()
    second = g.download_all_labels()
    g.predict_from_bgsub(b, 1)
    third = _check_handover(b, g, single, (True, False, True), 1)
    assert np.array_equal(second[0], third[2]) and np.array_equal(second[1], third[0]) and (second[2] == 255).all()
    assert not np.array_equal(third[0], first[0])          # the capped image: labelled inside `inside`, all 255 with `outside`
    # a handle without a run behind it is refused
    b.upload(imgs)
    with pytest.raises(capi.AvtError, match="no run"):
        g.predict_from_bgsub(b, 2)


def _policy():
    return dict(interval=4, frame_icp_iters=2, reinit_icp_iters=3, reinit_cnz=1000)


def tracker_inputs(smpl):
    """two streams, two steps at 480 x 640: an avatar in front of each stream's own room; stream 1 sees only its room in step 2"""
    rows, cols = 480, 640
    bgs = np.stack([room(4.5, 1.0, rows, cols), room(3.8, 1.2, rows, cols)])
    steps = [np.stack([scene(smpl, 81, bgs[0], noise=0.001), scene(smpl, 82, bgs[1], holes=0.01)]),
             np.stack([scene(smpl, 83, bgs[0], holes=0.01), bgs[1].copy()])]
    return bgs, steps


def _usable(tl, br, rows, cols):
    return 0 <= tl[0] <= br[0] < cols and 0 <= tl[1] <= br[1] < rows


def test_tracker_process_depth_equals_the_per_image_path(smpl, gmodel):
    bgs, steps = tracker_inputs(smpl)
    rows, cols = bgs.shape[1:3]
    tree = rtree.RTree(GOLD)
    pm = synth.identity_part_map()

    def make():
        return MultiFrameTracker.create(gmodel, 2, 24, pm, max_points=rows * cols // 16 + 1, beta_pose=0.05, beta_shape=0.12, **_policy())

    A, B = make(), make()
    front = bgsub.BGSubtractor(bgs)
    front.nnDistThreshRel, front.neighbThreshRel = LIVE
    A.attach_front_end(front, tree, rtree_interval=2, dist_to_pre_weight=0.001)
    per_image = bgsub.BGSubtractor(bgs)
    per_image.nnDistThreshRel, per_image.neighbThreshRel = LIVE
    single = rtree.RTree(GOLD)
    com = [None, None]
    box = [((0, 0), (0, 0))] * 2
    for t, images in enumerate(steps):
        fa = A.process_depth(images)
        frames = []
        for s in range(2):
            per_image.topLeft, per_image.botRight = box[s]
            per_image.run(images[s], background_index=s)
            tl, br = box[s] = (per_image.topLeft, per_image.botRight)
            if _usable(tl, br, rows, cols):
                lab = single.predictBest(per_image.maskedDepth, 0, 2, tl, br)
                com[s] = single.postProcess(lab, com[s], 2, 1, tl, br, 0.001)
                bbox = (tl[1], tl[0], br[1], br[0])
            else:                                   # the reference's loops over an empty box touch nothing: all 255, every comPre x -1
                lab = np.full((rows, cols), 255, np.uint8)
                com[s] = single.postProcess(lab, com[s], 2, 1, (0, 0), (-1, -1), 0.001)
                bbox = (rows - 1, cols - 1, 0, 0)
            frames.append((images[s], lab, bbox))
        fb = B.process(frames)
        assert fa == fb, t
        assert fa == ([True, True] if t == 0 else [True, False]), t
        assert np.array_equal(A.p, B.p) and np.array_equal(A.q, B.q) and np.array_equal(A.w, B.w), t
        for s in range(2):
            assert np.array_equal(A.comPre[s], com[s]), (t, s)
            assert A.boxes[s] == box[s], (t, s)
    assert A.boxes[1] == ((cols - 1, rows - 1), (0, 0)) and (A.comPre[1][0] == -1).all()
    assert max(st.num_correspondences for st in A.stats if st is not None) > 200


def test_cpp_multi_label_demo_matches_python(smpl, gmodel, tmp_path):
    """tests/cpp/multi_label_demo (ark::MultiFrameTracker::processDepth over ark::BGSubtractor::runBatch and
    ark::RTree::predictBestFromBGSub) on the inputs of the tracker test: the labels, boxes, fitted flags and states of the
    Python path, step by step."""
    from tests.test_gpu_facade import write_model_dir
    exe = os.path.join(HERE, "cpp", "multi_label_demo")
    assert os.path.exists(exe), "tests/cpp/multi_label_demo not built (make -C avatar_amd/csrc facade)"
    bgs, steps = tracker_inputs(smpl)
    rows, cols = bgs.shape[1:3]
    pol = _policy()
    mdir, inp, outp = str(tmp_path / "model"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_model_dir(smpl, mdir)
    with open(inp, "wb") as fh:
        np.array([2, len(steps), rows, cols, pol["interval"], pol["frame_icp_iters"], pol["reinit_icp_iters"], pol["reinit_cnz"], 2], np.int32).tofile(fh)
        np.array(LIVE, np.float32).tofile(fh)
        bgs.tofile(fh)
        for images in steps:
            images.tofile(fh)
    r = subprocess.run([exe, mdir, GOLD, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    A = MultiFrameTracker.create(gmodel, 2, 24, synth.identity_part_map(), max_points=rows * cols // 16 + 1, beta_pose=0.05, beta_shape=0.12, **pol)
    front = bgsub.BGSubtractor(bgs)
    front.nnDistThreshRel, front.neighbThreshRel = LIVE
    A.attach_front_end(front, rtree.RTree(GOLD), rtree_interval=2)
    J, K, off = 24, 10, 0
    for t, images in enumerate(steps):
        fitted = A.process_depth(images)
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
    assert off == len(raw) and (A.labels[0] != 255).sum() > 1000
