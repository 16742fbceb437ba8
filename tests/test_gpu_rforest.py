"""GPU tests of the forest of several trees (include/avt_rforest.h, avatar_amd/csrc/avt_rforest.hip): k_rforest_label and
k_rforest_dist through the C ABI, byte for byte against the numpy restatement (tests/rforest_restatement.py, itself anchored to
the single-tree oracle at T = 1 by tests/test_rforest_cpu.py): forests of 1, 2, 3 and 16 random trees over every interval, fill
and box variant, the arg-max and summation-order rules on hand-made leaves, the resident forms, the trackers, the C++ facade
and the training helper."""
import os
import subprocess

import numpy as np
import pytest

import rforest_restatement as rr
from avatar_amd import api, bgsub, capi, rforest, rtree, synth, synth_forest
from avatar_amd.tracker import FrameTracker, MultiFrameTracker

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "forest_small.srtr")
ROWS, COLS = 37, 53


def _random_tree(rng, depth, num_parts):
    """Random full-ish binary tree in parent-before-children order with random probe offsets and thresholds (depth 0: the
    root is a leaf)."""
    feature, links, leaves = [], [], []
    todo = [(0, -1, 0)]
    while todo:
        dep, parent, side = todo.pop(0)
        me = len(feature)
        if parent >= 0:
            links[parent][side] = me
        if dep < depth and (dep < 2 or rng.random() < 0.8):
            u, v = rng.uniform(-60, 60, 2), rng.uniform(-60, 60, 2)
            feature.append([u[0], u[1], v[0], v[1], rng.normal(0, 0.4)]); links.append([-1, -1, -1])
            todo.append((dep + 1, me, 0)); todo.append((dep + 1, me, 1))
        else:
            feature.append([0, 0, 0, 0, 0]); links.append([-1, -1, len(leaves)])
            d = rng.random(num_parts) * (rng.random(num_parts) < 0.4)
            if d.sum() == 0:
                d[rng.integers(num_parts)] = 1.0
            leaves.append(d / d.sum())
    return np.asarray(feature, np.float32), np.asarray(links, np.int32), np.asarray(leaves, np.float32)


def _forest(arrays, num_parts, **kw):
    """The device forest of trees given as arrays; the member trees are host-only (the forest copies them)."""
    return rforest.RForest([rtree.RTree.from_arrays(f, l, d, num_parts, device=-1, **kw) for f, l, d in arrays])


def _leaf(row):
    """A tree whose root is a leaf with the distribution `row`."""
    return np.zeros((1, 5), np.float32), np.array([[-1, -1, 0]], np.int32), np.array([row], np.float32)


def _image(rng, H, W):
    """about 30 % zero depth, the rest at a few distances so that probes land inside and outside the image"""
    depth = rng.choice([0.0, 0.6, 1.5, 2.5, 7.0], (H, W), p=[0.3, 0.1, 0.3, 0.2, 0.1]).astype(np.float32)
    return depth * (1 + 0.05 * rng.standard_normal((H, W))).astype(np.float32)


def _box_variants(H, W, interval):
    """(top_left, bot_right, labels nothing for sure): the whole image, boxes touching each border, a single column, a box
    shorter than the interval"""
    out = [((0, 0), (-1, -1), False), ((0, 0), (W - 1, H - 1), False), ((0, 0), (W // 2, H // 2), False), ((W // 2, H // 2), (W - 1, H - 1), False),
           ((W // 3, 0), (W // 3, H - 1), False), ((W - 1, 0), (W - 1, H - 1), False)]
    y0 = min(H // 4, H - 1)
    out.append(((0, y0), (W - 1, min(y0 + interval - 1, H - 1)), True))          # rows y0 .. y0 + interval - 1: the first row touched is past it
    return out


TREE_DEPTHS = [6, 0, 4, 9, 2, 7, 3, 8, 1, 5, 6, 0, 4, 9, 2, 7]      # tree 1 (and 11) is a single leaf


@pytest.mark.parametrize("num_parts", [2, 37, 127])
@pytest.mark.parametrize("T", [1, 2, 3, 16])
def test_random_forests_byte_for_byte(T, num_parts):
    rng = np.random.default_rng(1000 * T + num_parts)
    arrays = [_random_tree(rng, TREE_DEPTHS[t], num_parts) for t in range(T)]
    assert T == 1 or len(arrays[1][1]) == 1
    g = _forest(arrays, num_parts)
    assert (g.numTrees, g.numParts, g.totalNodes, g.totalLeafs) == (T, num_parts, sum(len(a[1]) for a in arrays), sum(len(a[2]) for a in arrays))
    labelled = 0
    for H, W in ((1, 1), (1, 40), (17, 33), (37, 53)):
        depth = _image(rng, H, W)
        if (H, W) == (1, 1):
            depth[0, 0] = 1.5
        for interval in range(1, 6):
            for k, (tl, br, nothing) in enumerate(_box_variants(H, W, interval)):
                for fill in ((True, False) if k == 0 else (bool((k + interval) & 1),)):
                    got = g.predictBest(depth, 0, interval, tl, br, fill)
                    ref = rr.predict_best(arrays, depth, interval, tl, br, fill)
                    assert got.tobytes() == ref.tobytes(), (H, W, interval, tl, br, fill)
                    assert not nothing or (got == 255).all()
                    labelled += int((got != 255).sum())
        got, ref = g.predict(depth), rr.predict(arrays, depth)
        assert got.shape == (num_parts, H, W) and got.tobytes() == ref.tobytes(), (H, W)
    assert labelled > 2000


def test_argmax_edges():
    depth = np.ones((2, 3), np.float32)
    nan = np.nan

    def label(*rows):
        arrays = [_leaf(r) for r in rows]
        got = _forest(arrays, len(rows[0])).predictBest(depth, 0, 1, fill_in_gaps=False)
        assert got.tobytes() == rr.predict_best(arrays, depth, 1, fill_in_gaps=False).tobytes()
        assert (got[0] == 255).all() and (got[1] == got[1, 0]).all()             # the first row is skipped, every other pixel reaches the one leaf
        return int(got[1, 0])

    assert label([0.25, 0.5, 0.5, 0.1]) == 1                     # a tie goes to the lowest index
    assert label([0.25, 0.25], [0.5, 0.5]) == 0
    assert label([0.5, 0.125, 0.25], [0, 0.375, 0.25]) == 0      # 0.5, 0.5, 0.5
    assert label([0, 0, 0]) == 255                               # all-zero sums
    assert label([0, 0], [0, 0], [0, 0]) == 255
    assert label([nan, 0.25, 0.5]) == 2                          # a NaN never wins ...
    assert label([0.5, nan, 0.25]) == 0
    assert label([0.5, 0.25], [nan, 0.5]) == 1                   # ... nor a sum that became NaN
    assert label([nan, 0], [1, 0]) == 255                        # ... and 255 results if nothing else is positive
    assert label([nan, nan]) == 255
    assert label([-1, -2]) == 255                                # a negative sum never wins
    assert label([-1, 0.5], [0.5, -0.25]) == 1
    assert label([1, 0.5], [-2, -0.25]) == 1
    assert label([-0.0, 0.0]) == 255
    assert label([np.inf, np.inf]) == 0 and label([np.inf, 1], [-np.inf, 0]) == 1          # inf - inf is NaN


def test_summation_order():
    """part 1 gets 2^24, 1, 1 from three trees, part 0 gets 2^24 from one: in tree order part 1 is (2^24 + 1) + 1 = 2^24 in
    float32 and label 0 wins the tie; with the two 1s added first it is 2^24 + 2 and label 1 wins"""
    big = float(2 ** 24)
    depth = np.ones((2, 2), np.float32)
    arrays = [_leaf([big, big]), _leaf([0, 1]), _leaf([0, 1])]
    g = _forest(arrays, 2)
    assert (g.predictBest(depth, fill_in_gaps=False)[1] == 0).all()
    planes = g.predict(depth)
    assert planes.tobytes() == rr.predict(arrays, depth).tobytes()
    assert planes[:, 0, 0].tolist() == [big, big]
    # the same trees in another order: the two 1s first make 2, and 2 + 2^24 is exact; one 1 on each side of 2^24 is lost twice
    for order, part1, winner in (((1, 2, 0), big + 2, 1), ((2, 1, 0), big + 2, 1), ((1, 0, 2), big, 0)):
        other = [arrays[i] for i in order]
        g = _forest(other, 2)
        assert (g.predictBest(depth, fill_in_gaps=False)[1] == winner).all(), order
        planes = g.predict(depth)
        assert planes.tobytes() == rr.predict(other, depth).tobytes() and planes[:, 1, 1].tolist() == [big, part1], order


# ------------------------------------------------------------------------------------------------ the toy tree and its siblings
@pytest.fixture(scope="module")
def renders(smpl):
    def one(seed):
        w, p, R = synth.sample_ground_truth(smpl, seed)
        xyz, mask, _ = synth.render_images(smpl, synth.pose_vertices(smpl, w, p, R), synth.identity_part_map())
        return xyz, mask, synth_forest.depth_of(xyz)
    return {seed: one(seed) for seed in (26, 28)}


@pytest.fixture(scope="module")
def toy():
    """the golden toy tree and two seeded siblings of it (the same toy trainer at a smaller scale), as arrays"""
    t = rtree.RTree(None, device=-1)
    assert t.loadFile(GOLD)
    arrays = [(t.feature, t.links, t.leafData)]
    for seed in (1, 2):
        f, l, d, npp = synth_forest.train(synth.load_model(0), num_images=3, points_per_image=300, num_features=6, threshes_per_feature=4,
                                          min_samples=20, max_depth=7, seed=seed)
        assert npp == 24 and len(l) > 7
        arrays.append((f, l, d))
    return arrays


def _toy_forest(toy, n):
    return _forest(toy[:n], 24, part_map=synth.identity_part_map(), part_map_type=0)


def _bbox(mask):
    r, c = np.nonzero(mask != 255)
    return (int(c.min()), int(r.min())), (int(c.max()), int(r.max()))


def test_one_tree_forest_equals_the_tree(renders):
    g, f = rtree.RTree(GOLD), rforest.RForest([GOLD])
    assert f.numParts == g.numParts and np.array_equal(f.partMap, g.partMap) and f.partMapType == g.partMapType
    _, mask, depth = renders[26]
    tl, br = _bbox(mask)
    rng = np.random.default_rng(5)
    noise = rng.uniform(0.3, 6.0, (ROWS, COLS)).astype(np.float32)
    noise[rng.random((ROWS, COLS)) < 0.2] = 0
    for img, variants in ((depth, (dict(interval=1, fill_in_gaps=False), dict(interval=2), dict(interval=3), dict(interval=2, top_left=tl, bot_right=br),
                                   dict(interval=2, top_left=(tl[0] + 40, tl[1] + 60), bot_right=(br[0] - 30, br[1] - 50)))),
                          (noise, (dict(interval=1), dict(interval=5), dict(interval=4, top_left=(3, 1), bot_right=(52, 36)),
                                   dict(interval=1, top_left=(10, 10), bot_right=(10, 11))))):
        for kw in variants:
            a, b = f.predictBest(img, **kw), g.predictBest(img, **kw)
            assert np.array_equal(a, b), kw
    assert (a != 255).any()


def test_distribution_form(renders, toy):
    tile = np.ascontiguousarray(renders[28][2][200:520:4, 400:900:4])
    assert tile.shape == (80, 125)
    got = _toy_forest(toy, 3).predict(tile)
    assert got.shape == (24, 80, 125) and got.tobytes() == rr.predict(toy, tile).tobytes()
    fg = tile > 0
    assert fg.sum() > 300 and np.allclose(got.sum(0)[fg], 3.0, atol=1e-4) and (got[:, ~fg] == 0).all()


# ------------------------------------------------------------------------------------------------ resident forms
def test_resident_boxes(toy):
    rng = np.random.default_rng(7)
    arrays = toy[:2]
    g, single = _toy_forest(toy, 2), _toy_forest(toy, 2)
    depths = np.stack([_image(rng, ROWS, COLS) for _ in range(3)])
    boxes = [(3, 1, 52, 36), (5, 5, 4, 20), (COLS + 7, ROWS + 3, COLS, ROWS)]      # a usable one, an empty one, an empty one outside the image
    g.upload_images(depths)
    for interval, fill in ((2, True), (1, False), (5, True)):
        for shift in range(3):
            bx = boxes[shift:] + boxes[:shift]
            g.predict_resident_boxes(interval, bx, fill)
            got = g.download_all_labels()
            for i, b in enumerate(bx):
                if b == boxes[0]:
                    ref = single.predictBest(depths[i], 0, interval, b[:2], b[2:], fill)
                    assert ref.tobytes() == rr.predict_best(arrays, depths[i], interval, b[:2], b[2:], fill).tobytes()
                    assert (ref != 255).sum() > 20
                else:
                    ref = np.full((ROWS, COLS), 255, np.uint8)
                assert got[i].tobytes() == ref.tobytes() and g.download_labels(i).tobytes() == ref.tobytes(), (interval, fill, shift, i)
    g.predict_resident_boxes(2, [(0, 0, -1, -1)] * 3)
    got = g.download_all_labels()
    for i in range(3):
        assert got[i].tobytes() == rr.predict_best(arrays, depths[i], 2).tobytes()
    # bad arguments fail before anything is queued: the labels of the previous call are still there
    with pytest.raises(capi.AvtError, match="interval or region"):
        g.predict_resident_boxes(0, [(0, 0, -1, -1)] * 3)
    with pytest.raises(capi.AvtError, match="interval or region"):
        g.predict_resident_boxes(2, [(0, 0, -1, -1)] * 2 + [(0, 0, COLS, ROWS - 1)])
    with pytest.raises(ValueError):
        g.predict_resident_boxes(2, [(0, 0, -1, -1)] * 2)
    with pytest.raises(capi.AvtError, match="interval or region"):
        single.predictBest(depths[0], 0, 0)
    with pytest.raises(capi.AvtError, match="interval or region"):
        single.predictBest(depths[0], 0, 1, (0, 0), (COLS, ROWS - 1))
    assert g.download_all_labels().tobytes() == got.tobytes()


def _bgsub_scene():
    """three 37 x 53 XYZ maps in front of a wall at 3 m: a slanted block with sensor holes, the wall alone (an empty mask), two
    blocks at two depths; thresholds in metres for this image size"""
    rng = np.random.default_rng(9)
    wall = np.zeros((ROWS, COLS, 3), np.float32)
    wall[:, :, 2] = 3.0
    a = wall.copy()
    a[4:30, 8:44, 2] = (1.0 + 0.004 * np.arange(36, dtype=np.float32))[None, :]
    a[4:30, 8:44, 2][rng.random((26, 36)) < 0.1] = 0
    c = wall.copy()
    c[2:20, 3:25, 2] = 1.0
    c[18:35, 30:50, 2] = 2.0 + 0.003 * np.arange(17, dtype=np.float32)[:, None]
    scale = ROWS * COLS / 1.2e6
    return np.stack([wall] * 3), np.stack([a, wall, c]), (0.5 * scale, 0.05 * scale)


def test_from_bgsub(toy):
    arrays = toy[:2]
    g = _toy_forest(toy, 2)
    bgs, imgs, rel = _bgsub_scene()
    b = bgsub.BGSubtractor(bgs)
    b.nnDistThreshRel, b.neighbThreshRel = rel
    # no run behind bg, a bad interval: refused, nothing queued
    b.upload(imgs)
    with pytest.raises(capi.AvtError, match="no run"):
        g.predict_from_bgsub(b, 2)
    b.run_resident()
    with pytest.raises(capi.AvtError, match="interval or region"):
        g.predict_from_bgsub(b, 0)
    import torch
    if torch.cuda.device_count() > 1:                            # handles on different devices
        far = rforest.RForest(g.trees, device=1)
        with pytest.raises(capi.AvtError, match="different devices"):
            far.predict_from_bgsub(b, 2)
    for interval, fill in ((2, True), (1, False), (3, True)):
        g.predict_from_bgsub(b, interval, fill)
        with pytest.raises(capi.AvtError, match="no images resident"):       # the forest has no resident depth of its own
            g.predict_resident_boxes(interval, [(0, 0, -1, -1)] * 3)
        got = g.download_all_labels()
        assert got.shape == (3, ROWS, COLS)
        for i in range(3):
            res = b.download(i)
            ref = rr.predict_best_box_on_device(arrays, res.masked_depth, res.topLeft + res.botRight, interval, fill)
            assert got[i].tobytes() == ref.tobytes(), (interval, fill, i)
            assert g.download_labels(i).tobytes() == ref.tobytes()
            if i == 1:
                assert res.fg_count == 0 and res.topLeft == (COLS - 1, ROWS - 1) and res.botRight == (0, 0) and (got[i] == 255).all()
            else:
                assert (got[i] != 255).sum() > (60 if interval > 1 and not fill else 100), (interval, fill, i)
    # the next batch on the same two handles is queued behind the labelling
    b.upload(imgs[::-1].copy())
    b.run_resident()
    g.predict_from_bgsub(b, 2)
    again = g.download_all_labels()
    assert again[0].tobytes() == rr.predict_best_box_on_device(arrays, b.download(0).masked_depth, b.download(0).topLeft + b.download(0).botRight, 2).tobytes()
    assert (again[1] == 255).all()


# ------------------------------------------------------------------------------------------------ the trackers
def _room(wall, floor, rows, cols):
    """XYZ of a wall at z = wall and a floor at y = floor (camera coordinates, y down) through every pixel"""
    k = synth.K4A_INTRIN
    u, v = np.meshgrid(np.arange(k["width"], dtype=np.float64), np.arange(k["height"], dtype=np.float64))
    rx, ry = (u - k["cx"]) / k["fx"], (v - k["cy"]) / k["fy"]
    t = np.full(u.shape, wall)
    hit = ry > 0
    t[hit] = np.minimum(wall, floor / ry[hit])
    xyz = np.stack([rx * t, ry * t, t], -1).astype(np.float32)
    r0, c0 = (k["height"] - rows) // 2, (k["width"] - cols) // 2
    return np.ascontiguousarray(xyz[r0:r0 + rows, c0:c0 + cols])


def _in_room(render, bg):
    xyz, mask, _ = render
    rows, cols = bg.shape[:2]
    r0, c0 = (xyz.shape[0] - rows) // 2, (xyz.shape[1] - cols) // 2
    im = bg.copy()
    fg = mask[r0:r0 + rows, c0:c0 + cols] != 255
    im[fg] = xyz[r0:r0 + rows, c0:c0 + cols][fg]
    return np.ascontiguousarray(im, np.float32)


def test_frame_tracker_on_a_forest(smpl, gmodel, renders, toy):
    arrays = toy[:2]
    g = _toy_forest(toy, 2)
    xyz, mask, depth = renders[26]
    tl, br = _bbox(mask)
    lab = rr.predict_best(arrays, depth, 2, tl, br)
    assert g.predictBest(depth, 0, 2, tl, br).tobytes() == lab.tobytes() and (lab != 255).sum() > 5000
    com = g.trees[0].postProcess(lab, None, 2, 1, tl, br)
    pm = synth.identity_part_map()
    ava = api.Avatar(gmodel)
    opt = api.AvatarOptimizer(ava, None, (1280, 720), g.numParts, g.partMap, max_points=8192)
    opt.betaPose, opt.betaShape = 0.05, 0.12
    trk = FrameTracker(opt, interval=3, rtree=g)
    assert trk.process_depth(xyz, (tl[1], tl[0], br[1], br[0]))
    assert np.array_equal(trk.comPre, com)
    ava2 = api.Avatar(gmodel)
    opt2 = api.AvatarOptimizer(ava2, None, (1280, 720), 24, pm, max_points=8192)
    opt2.betaPose, opt2.betaShape = 0.05, 0.12
    assert FrameTracker(opt2, interval=3).process(xyz, lab, (tl[1], tl[0], br[1], br[0]))
    assert np.array_equal(ava.p, ava2.p) and np.array_equal(ava.w, ava2.w) and np.array_equal(ava.r, ava2.r)
    assert opt.last_stats.num_correspondences > 1000


def test_multi_frame_tracker_on_a_forest(smpl, gmodel, renders, toy):
    arrays = toy[:2]
    g = _toy_forest(toy, 2)
    rows, cols = 480, 640
    bgs = np.stack([_room(4.5, 1.0, rows, cols), _room(3.8, 1.2, rows, cols)])
    images = np.stack([_in_room(renders[26], bgs[0]), _in_room(renders[28], bgs[1])])
    pm = synth.identity_part_map()

    def make():
        return MultiFrameTracker.create(gmodel, 2, 24, pm, max_points=rows * cols // 16 + 1, beta_pose=0.05, beta_shape=0.12, interval=4,
                                        frame_icp_iters=2, reinit_icp_iters=3, reinit_cnz=1000)

    A, B = make(), make()
    front = bgsub.BGSubtractor(bgs)
    front.nnDistThreshRel, front.neighbThreshRel = 0.002, 0.001          # live-demo.cpp:96-100
    A.attach_front_end(front, g, rtree_interval=2, dist_to_pre_weight=0.001)
    fa = A.process_depth(images)
    frames, coms = [], []
    for s in range(2):
        res = front.download(s)
        tl, br = res.topLeft, res.botRight
        assert 0 <= tl[0] <= br[0] < cols and 0 <= tl[1] <= br[1] < rows
        lab = rr.predict_best(arrays, res.masked_depth, 2, tl, br)
        assert (lab != 255).sum() > 2000
        coms.append(g.trees[0].postProcess(lab, None, 2, 1, tl, br, 0.001))
        frames.append((images[s], lab, (tl[1], tl[0], br[1], br[0])))
        assert A.boxes[s] == (tl, br)
    fb = B.process(frames)
    assert fa == fb == [True, True]
    assert np.array_equal(A.p, B.p) and np.array_equal(A.q, B.q) and np.array_equal(A.w, B.w)
    for s in range(2):
        assert np.array_equal(A.comPre[s], coms[s]), s


# ------------------------------------------------------------------------------------------------ C++ facade, training helper
def test_cpp_facade_labels_like_the_restatement(renders, toy, tmp_path):
    """include/ark/RForest.h through tests/cpp/rforest_demo.cpp on two tree files: predictBest(interval 2, box) + postProcess"""
    exe = os.path.join(HERE, "cpp", "rforest_demo")
    assert os.path.exists(exe), "tests/cpp/rforest_demo not built (make -C avatar_amd/csrc facade)"
    second = str(tmp_path / "second.srtr")
    f, l, d = toy[1]
    assert rtree.RTree.from_arrays(f, l, d, 24, device=-1).exportFile(second)
    synth_forest.write_part_map(second + ".partmap", synth.identity_part_map())
    arrays = []
    for path in (GOLD, second):                                  # as the files number the leaves
        t = rtree.RTree(None, device=-1)
        assert t.loadFile(path)
        arrays.append((t.feature, t.links, t.leafData))
    _, mask, depth = renders[28]
    tl, br = _bbox(mask)
    inp, outp = str(tmp_path / "depth.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        np.array([depth.shape[0], depth.shape[1], tl[0], tl[1], br[0], br[1]], np.int32).tofile(fh)
        depth.tofile(fh)
    subprocess.check_call([exe, inp, outp, GOLD, second])
    raw = np.fromfile(outp, np.uint8)
    got = raw[:depth.size].reshape(depth.shape)
    com = np.frombuffer(raw[depth.size:].tobytes(), np.float64).reshape(-1, 2).T
    ref = rr.predict_best(arrays, depth, 2, tl, br)
    assert (ref != 255).sum() > 5000
    com_ref = t.postProcess(ref, None, interval=2, top_left=tl, bot_right=br)
    assert got.tobytes() == ref.tobytes() and np.array_equal(com, com_ref)


def test_training_helper_seeds(renders):
    d = np.ascontiguousarray(np.stack([renders[s][2][::8, ::8] for s in (26, 28, 26, 28)]))
    m = np.ascontiguousarray(np.stack([renders[s][1][::8, ::8] for s in (26, 28, 26, 28)]))
    d[2:] = d[2:, :, ::-1]; m[2:] = m[2:, :, ::-1]               # four images from two renders
    args = (24, 300, 24, 170.0, 1, 7, 20)

    def same(a, b):
        return np.array_equal(a.links, b.links) and a.feature.tobytes() == b.feature.tobytes() and a.leafData.tobytes() == b.leafData.tobytes()

    for seed in (3, 2 ** 64 - 1):                                # the second wraps: tree 1 is seed 0's
        f = rforest.RForest.train_from_images(2, d, m, *args, seed=seed)
        assert f.numTrees == 2 and f.numParts == 24 and f.totalNodes == len(f.trees[0].links) + len(f.trees[1].links)
        for t in range(2):
            assert same(f.trees[t], rtree.RTree.train_from_images(d, m, *args, seed=(seed + t) % 2 ** 64)), (seed, t)
        assert not same(f.trees[0], f.trees[1]) and len(f.trees[0].links) > 7
        arrays = [(t.feature, t.links, t.leafData) for t in f.trees]
        assert f.predictBest(d[0], 0, 1).tobytes() == rr.predict_best(arrays, d[0], 1).tobytes()
