"""postProcess for label batches on the device (avatar_amd/csrc/avt_post.hip) against the restatement of its rule
(tests/post_grid_restatement.py, which tests/test_post_grid_cpu.py ties to the reference at interval 1): labels are bytes and the
centres of mass are doubles computed from exact integer sums by the same IEEE operations, so every comparison is np.array_equal.
The shapes are the smallest that reach each internal boundary: the 32 x 32 grid tile, the borders between tiles, the image
index of a batch, the clamp of the up-scaling at the row end."""
import os
import subprocess

import numpy as np
import pytest

import bgsub_scenes as S
import post_grid_restatement as pgr
from avatar_amd import bgsub, capi, rforest, rtree, synth
from avatar_amd.tracker import MultiFrameTracker

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "forest_small.srtr")
WHOLE = (0, 0, -1, -1)
_TREES = {}


def tree(parts=4, ptype=0, fresh=False):
    """a stump with `parts` parts: the stage reads numParts and the part-map type only"""
    if fresh or (parts, ptype) not in _TREES:
        f = np.array([[3, 0, 0, -2, 0.5], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.float32)
        l = np.array([[1, 2, -1], [-1, -1, 0], [-1, -1, 1]], np.int32)
        d = np.zeros((2, parts), np.float32); d[0, 0] = d[1, parts - 1] = 1.0
        t = rtree.RTree.from_arrays(f, l, d, parts, part_map=np.arange(parts), part_map_type=ptype)
        if fresh:
            return t
        _TREES[parts, ptype] = t
    return _TREES[parts, ptype]


def content(rng, rows, cols, parts=4, count=None, big=8):
    img = np.full((rows, cols), 255, np.uint8)
    for _ in range(count if count is not None else 4 + rows * cols // 40):
        r, c = rng.integers(0, rows), rng.integers(0, cols)
        img[r:r + rng.integers(1, big), c:c + rng.integers(1, big + 2)] = rng.integers(0, parts)
    return img


def run(t, images, boxes, interval, weight, com=None):
    """uploads, runs the stage and compares every image and every slot with the restatement; com: per image (2, parts) or None.
    Returns (labels, com_pre (n, 2, parts))."""
    images = np.ascontiguousarray(images, np.uint8)
    n = len(images)
    boxes = [WHOLE] * n if boxes is None else boxes
    com = [None] * n if com is None else com               # a slot is "not sized" unless the caller gives its memory
    t.com_pre_set(0, np.stack([np.zeros((2, t.numParts)) if c is None else c for c in com]), [c is not None for c in com])
    t.upload_labels(images)
    t.post_process_resident(interval, boxes, weight)
    got = t.download_all_labels()
    got_com, valid = t.com_pre_get(0, n)
    assert valid.all()
    for i in range(n):
        ref, ref_com = pgr.post_process(images[i], boxes[i], interval, com[i], weight, t.numParts, t.partMapType)
        assert np.array_equal(got[i], ref), (i, boxes[i], np.argwhere(got[i] != ref)[:5])
        assert np.array_equal(got_com[i], ref_com), (i, boxes[i])
    return got, got_com


@pytest.mark.parametrize("interval", [1, 2, 3])
def test_grid_extents_at_the_tile_boundaries(interval):
    """1, 31, 32, 33 and 65 grid pixels in each axis: one tile, one short of it, exactly it, one more, and three tiles; the image
    ends right on the last grid pixel or interval - 1 pixels behind it"""
    rng = np.random.default_rng(interval)
    t, ext = tree(), (1, 31, 32, 33, 65)
    for k, gh in enumerate(ext):
        for m, gw in enumerate(ext):
            extra = (interval - 1) * ((k + m) % 2)
            img = content(rng, (gh - 1) * interval + 1 + extra, (gw - 1) * interval + 1 + extra)
            got, _ = run(t, [img], None, interval, 0.01)
    assert (got != 255).any()


def serpentine(rows, cols, step=2):
    img = np.full((rows, cols), 255, np.uint8)
    for i, r in enumerate(range(0, rows, 2 * step)):
        img[r, :] = 1
        if r + 2 * step < rows:
            img[r:r + 2 * step, cols - 1 if i % 2 == 0 else 0] = 1
    return img


def test_components_across_tiles():
    """70 x 70 grid pixels, three tiles each way: a one-pixel serpentine that crosses every tile border many times, a U whose arms
    lie in different tiles and join only in the last row, two arms that never join (the larger wins), each with a decoy"""
    t = tree()
    snake = np.full((70, 70), 255, np.uint8)
    snake[:, :66] = serpentine(70, 66, 1)                  # every run crosses the tile borders at columns 32 and 64
    snake[10:40, 68] = 1                                   # a 30-pixel decoy of the same part, touching nothing
    u = np.full((70, 70), 255, np.uint8)
    u[5:70, 3] = 2; u[0:70, 66] = 2; u[69, 3:67] = 2        # arms in the first and the last tile column, joined on the last row
    u[10:40, 34] = 2                                        # a piece of the same part in the middle tile
    arms = np.full((70, 70), 255, np.uint8)
    arms[2:60, 10] = 0; arms[0:70, 50] = 0                  # 58 against 70 pixels, never joined: the later one is the larger
    arms[69, 11:50] = 3
    for iv in (1, 2):
        imgs = [np.repeat(np.repeat(a, iv, 0), iv, 1) for a in (snake, u, arms)]
        got, com = run(t, imgs, None, iv, 0.01)
        g = [x[::iv, ::iv] for x in got]
        assert (g[0] == 1).sum() > 300 and (g[1] == 2).sum() == 65 + 70 + 62 and (g[2][:, 10] == 255).all() and (g[2][:, 50] == 0).all()


def test_checkerboard_every_pixel_is_a_root():
    """65 x 65 of two parts: 4225 one-pixel components, every score ties at 1: the first raster pixel of each part stays"""
    r, c = np.meshgrid(np.arange(65), np.arange(65), indexing="ij")
    img = ((r + c) % 2).astype(np.uint8)
    got, com = run(tree(2), [img], None, 1, 0.0)
    assert (got[0] != 255).sum() == 2 and got[0][0, 0] == 0 and got[0][0, 1] == 1
    assert com[0].tolist() == [[0.0, 1.0], [0.0, 0.0]]
    up = np.repeat(np.repeat(img, 3, 0), 3, 1)[:193, :194]
    got, _ = run(tree(2), [up], [(0, 0, 193, 192)], 3, 0.0)
    assert (got[0][::3, ::3] != 255).sum() == 2


def test_selection_and_the_memory():
    t = tree(2, fresh=True)
    img = np.full((40, 50), 255, np.uint8)
    img[3:6, 4:8] = 0; img[30:33, 40:44] = 0               # two components of 12 pixels
    img[20, 20] = 1
    got, com = run(t, [img], None, 1, 0.01)                # no memory: the earlier one
    assert (got[0][3:6, 4:8] == 0).all() and (got[0][30:33] == 255).all() and com[0][:, 0].tolist() == [5.5, 4.0]
    mem = np.array([[41.0, 20.0], [31.0, 20.0]])
    got, com = run(t, [img], None, 1, 0.01, [mem])         # the memory on the later one
    assert (got[0][30:33, 40:44] == 0).all() and (got[0][3:6] == 255).all() and com[0][:, 0].tolist() == [41.5, 31.0]
    far = np.array([[5000.0, 20.0], [7.25, 20.0]])
    got, com = run(t, [img], None, 1, 0.01, [far])         # every score of part 0 is <= 0: it vanishes, x = -1, y kept
    assert (got[0] != 255).sum() == 1 and com[0][:, 0].tolist() == [-1.0, 7.25] and com[0][:, 1].tolist() == [20.0, 20.0]
    # three frames, the memory carried on the device, in two slots that see the frames in opposite order
    rng = np.random.default_rng(5)
    frames = [content(rng, 40, 50, 2, count=25) for _ in range(3)]
    t.com_pre_set(0, np.zeros((2, 2, 2)), [False, False])
    ref = [None, None]
    for k in range(3):
        pair = [frames[k], frames[2 - k]]
        t.upload_labels(np.stack(pair))
        t.post_process_resident(1, None, 0.05)
        got = t.download_all_labels()
        com, valid = t.com_pre_get(0, 2)
        for s in range(2):
            want, ref[s] = pgr.post_process(pair[s], WHOLE, 1, ref[s], 0.05, 2, 0)
            assert np.array_equal(got[s], want) and np.array_equal(com[s], ref[s]) and valid[s], (k, s)
    # a slot that was never set reads as not sized; the memory survives a labelling call and images_upload
    com, valid = t.com_pre_get(0, 4)
    assert valid.tolist() == [True, True, False, False] and com[3].tolist() == [[-1.0, -1.0], [0.0, 0.0]]
    t.upload_images(np.ones((1, 8, 8), np.float32))
    t.predict_resident_boxes(1, [WHOLE])
    again, _ = t.com_pre_get(0, 2)
    assert np.array_equal(again, com[:2])


@pytest.mark.parametrize("interval", [1, 2, 3])
def test_boxes(interval):
    rng = np.random.default_rng(40 + interval)
    rows, cols = 47, 61
    boxes = [(3, 5, 40, 33),                               # tl = (3, 5)
             (3, 5, 3 + 7 * interval + interval - 1, 5 + 5 * interval + max(0, interval - 2)),   # extents that are no multiple of interval
             (2, 1, cols - 1, 30),                         # br.x = cols - 1 ...
             (1 if (cols - 2) % interval else 2, 1, cols - 1, 30),   # ... with (br.x - tl.x) % interval != 0 when interval > 1: the fill clamp
             (4, 6, 50, 6 + interval - 1),                 # lower than interval: nothing is up-scaled
             (9, 11, 9, 11),                               # one pixel
             WHOLE]
    if interval > 1:
        assert (boxes[3][2] - boxes[3][0]) % interval != 0
    imgs = [content(rng, rows, cols) for _ in boxes]
    imgs[5][11, 9] = 2
    run(tree(), imgs, boxes, interval, 0.01)
    t = tree()
    with pytest.raises(capi.AvtError, match="region of interest"):    # validated before anything is queued
        t.post_process_resident(interval, [WHOLE] * 6 + [(0, 0, cols, rows - 1)], 0.01)
    with pytest.raises(capi.AvtError, match="interval"):
        t.post_process_resident(0, None, 0.01)


def test_batch_of_five_with_an_empty_box():
    rng = np.random.default_rng(9)
    rows, cols = 70, 90
    same = content(rng, rows, cols)
    imgs = [same, content(rng, rows, cols), same.copy(), content(rng, rows, cols), content(rng, rows, cols)]
    boxes = [(0, 0, 80, 66), (5, 3, 89, 69), (0, 0, 80, 66), (cols - 1, rows - 1, 0, 0), (33, 2, 70, 40)]
    mem = [None, None, None, np.array([[3.0, 4.0, -1.0, 6.0], [1.0, 2.0, 3.0, 4.0]]), None]
    for iv in (1, 2):
        got, com = run(tree(), imgs, boxes, iv, 0.01, mem)
        assert np.array_equal(got[0], got[2]) and np.array_equal(com[0], com[2])       # the roots of two images do not meet
        assert np.array_equal(got[3], imgs[3]) and com[3].tolist() == [[-1.0] * 4, [1.0, 2.0, 3.0, 4.0]]


def test_parts_1_and_127_and_no_labels():
    rng = np.random.default_rng(3)
    run(tree(1), [content(rng, 40, 40, 1), np.full((40, 40), 255, np.uint8)], None, 2, 0.01)
    img = content(rng, 66, 70, 127, count=400, big=5)
    img[65, 69] = 126
    run(tree(127), [img], None, 1, 0.01)


def test_disjoint_part_map_drops_small_pieces():
    rng = np.random.default_rng(8)
    t = tree(4, 1)
    img = content(rng, 120, 200, count=160)                # 0.05 % of 24000 pixels: pieces below 12 go
    got, com = run(t, [img], None, 1, 0.01)
    assert 0 < ((got[0] == 255) & (img != 255)).sum() < (img != 255).sum()
    assert com[0].tolist() == [[-1.0] * 4, [0.0] * 4]                                 # only sized
    up = np.repeat(np.repeat(img, 2, 0), 2, 1)[:239, :399]
    got, _ = run(t, [up], None, 2, 0.01, [np.arange(8.0).reshape(2, 4)])               # 0.05 % of 95361 // 4: 11
    assert 0 < ((got[0] == 255) & (up != 255)).sum()


def test_bad_label_fails_the_call_and_spares_the_others():
    rng = np.random.default_rng(12)
    t = tree()
    imgs = np.stack([content(rng, 40, 50), content(rng, 40, 50), content(rng, 40, 50)])
    bad = imgs.copy()
    bad[1, 17, 23] = 4                                     # num_parts
    t.com_pre_set(0, np.zeros((3, 2, 4)), [False] * 3)
    t.upload_labels(bad)
    with pytest.raises(capi.AvtError, match="label out of range.*image 1"):
        t.post_process_resident(1, None, 0.01)
    got = t.download_all_labels()
    assert np.array_equal(got[1], bad[1])                  # that image is not written, and its memory is not sized
    assert t.com_pre_get(0, 3)[1].tolist() == [True, False, True]
    for i in (0, 2):
        assert np.array_equal(got[i], pgr.post_process(imgs[i], WHOLE, 1, None, 0.01, 4, 0)[0])
    run(t, imgs, None, 1, 0.01)                            # the next call is right for all three


def test_one_frame_of_1280_x_720():
    rng = np.random.default_rng(21)
    small = content(rng, 360, 640, 4, count=500, big=60)
    img = np.repeat(np.repeat(small, 2, 0), 2, 1)
    got, com = run(tree(), [img], None, 2, 0.001)
    assert (got[0] != 255).sum() > 20000


def test_rforest_batch():
    a, b = tree(), tree()
    f = rforest.RForest([a, b])
    rng = np.random.default_rng(31)
    imgs = [content(rng, 50, 70), content(rng, 50, 70), content(rng, 50, 70)]
    run(f, imgs, [(2, 3, 60, 44), WHOLE, (69, 49, 0, 0)], 2, 0.01)


def _front(bgs):
    b = bgsub.BGSubtractor(bgs)
    b.nnDistThreshRel, b.neighbThreshRel = 0.005, 0.005
    return b


def test_from_bgsub_against_the_host_chain():
    """background subtraction, the forest, the device stage, nothing of it through the host; against bgsub's download, the
    single-image forest call and the restatement.  The third scene's mask is empty: its box is not inside the image."""
    scenes = [S.checker_scene(100, 130, 11), S.spiral_scene(100, 130), S.checker_scene(100, 130, 11)]
    bgs = np.stack([s[0] for s in scenes])
    imgs = np.stack([s[1] for s in scenes])
    imgs[2] = 0
    b, g, single = _front(bgs), rtree.RTree(GOLD), rtree.RTree(GOLD)
    ref_com = [None] * 3
    for frame, iv in enumerate((2, 2, 1)):
        b.upload(imgs)
        b.run_resident()
        g.predict_from_bgsub(b, iv)
        g.post_process_from_bgsub(b, iv, 0.001)
        got = g.download_all_labels()
        com, valid = g.com_pre_get(0, 3)
        for i in range(3):
            res = b.download(i)
            tl, br = res.topLeft, res.botRight
            if i < 2:
                lab = single.predictBest(res.masked_depth, 0, iv, tl, br)
                assert (lab != 255).sum() > 50
            else:
                assert tl == (129, 99) and br == (0, 0)
                lab = np.full((100, 130), 255, np.uint8)
            want, ref_com[i] = pgr.post_process(lab, tl + br, iv, ref_com[i], 0.001, 24, 0)
            assert np.array_equal(got[i], want), (frame, i)
            assert np.array_equal(com[i], ref_com[i]) and valid[i], (frame, i)
    # without the labels of that run behind the tree the call is refused
    g.upload_images(np.ones((3, 100, 130), np.float32))
    g.upload_labels(np.full((2, 100, 130), 255, np.uint8))
    with pytest.raises(capi.AvtError, match="not those of"):
        g.post_process_from_bgsub(b, 2, 0.001)


def _tracker_inputs(smpl, steps=6):
    """three streams at 240 x 320 in front of one room, four rendered scenes among them; stream 2 sees only the room from step
    3 on (lost)"""
    from test_gpu_bgsub import room, scene
    rows, cols = 240, 320
    bg = room(4.5, 1.0, rows, cols)
    a, b, c, d = scene(smpl, 60, bg, noise=0.001), scene(smpl, 71, bg, holes=0.01), scene(smpl, 82, bg), scene(smpl, 93, bg, noise=0.001)
    return np.stack([bg, bg, bg]), [np.stack([(a, b)[t % 2], (c, d, a)[t % 3], (b, d, c)[t] if t < 3 else bg]) for t in range(steps)]


def _make_tracker(gmodel, bgs, interval, device):
    from test_gpu_bgsub import LIVE
    rows, cols = bgs.shape[1:3]
    A = MultiFrameTracker.create(gmodel, 3, 24, synth.identity_part_map(), max_points=rows * cols // 4 + 1, beta_pose=0.05, beta_shape=0.12,
                                 interval=2, frame_icp_iters=2, reinit_icp_iters=3, reinit_cnz=400)
    front = bgsub.BGSubtractor(bgs)
    front.nnDistThreshRel, front.neighbThreshRel = LIVE
    A.attach_front_end(front, rtree.RTree(GOLD), rtree_interval=interval, dist_to_pre_weight=0.001, device_post_process=device)
    return A


def test_tracker_with_the_device_stage(smpl, gmodel):
    """rtree_interval 1: the rule is the reference's, so the tracker with the flag is the tracker without it, bit for bit.
    rtree_interval 2: labels and comPre are the restatement's of what the forest made."""
    bgs, steps = _tracker_inputs(smpl)
    A, B = _make_tracker(gmodel, bgs, 1, True), _make_tracker(gmodel, bgs, 1, False)
    seen = []
    for t, images in enumerate(steps):
        fa, fb = A.process_depth(images), B.process_depth(images)
        seen.append(fa)
        assert fa == fb, t
        assert np.array_equal(A.p, B.p) and np.array_equal(A.q, B.q) and np.array_equal(A.w, B.w), t
        assert np.array_equal(A.labels, B.labels) and A.boxes == B.boxes, t
        for s in range(3):
            assert np.array_equal(A.comPre[s], B.comPre[s]), (t, s)
    assert seen[0] == [True, True, True] and seen[-1] == [True, True, False]
    assert (A.comPre[2][0] == -1).all() and (A.labels[0] != 255).sum() > 500
    # interval 2: against a forest of its own and the restatement
    C = _make_tracker(gmodel, bgs, 2, True)
    front, g = _front(bgs), rtree.RTree(GOLD)
    front.nnDistThreshRel, front.neighbThreshRel = C.bgsub.nnDistThreshRel, C.bgsub.neighbThreshRel
    com = [None] * 3
    for t, images in enumerate(steps[:4]):
        C.process_depth(images)
        front.upload(images)
        front.run_resident()
        g.predict_from_bgsub(front, 2)
        raw = g.download_all_labels()
        for s in range(3):
            tl, br = C.boxes[s]
            want, com[s] = pgr.post_process(raw[s], tl + br, 2, com[s], 0.001, 24, 0)
            assert np.array_equal(C.labels[s], want), (t, s)
            assert np.array_equal(C.comPre[s], com[s]), (t, s)


def test_cpp_post_device_demo(tmp_path):
    """tests/cpp/post_device_demo: ark::RTree::postProcessResident, comPre and setComPre, and ark::RForest's, on a batch"""
    exe = os.path.join(HERE, "cpp", "post_device_demo")
    assert os.path.exists(exe), "tests/cpp/post_device_demo not built (make -C avatar_amd/csrc facade)"
    rng = np.random.default_rng(77)
    rows, cols, n, iv, w = 50, 70, 3, 2, 0.01
    imgs = np.stack([content(rng, rows, cols, 24) for _ in range(n)])
    boxes = np.array([(2, 3, 60, 44), WHOLE, (69, 49, 0, 0)], np.int32)
    mem = np.zeros((2, 24)); mem[0] = 30.0; mem[1] = 20.0
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        np.array([n, rows, cols, iv], np.int32).tofile(fh)
        np.array([w], np.float64).tofile(fh)
        boxes.tofile(fh)
        np.ascontiguousarray(mem.T).tofile(fh)             # slot 1's memory, num_parts x 2
        imgs.tofile(fh)
    r = subprocess.run([exe, GOLD, inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    off = 0
    for who in ("tree", "forest"):
        lab = np.frombuffer(raw, np.uint8, n * rows * cols, off).reshape(n, rows, cols); off += n * rows * cols
        com = np.frombuffer(raw, np.float64, n * 24 * 2, off).reshape(n, 24, 2).transpose(0, 2, 1); off += n * 24 * 16
        for i in range(n):
            want, want_com = pgr.post_process(imgs[i], tuple(boxes[i]), iv, mem if i == 1 else None, w, 24, 0)
            assert np.array_equal(lab[i], want), (who, i)
            assert np.array_equal(com[i], want_com), (who, i)
    assert off == len(raw)
