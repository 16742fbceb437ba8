"""GPU parity of the background subtraction (include/avt_bgsub.h, avatar_amd/csrc/avt_bgsub.hip) against restatement
(b) of tests/bgsub_restatement.py: mask, box, comps_by_size, masked depth and foreground count, every comparison exact.
Scenes: a wall and a floor back-projected with the K4A intrinsics, the avatar's XYZ map pasted over them."""
import os
import subprocess

import numpy as np
import pytest

import bgsub_restatement as R
from avatar_amd import api, bgsub, rtree, synth, synth_forest
from avatar_amd.tracker import FrameTracker

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "forest_small.srtr")
LIVE = (0.002, 0.001)                                     # live-demo.cpp:96-100


def room(wall=4.5, floor=1.0, rows=720, cols=1280):
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


def avatar(smpl, seed, rows=720, cols=1280):
    w, p, Rm = synth.sample_ground_truth(smpl, seed)
    xyz, mask, _ = synth.render_images(smpl, synth.pose_vertices(smpl, w, p, Rm), synth.identity_part_map())
    k = synth.K4A_INTRIN
    r0, c0 = (k["height"] - rows) // 2, (k["width"] - cols) // 2
    return xyz[r0:r0 + rows, c0:c0 + cols], mask[r0:r0 + rows, c0:c0 + cols] != 255


def scene(smpl, seed, bg, holes=0.0, noise=0.0, second=False, specks=0):
    rng = np.random.default_rng(seed)
    im = bg.copy()
    xyz, fg = avatar(smpl, seed, *bg.shape[:2])
    im[fg] = xyz[fg]
    if second:                                          # a box in front of the wall, away from the avatar
        im[60:200, 80:260] = bg[60:200, 80:260] * np.float32(0.6)
    for _ in range(specks):                             # small blobs far from the background: too small to keep
        r, c, s = int(rng.integers(0, bg.shape[0] - 6)), int(rng.integers(0, bg.shape[1] - 6)), int(rng.integers(1, 6))
        im[r:r + s, c:c + s] = bg[r:r + s, c:c + s] * np.float32(0.5)
    if noise:
        im += rng.normal(0, noise, im.shape).astype(np.float32)
    if holes:
        im[rng.random(bg.shape[:2]) < holes, 2] = 0
    return np.ascontiguousarray(im, np.float32)


def grid(rows, cols, bg, period=21):
    """(period-1)^2-pixel squares between zero-depth lines at 3 m: far more than 254 kept components"""
    im = bg.copy()
    im[:, :, 2] = 0
    for r in range(0, rows - period + 1, period):
        for c in range(0, cols - period + 1, period):
            im[r:r + period - 1, c:c + period - 1] = (0.01 * c, 0.01 * r, 3.0)
    return im


def check(res, ref):
    assert np.array_equal(res.mask, ref["mask"])
    assert res.topLeft == ref["top_left"] and res.botRight == ref["bot_right"]
    assert res.capped == ref["capped"] and res.comps_by_size == ref["comps"] and res.fg_count == ref["fg_count"]
    assert np.array_equal(res.masked_depth.view(np.uint32), ref["masked_depth"].view(np.uint32))


def run_one(b, im, rel=(0.005, 0.005), prev=((0, 0), (0, 0))):
    b.nnDistThreshRel, b.neighbThreshRel = rel
    b.topLeft, b.botRight = prev
    mask, comps = b.run(im, comps_by_size=True)
    res = bgsub.Result(mask, b.maskedDepth, bgsub.Frame())
    res.topLeft, res.botRight, res.capped, res.fg_count, res.comps_by_size = b.topLeft, b.botRight, b.capped, b.fgCount, comps
    return res


@pytest.mark.parametrize("shape", [(480, 640), (720, 1280)])
@pytest.mark.parametrize("rel", [(0.005, 0.005), LIVE])
def test_scenes_bit_exact(smpl, shape, rel):
    bg = room(rows=shape[0], cols=shape[1])
    b = bgsub.BGSubtractor(bg)
    cases = [scene(smpl, 41, bg), scene(smpl, 42, bg, holes=0.02, noise=0.002), scene(smpl, 43, bg, second=True, noise=0.001),
             scene(smpl, 44, bg, specks=60, holes=0.01), bg.copy()]
    for i, im in enumerate(cases):
        ref = R.fast(bg, im, *rel)
        check(run_one(b, im, rel), ref)
        if i == 0:
            assert len(ref["comps"]) >= 1 and ref["fg_count"] > 5000
        if i == 4:                                      # the frame is its background: nothing is foreground
            assert (ref["mask"] == 255).all() and ref["top_left"] == (shape[1] - 1, shape[0] - 1)


def test_cap_keeps_the_previous_box(smpl):
    bg = room(rows=480, cols=640)
    b = bgsub.BGSubtractor(bg)
    first = scene(smpl, 45, bg)
    ref1 = R.fast(bg, first)
    check(run_one(b, first), ref1)
    capped = grid(480, 640, bg)
    ref2 = R.fast(bg, capped, prev_box=(ref1["top_left"], ref1["bot_right"]))
    assert ref2["capped"] and (ref2["mask"] == 254).any()
    # the object keeps the box of the previous run across the capped call, as the reference's members do
    mask = b.run(capped)
    assert b.capped and b.topLeft == ref1["top_left"] and b.botRight == ref1["bot_right"]
    assert np.array_equal(mask, ref2["mask"]) and b.fgCount == ref2["fg_count"]
    assert np.array_equal(b.maskedDepth.view(np.uint32), ref2["masked_depth"].view(np.uint32))
    # the C ABI's default previous box is cv::Point()
    check(run_one(b, capped), R.fast(bg, capped))


def test_errors_are_reported_not_faulted():
    bg = room(rows=48, cols=64)
    b = bgsub.BGSubtractor(bg)
    with pytest.raises(ValueError):
        b.run(np.zeros((48, 65, 3), np.float32))
    with pytest.raises(RuntimeError):
        b.run(bg, background_index=1)
    with pytest.raises(RuntimeError):
        b.download(5)
    with pytest.raises(RuntimeError):
        bgsub.BGSubtractor(np.zeros((2, 65536, 3), np.float32))


def test_resident_batch_equals_single_calls(smpl):
    rows, cols = 480, 640
    bgs = np.stack([room(4.5, 1.0, rows, cols), room(3.8, 1.2, rows, cols)])
    b = bgsub.BGSubtractor(bgs)
    rng = np.random.default_rng(7)
    idx = rng.integers(0, 2, 64).astype(np.int32)
    base = [avatar(smpl, 50 + s, rows, cols) for s in range(4)]
    imgs = np.empty((64, rows, cols, 3), np.float32)
    for i in range(64):
        xyz, fg = base[i % 4]
        im = bgs[idx[i]].copy()
        sh = int(rng.integers(-40, 40))
        im[np.roll(fg, sh, 1)] = np.roll(xyz, sh, 1)[np.roll(fg, sh, 1)]
        im += rng.normal(0, 0.001, im.shape).astype(np.float32)
        im[rng.random((rows, cols)) < 0.01, 2] = 0
        imgs[i] = im
    imgs[9] = grid(rows, cols, bgs[idx[9]])                          # one capped image in the batch
    imgs[10] = bgs[idx[10]]                                          # one empty
    prev = rng.integers(0, 300, (64, 4)).astype(np.int32)
    b.nnDistThreshRel, b.neighbThreshRel = LIVE
    batch = b.run_batch(imgs, idx, prev)
    again = b.run_batch(imgs, idx, prev)
    assert batch[9].capped and batch[9].topLeft == tuple(prev[9, :2]) and not batch[10].comps_by_size
    for i in range(64):
        single = run_one(b, imgs[i], LIVE, (tuple(prev[i, :2]), tuple(prev[i, 2:]))) if idx[i] == 0 else None
        ref = R.fast(bgs[idx[i]], imgs[i], *LIVE, prev_box=(tuple(prev[i, :2]), tuple(prev[i, 2:]))) if i % 8 == 0 or i in (9, 10) else None
        for other in (again[i],) + ((single,) if single is not None else ()):
            assert np.array_equal(batch[i].mask, other.mask) and batch[i].topLeft == other.topLeft and batch[i].botRight == other.botRight
            assert batch[i].comps_by_size == other.comps_by_size and batch[i].fg_count == other.fg_count
            assert np.array_equal(batch[i].masked_depth.view(np.uint32), other.masked_depth.view(np.uint32))
        if ref is not None:
            check(batch[i], ref)
    # backgrounds 1 through single calls as well, and a background replaced in place (live-demo.cpp:207)
    for i in np.nonzero(idx == 1)[0][:4]:
        b.topLeft, b.botRight = tuple(prev[i, :2]), tuple(prev[i, 2:])
        assert np.array_equal(b.run(imgs[i], background_index=1), batch[i].mask)
    b.set_background(bgs[1], 0)
    i = int(np.nonzero(idx == 1)[0][0])
    b.topLeft, b.botRight = tuple(prev[i, :2]), tuple(prev[i, 2:])
    assert np.array_equal(b.run(imgs[i]), batch[i].mask)


def test_end_to_end_into_the_tracker(smpl, gmodel):
    """demo.cpp:179-268: bgsub.run -> masked depth -> predictBest(interval 2, the box) -> postProcess -> the tracker.
    The GPU front end must land on the same fitted state as the same pipeline fed by the restatement's mask and box."""
    bg = room()
    tree = rtree.RTree(GOLD)
    b = bgsub.BGSubtractor(bg)
    b.nnDistThreshRel, b.neighbThreshRel = LIVE

    def tracker():
        opt = api.AvatarOptimizer(api.Avatar(gmodel), None, (1280, 720), tree.numParts, tree.partMap, max_points=8192)
        opt.betaPose, opt.betaShape = 0.05, 0.12
        return FrameTracker(opt, interval=3)

    tg, tr = tracker(), tracker()
    com_g = com_r = None
    prev = ((0, 0), (0, 0))
    for s in (61, 62, 63):
        im = scene(smpl, s, bg, holes=0.01, noise=0.001)
        b.run(im)
        ref = R.fast(bg, im, *LIVE, prev_box=prev)
        prev = (ref["top_left"], ref["bot_right"])
        assert b.topLeft == ref["top_left"] and b.botRight == ref["bot_right"] and b.fgCount == ref["fg_count"]
        assert np.array_equal(b.maskedDepth, ref["masked_depth"])
        outs = []
        for depth, tl, br, com in ((b.maskedDepth, b.topLeft, b.botRight, com_g), (ref["masked_depth"], ref["top_left"], ref["bot_right"], com_r)):
            lab = tree.predictBest(np.ascontiguousarray(depth), 0, 2, tl, br)
            com = tree.postProcess(lab, com, 2, 1, tl, br)
            outs.append((lab, com, (tl[1], tl[0], br[1], br[0])))
        (lab_g, com_g, box_g), (lab_r, com_r, box_r) = outs
        assert np.array_equal(lab_g, lab_r) and np.array_equal(com_g, com_r)
        xyz = im.copy()
        xyz[:, :, 2] = b.maskedDepth
        assert tg.process(xyz, lab_g, box_g) == tr.process(xyz, lab_r, box_r)
        for a, c in ((tg.ava.p, tr.ava.p), (tg.ava.w, tr.ava.w), (tg.ava.r, tr.ava.r)):
            assert np.array_equal(a, c)
    assert tg.opt.last_stats.num_correspondences > 500


def test_cpp_facade_like_python(smpl, tmp_path):
    exe = os.path.join(HERE, "cpp", "bgsub_demo")
    assert os.path.exists(exe), "tests/cpp/bgsub_demo not built (make -C avatar_amd/csrc facade)"
    rows, cols = 480, 640
    bg = room(rows=rows, cols=cols)
    frames = [scene(smpl, 71, bg, holes=0.01, second=True), grid(rows, cols, bg), scene(smpl, 72, bg, specks=20)]
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        np.array([rows, cols, len(frames)], np.int32).tofile(fh)
        np.array(LIVE, np.float32).tofile(fh)
        bg.tofile(fh)
        for f in frames:
            f.tofile(fh)
    subprocess.check_call([exe, inp, outp])
    raw = open(outp, "rb").read()
    py = bgsub.BGSubtractor(bg)
    py.nnDistThreshRel, py.neighbThreshRel = LIVE
    prev = ((0, 0), (0, 0))
    o = 0
    for f in frames:
        mask = np.frombuffer(raw, np.uint8, rows * cols, o); o += rows * cols
        rec = np.frombuffer(raw, np.int32, 6, o); o += 24
        comps = [tuple(int(v) for v in c) for c in np.frombuffer(raw, np.int32, 2 * rec[5], o).reshape(-1, 2)]; o += 8 * int(rec[5])
        depth = np.frombuffer(raw, np.float32, rows * cols, o).reshape(rows, cols); o += 4 * rows * cols
        m, c = py.run(f, comps_by_size=True)
        ref = R.fast(bg, f, *LIVE, prev_box=prev)
        prev = (ref["top_left"], ref["bot_right"])
        assert np.array_equal(mask.reshape(rows, cols), m) and np.array_equal(m, ref["mask"])
        assert (int(rec[0]), int(rec[1])) == py.topLeft == ref["top_left"] and (int(rec[2]), int(rec[3])) == py.botRight == ref["bot_right"]
        assert comps == c == ref["comps"] and int(rec[4]) == py.fgCount == ref["fg_count"]
        assert np.array_equal(depth.view(np.uint32), ref["masked_depth"].view(np.uint32))
    assert o == len(raw)
