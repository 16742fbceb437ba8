"""The forest trainer on the GPU (include/avt_rtree_train.h, avatar_amd/rtree_train.py) against its CPU restatement
(tests/cpp/rtree_train_restatement.cpp): chosen samples, whole trees bit for bit (features, thresholds, links, leaf
distributions), determinism across runs and batchings, a usable forest (oracle-loadable, above the toy forest's accuracy),
trainTransfer, and the edge cases."""
import os

import numpy as np
import pytest

from avatar_amd import rtree, rtree_train, synth, synth_forest
from oracle import rtree_oracle as ro

import rtree_train_restatement as rst

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forest_small.srtr")


def _renders(smpl, seeds, step):
    d, m = [], []
    for s in seeds:
        w, p, R = synth.sample_ground_truth(smpl, s)
        xyz, mask, _ = synth.render_images(smpl, synth.pose_vertices(smpl, w, p, R), synth.identity_part_map())
        d.append(synth_forest.depth_of(xyz)[::step, ::step])
        m.append(mask[::step, ::step])
    return np.ascontiguousarray(np.stack(d)), np.ascontiguousarray(np.stack(m))


@pytest.fixture(scope="module")
def small(smpl):
    """12 renders at 320x180; image 3 has no foreground, image 7 fewer labelled pixels than asked, image 5 labelled pixels of
    zero depth"""
    d, m = _renders(smpl, range(300, 312), 4)
    m[3] = 255; d[3] = 0
    keep = np.zeros_like(m[7], bool)
    keep[np.nonzero(m[7] != 255)[0][:150], np.nonzero(m[7] != 255)[1][:150]] = True
    m[7][~keep] = 255
    rr, cc = np.nonzero(m[5] != 255)
    d[5][rr[::7], cc[::7]] = 0
    return d, m


def _device(d, m, P, k, F, M, ms, depth, T, seed, batches=None):
    tr = rtree_train.Trainer(P, k, F, M, ms, depth, T, seed)
    cuts = [0] + list(np.cumsum(batches or [len(d)]))
    for a, b in zip(cuts[:-1], cuts[1:]):
        tr.add_images(d[a:b], m[a:b])
    tree, stats = tr.run()
    return tr, tree, stats


def test_sample_choice_matches_the_restatement(small):
    d, m = small
    tr = rtree_train.Trainer(24, 400, 8, 170.0, 1, 7, 20, seed=77)
    tr.add_images(d, m)
    img, x, y, lab = tr.samples()
    ref = rst.train(d, m, 24, 400, 8, 170.0, 1, 7, 20, seed=77, train=False)
    assert len(img) == len(ref["img"])
    for k, v in (("img", img), ("x", x), ("y", y), ("label", lab)):
        assert np.array_equal(v, ref[k]), k
    assert not (img == 3).any() and (img == 7).sum() == 150 and (img == 0).sum() == 400


@pytest.mark.parametrize("min_samples", [1, 20])
def test_whole_trees_equal_the_restatement(small, min_samples):
    d, m = small
    args = (24, 400, 48, 170.0, min_samples, 7, 20)
    _, tree, stats = _device(d, m, *args, seed=5)
    ref = rst.train(d, m, *args, seed=5, device_tree=(tree.feature, tree.links))
    print(f"min_samples {min_samples}: {stats['n_nodes']} nodes, {stats['n_leafs']} leaves, {stats['n_levels']} levels, "
          f"near ties settled by the device's choice: {ref['ties']}")
    assert ref["ties"] <= 2
    assert np.array_equal(tree.links, ref["links"])
    assert tree.feature.tobytes() == ref["feature"].tobytes()
    assert tree.leafData.tobytes() == ref["leaf"].tobytes()
    assert stats["n_nodes"] == len(ref["links"]) > 15


def test_deterministic_across_runs_and_batchings(small):
    d, m = small
    args = (24, 300, 32, 120.0, 1, 8, 16)
    tr, t1, _ = _device(d, m, *args, seed=9)
    t2, _ = tr.run()
    _, t3, _ = _device(d, m, *args, seed=9, batches=[5, 1, 6])
    for t in (t2, t3):
        assert np.array_equal(t.links, t1.links) and t.feature.tobytes() == t1.feature.tobytes() and t.leafData.tobytes() == t1.leafData.tobytes()
    _, t4, _ = _device(d, m, *args, seed=10)
    assert t4.feature.tobytes() != t1.feature.tobytes()


def test_trained_forest_is_usable_and_beats_the_toy_forest(smpl, tmp_path):
    d, m = _renders(smpl, range(400, 430), 1)
    tree, stats = rtree.RTree.train_from_images(d, m, 24, num_points_per_image=2000, num_features=400, max_probe_offset=170.0,
                                                min_samples=10, max_tree_depth=16, seed=3, part_map=synth.identity_part_map(),
                                                return_stats=True)
    print(f"trained: {stats['n_nodes']} nodes, {stats['n_levels']} levels, {stats['total_ms']:.0f} ms")
    path = str(tmp_path / "trained.srtr")
    assert tree.exportFile(path)
    orc = ro.OracleRTree.load(path)
    # the file stores each leaf's distribution at its node, so a loaded tree numbers leaves in node order, not in the
    # trainer's depth-first visit order: compare links of internal nodes and distributions node by node
    inner = tree.links[:, 2] < 0
    assert np.array_equal(orc.links[:, 2] < 0, inner) and np.array_equal(orc.links[inner], tree.links[inner])
    assert orc.feature[inner].tobytes() == tree.feature[inner].tobytes()
    assert orc.leafData[orc.links[~inner, 2]].tobytes() == tree.leafData[tree.links[~inner, 2]].tobytes()
    gold = rtree.RTree(GOLD)
    hd, hm = _renders(smpl, range(21, 25), 1)
    acc_t, acc_g = [], []
    for i in range(len(hd)):
        a = tree.predictBest(hd[i], interval=1, fill_in_gaps=False)
        assert np.array_equal(a, orc.predictBest(hd[i], interval=1, fill_in_gaps=False))
        fg = hm[i] != 255
        fg[0] = False
        acc_t.append((a[fg] == hm[i][fg]).mean())
        acc_g.append((gold.predictBest(hd[i], interval=1, fill_in_gaps=False)[fg] == hm[i][fg]).mean())
    print(f"held-out pixel accuracy: trained {np.mean(acc_t):.3f}, toy forest {np.mean(acc_g):.3f}")
    assert np.mean(acc_t) > np.mean(acc_g)


def test_train_transfer_matches_the_restatement(small, smpl):
    d, m = small
    _, tree, _ = _device(d, m, 24, 300, 32, 170.0, 1, 9, 20, seed=2)
    old = tree.leafData.copy()
    fd, fm = _renders(smpl, range(500, 503), 4)
    fm[1][:, :40] = 255
    ref, zero = rst.transfer(tree.feature, tree.links, old, fd, fm)
    z = tree.trainTransfer(fd, fm)
    assert z == zero > 0
    assert tree.leafData.tobytes() == ref.tobytes()
    unvisited = np.all(ref == old, axis=1)
    assert unvisited.sum() >= zero
    # the device tree's best-match table follows the new distributions
    assert np.array_equal(tree.leafBestMatch, np.argmax(tree.leafData, axis=1).astype(np.uint8))


def test_edge_cases(small):
    d, m = small
    bad = m[:2].copy()
    bad[0, 100, 100] = 24
    tr = rtree_train.Trainer(24, 50, 8, 170.0, 1, 5, 20, seed=1)
    with pytest.raises(RuntimeError, match="num_parts"):
        tr.add_images(d[:2], bad)
    with pytest.raises(RuntimeError, match="no samples"):
        tr.run()
    tr.add_images(d[3:4], m[3:4])                  # no foreground: still no samples
    with pytest.raises(RuntimeError, match="no samples"):
        tr.run()
    with pytest.raises(RuntimeError):
        rtree_train.Trainer(128, 50, 8, 170.0, 1, 5, 20)
    # a single part, and 127 parts, both against the restatement
    one = np.where(m[:4] != 255, 0, 255).astype(np.uint8)
    for P, mm in ((1, one), (127, np.where(m[:4] != 255, (m[:4].astype(np.int32) * 5) % 127, 255).astype(np.uint8))):
        _, tree, _ = _device(d[:4], mm, P, 200, 16, 170.0, 1, 6, 20, seed=4)
        ref = rst.train(d[:4], mm, P, 200, 16, 170.0, 1, 6, 20, seed=4, device_tree=(tree.feature, tree.links))
        assert np.array_equal(tree.links, ref["links"]) and tree.leafData.tobytes() == ref["leaf"].tobytes(), P
        assert tree.feature.tobytes() == ref["feature"].tobytes(), P


# ---- the device paths: root histograms, rendered images, the C++ facade ------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))


def test_root_histograms_are_the_restatements_integers(small):
    d, m = small
    tr = rtree_train.Trainer(24, 400, 8, 170.0, 1, 7, 20, seed=5)
    tr.add_images(d[:6], m[:6])                        # 2 250 samples: the 256-thread form
    h, mm = tr.root_histograms(40)
    rh, rmm = rst.root_histograms(d[:6], m[:6], 24, 400, 170.0, 20, 5, 40)
    assert np.array_equal(h, rh) and mm.tobytes() == rmm.tobytes()
    assert h.sum() > 0
    tr2 = rtree_train.Trainer(24, 100, 8, 170.0, 1, 7, 20, seed=5)
    tr2.add_images(d[:6], m[:6])                       # 550 samples: the one-wave form
    h2, _ = tr2.root_histograms(40)
    assert np.array_equal(h2, rst.root_histograms(d[:6], m[:6], 24, 100, 170.0, 20, 5, 40)[0])


def _posed_renderer(gmodel, smpl, seeds, W=640, H=360):
    from avatar_amd import render
    intrin = dict(fx=303.219, fy=303.1755, cx=318.647, cy=183.496)
    rend = render.Renderer(gmodel, W, H, intrin, max_images=len(seeds))
    rend.set_part_map(synth.identity_part_map())
    clouds = [synth.pose_vertices(smpl, *synth.sample_ground_truth(smpl, s)) for s in seeds]
    rend.upload(np.stack(clouds))
    rend.run(render.DEPTH | render.PART_MASK)
    imgs = [rend.download(i, render.DEPTH | render.PART_MASK) for i in range(len(seeds))]
    return rend, np.stack([x["depth"] for x in imgs]), np.stack([x["mask"] for x in imgs])


def test_add_rendered_equals_add_images_and_transfer_rendered(gmodel, smpl):
    rend, d, m = _posed_renderer(gmodel, smpl, range(600, 606))
    a = rtree_train.Trainer(24, 500, 24, 170.0, 1, 8, 20, seed=8)
    a.add_rendered(rend)
    b = rtree_train.Trainer(24, 500, 24, 170.0, 1, 8, 20, seed=8)
    b.add_images(d, m)
    for x, y in zip(a.samples(), b.samples()):
        assert np.array_equal(x, y)
    ta, _ = a.run()
    tb, _ = b.run()
    assert np.array_equal(ta.links, tb.links) and ta.feature.tobytes() == tb.feature.tobytes() and ta.leafData.tobytes() == tb.leafData.tobytes()
    # trainTransfer from the renderer in two batches == from the host images in one call == the restatement
    rend2, d2, m2 = _posed_renderer(gmodel, smpl, range(610, 613))
    ref, zero = rst.transfer(ta.feature, ta.links, ta.leafData, np.concatenate([d, d2]), np.concatenate([m, m2]))
    rtree_train.transfer_rendered(ta, rend)
    rtree_train.transfer_rendered(ta, rend2)
    assert rtree_train.transfer_finish(ta) == zero
    assert ta.leafData.tobytes() == ref.tobytes()
    assert tb.trainTransfer(np.concatenate([d, d2]), np.concatenate([m, m2])) == zero and tb.leafData.tobytes() == ref.tobytes()
    # predictBest after the transfer runs on the re-uploaded tree: equal to the oracle on the same arrays
    orc = ro.OracleRTree.from_arrays(ta.feature, ta.links, ta.leafData, 24)
    for i in range(2):
        assert np.array_equal(ta.predictBest(d2[i], interval=1), orc.predictBest(d2[i], interval=1))
    assert ta.device == 0


def _write_images(path, d, m):
    with open(path, "wb") as f:
        f.write(np.array(d.shape, np.int32).tobytes())
        f.write(np.ascontiguousarray(d, np.float32).tobytes())
        f.write(np.ascontiguousarray(m, np.uint8).tobytes())


def _read_images(path):
    buf = open(path, "rb").read()
    n, rows, cols = np.frombuffer(buf[:12], np.int32)
    px = n * rows * cols
    d = np.frombuffer(buf[12:12 + 4 * px], np.float32).reshape(n, rows, cols)
    m = np.frombuffer(buf[12 + 4 * px:12 + 5 * px], np.uint8).reshape(n, rows, cols)
    return d, m


def _same_file_tree(a, b):
    return (np.array_equal(a.links, b.links) and a.feature.tobytes() == b.feature.tobytes() and a.leafData.tobytes() == b.leafData.tobytes())


def test_cpp_demo_trains_the_python_trainers_forest(small, tmp_path):
    import subprocess
    d, m = small
    exe = os.path.join(HERE, "cpp", "rtree_train_demo")
    imgs, out = str(tmp_path / "imgs.bin"), str(tmp_path / "demo.srtr")
    _write_images(imgs, d, m)
    r = subprocess.run([exe, "images", imgs, out, "24", "400", "48", "170", "1", "7", "20", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    py = rtree.RTree.train_from_images(d, m, 24, 400, 48, 170.0, 1, 7, 20, seed=5)
    path = str(tmp_path / "py.srtr")
    assert py.exportFile(path)
    assert open(out, "rb").read() == open(path, "rb").read()


def test_cpp_train_from_avatar_equals_training_on_its_host_rendered_images(smpl, tmp_path):
    import subprocess
    from test_gpu_facade import write_model_dir
    mdir = str(tmp_path / "model")
    write_model_dir(smpl, mdir)
    exe = os.path.join(HERE, "cpp", "rtree_train_demo")
    out, imgs = str(tmp_path / "avatar.srtr"), str(tmp_path / "avatar_imgs.bin")
    # 10 avatars at 640x360 in batches of 4: skinned, rendered and sampled on the device
    r = subprocess.run([exe, "avatar", mdir, out, imgs, "10", "640", "360", "300", "32", "170", "1", "8", "20", "77", "4"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    d, m = _read_images(imgs)
    assert (m != 255).sum() > 1000
    py = rtree.RTree.train_from_images(d, m, 24, 300, 32, 170.0, 1, 8, 20, seed=77, part_map=synth.identity_part_map())
    path = str(tmp_path / "py.srtr")
    assert py.exportFile(path)
    assert open(out, "rb").read() == open(path, "rb").read()


def test_python_train_from_avatar_renders_on_the_device(gmodel, smpl):
    from avatar_amd import api, render
    intrin = dict(fx=303.219, fy=303.1755, cx=318.647, cy=183.496)
    kw = dict(num_images=6, num_points_per_image=300, num_features=24, max_probe_offset=170, min_samples=1, max_tree_depth=7, seed=3)
    tree = rtree.RTree.trainFromAvatar(gmodel, intrin, (640, 360), batch=4, **kw)
    # the same avatars by hand: randomize(idx ^ xor_key), update, render, download, train from the host images
    key = rtree_train.xor_key(3)
    ava = api.Avatar(gmodel)
    rend = render.Renderer(gmodel, 640, 360, intrin, max_images=6)
    rend.set_part_map(synth.identity_part_map())
    clouds = []
    for idx in range(6):
        ava.randomize(True, True, True, (idx ^ key) & 0xFFFFFFFF)
        ava.update()
        clouds.append(ava.cloud.copy())
    rend.upload(np.stack(clouds))
    rend.run(render.DEPTH | render.PART_MASK)
    imgs = [rend.download(i, render.DEPTH | render.PART_MASK) for i in range(6)]
    d, m = np.stack([x["depth"] for x in imgs]), np.stack([x["mask"] for x in imgs])
    ref = rtree.RTree.train_from_images(d, m, 24, 300, 24, 170.0, 1, 7, 20, seed=3)
    assert _same_file_tree(tree, ref) and len(tree.links) > 3
