"""GPU tests of the forest's score (include/avt_rforest.h, THE SCORE; k_rforest_score in avatar_amd/csrc/avt_rforest.hip): the
(P + 1) x (P + 1) confusion matrix of a forest against ground-truth part masks through the C ABI, equal count for count to the
numpy restatement (tests/rforest_score_restatement.py, itself on tests/rforest_restatement.py).  The counts are integers: every
comparison is np.array_equal on int64, none is within a tolerance.  The kernel takes one path for every P (two 16-bit cells per
LDS word), so the table of P has no switch to straddle; 63 / 64 and 127 stand at the word and size edges of that packing."""
import os
import subprocess

import numpy as np
import pytest

import rforest_restatement as rr
import rforest_score_restatement as rs
from avatar_amd import api, capi, render, rforest, rtree, rtree_train, synth
from test_gpu_rforest import GOLD, TREE_DEPTHS, _forest, _leaf, _random_tree

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = ((1, 1, 1), (1, 40, 3), (17, 33, 3), (37, 53, 5))          # rows, cols, images
STRIDES = (1, 2, 3, 5, 1000)                                         # the last is larger than any image: pixel (0, 0) alone
SMALL_INTRIN = dict(fx=75.805, fy=75.794, cx=79.662, cy=45.874)      # synth.K4A_INTRIN scaled from 1280 x 720 to 160 x 90
SMALL = (160, 90)


def _trees(rng, T, P):
    """T random trees as test_gpu_rforest builds them (tree 1 a single leaf), about a tenth of the leaves all zero"""
    arrays = [_random_tree(rng, TREE_DEPTHS[t], P) for t in range(T)]
    for _, _, leaves in arrays:
        leaves[rng.random(len(leaves)) < 0.1] = 0
    if all(leaves.any(1).all() for _, _, leaves in arrays):
        arrays[0][2][-1] = 0
    return arrays


def _images(rng, n, H, W, P):
    """depth with 25 % zeros, 5 % negatives and one NaN, at distances that send probes inside and outside the image; masks drawn
    independently of the depth, 60 % labelled"""
    depth = rng.choice([0.0, 0.6, 1.5, 2.5, 7.0], (n, H, W), p=[0.25, 0.1, 0.3, 0.25, 0.1]).astype(np.float32)
    depth *= (1 + 0.05 * rng.standard_normal((n, H, W))).astype(np.float32)
    neg = rng.random((n, H, W)) < 0.05
    depth[neg] = -np.abs(depth[neg]) - np.float32(0.25)
    mask = np.where(rng.random((n, H, W)) < 0.6, rng.integers(0, P, (n, H, W)), 255).astype(np.uint8)
    if H * W == 1:
        depth[:], mask[:] = 1.5, 0
    else:
        depth.reshape(-1)[int(rng.integers(depth.size))] = np.nan
    return depth, mask


def _score(g, depth, mask, stride=1):
    g.score_reset()
    g.score_images(depth, mask, stride)
    return g.score_get()


def _selected(n, H, W, stride):
    return n * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)


# ------------------------------------------------------------------------------------------------ 1. random forests, exact
@pytest.mark.parametrize("P", [1, 2, 37, 63, 64, 127])
@pytest.mark.parametrize("T", [1, 2, 3, 16])
def test_random_forests_exact(T, P):
    rng = np.random.default_rng(7000 * T + P)
    arrays = _trees(rng, T, P)
    assert T == 1 or len(arrays[1][1]) == 1
    assert any((~leaves.any(1)).any() for _, _, leaves in arrays)
    g = _forest(arrays, P)
    for H, W, n in BATCHES:
        depth, mask = _images(rng, n, H, W, P)
        pred = rs.predicted_batch(arrays, depth)
        if H * W > 1:
            with np.errstate(invalid="ignore"):
                walked, labelled = depth > 0, mask != 255
            assert np.isnan(depth).sum() == 1 and (depth < 0).any() and (depth == 0).any()
            for a in (walked, ~walked):
                for b in (labelled, ~labelled):
                    assert (a & b).any(), (H, W)
        for stride in STRIDES:
            ref, npx = rs.confusion(arrays, depth, mask, stride, pred)
            got = _score(g, depth, mask, stride)
            assert got.conf.dtype == np.int64 and np.array_equal(got.conf, ref), (H, W, stride)
            assert got.n_images == n and got.n_pixels == npx == _selected(n, H, W, stride), (H, W, stride)
            assert got.conf[P, P] == 0
            if (H, W, stride) == (37, 53, 1):                    # every kind of cell: diagonal, off-diagonal, row P, column P
                inner = ref[:P, :P]
                assert np.trace(inner) > 0 and ref[P, :P].sum() > 0 and ref[:P, P].sum() > 0
                assert P == 1 or inner.sum() > np.trace(inner)
            if stride == 1000:
                assert ref.sum() <= n


# ------------------------------------------------------------------------------------------------ 2. batch boundaries
@pytest.mark.parametrize("T,P", [(1, 2), (3, 37), (16, 127)])
def test_a_batch_is_the_sum_of_its_images(T, P):
    """a probe that read a neighbouring image of the batch would break this: the offsets of up to 60 pixels at depths down to
    0.6 m leave the image constantly"""
    rng = np.random.default_rng(90 * T + P)
    arrays = _trees(rng, T, P)
    g = _forest(arrays, P)
    for H, W, n in BATCHES[2:]:
        depth, mask = _images(rng, n, H, W, P)
        for stride in (1, 2):
            whole = _score(g, depth, mask, stride)
            parts = [_score(g, depth[i], mask[i], stride) for i in range(n)]
            assert np.array_equal(whole.conf, sum(p.conf for p in parts)) and whole.n_pixels == sum(p.n_pixels for p in parts)
            assert np.array_equal(whole.conf, rs.confusion(arrays, depth, mask, stride)[0])
            # ... and an image alone scores as it does with the others swapped around it
            swapped = _score(g, depth[::-1].copy(), mask[::-1].copy(), stride)
            assert np.array_equal(whole.conf, swapped.conf)


# ------------------------------------------------------------------------------------------------ 3. arg-max and "none"
def test_argmax_and_none_by_hand():
    nan = np.nan
    depth = np.array([[1, 1, 0], [-1, nan, 1]], np.float32)
    mask = np.array([[0, 255, 1], [0, 1, 255]], np.uint8)

    def check(q, *rows):
        """the forest of root leaves `rows` predicts q (255: none) wherever it walks"""
        arrays = [_leaf(r) for r in rows]
        P = len(rows[0])
        want = np.zeros((P + 1, P + 1), np.int64)
        want[1, P] += 2                                          # depth 0 and NaN under label 1: labelled, not walked
        want[0, P] += 1                                          # a negative depth under label 0
        if q != 255:
            want[0, q] += 1                                      # the walked pixel under label 0
            want[P, q] += 2                                      # the two walked pixels the truth calls background
        else:
            want[0, P] += 1                                      # walked, nothing predicted, labelled; both-none counts nothing
        got = _score(_forest(arrays, P), depth, mask)
        assert np.array_equal(got.conf, want) and np.array_equal(got.conf, rs.confusion(arrays, depth, mask)[0]), rows
        assert got.conf[P, P] == 0 and got.n_pixels == 6 and got.n_images == 1

    check(1, [0.25, 0.5, 0.5, 0.1])                              # a tie goes to the lowest part
    check(0, [0.25, 0.25], [0.5, 0.5])
    check(0, [0.5, 0.125, 0.25], [0, 0.375, 0.25])
    check(255, [0, 0, 0])                                        # all-zero sums: column P
    check(255, [0, 0], [0, 0], [0, 0])
    check(2, [nan, 0.25, 0.5])                                   # a NaN never wins
    check(1, [0.5, 0.25], [nan, 0.5])
    check(255, [nan, 0], [1, 0])                                 # NaN sums: column P
    check(255, [nan, nan])
    check(255, [-1, -2])
    check(1, [-1, 0.5], [0.5, -0.25])
    big = float(2 ** 24)
    check(0, [big, big], [0, 1], [0, 1])                         # (2^24 + 1) + 1 == 2^24 in tree order: the tie stays with part 0
    check(1, [0, 1], [0, 1], [big, big])


# ------------------------------------------------------------------------------------------------ 4. accumulation
def test_totals_accumulate_until_reset():
    rng = np.random.default_rng(41)
    P = 6
    arrays = _trees(rng, 3, P)
    g = _forest(arrays, P)
    zero = g.score_get()
    assert not zero.conf.any() and zero.conf.shape == (P + 1, P + 1) and (zero.n_images, zero.n_pixels) == (0, 0)
    d, m = _images(rng, 5, 17, 33, P)
    d2, m2 = _images(rng, 2, 9, 70, P)                           # another size in the same totals
    a, b = _score(g, d, m, 2), _score(g, d2, m2, 3)
    g.score_reset()
    g.score_images(d, m, 2)
    g.score_images(d2, m2, 3)
    both = g.score_get()
    assert np.array_equal(both.conf, a.conf + b.conf) and both.n_images == 7 and both.n_pixels == a.n_pixels + b.n_pixels
    again = g.score_get()
    assert again.conf.tobytes() == both.conf.tobytes() and (again.n_images, again.n_pixels) == (both.n_images, both.n_pixels)
    g.score_reset()
    cleared = g.score_get()
    assert not cleared.conf.any() and (cleared.n_images, cleared.n_pixels) == (0, 0)
    g.score_images(d[:2], m[:2])
    g.score_images(d[2:], m[2:])
    split = g.score_get()
    one = _score(g, d, m)
    assert np.array_equal(split.conf, one.conf) and split.n_images == one.n_images == 5 and split.n_pixels == one.n_pixels
    assert np.array_equal(one.conf, rs.confusion(arrays, d, m)[0])
    for bad in (0, -1):
        with pytest.raises(capi.AvtError, match="stride"):
            g.score_images(d, m, bad)
    assert np.array_equal(g.score_get().conf, one.conf)


# ------------------------------------------------------------------------------------------------ 5. refusal
def test_a_label_out_of_range_refuses_the_whole_call():
    rng = np.random.default_rng(43)
    P = 5
    arrays = _trees(rng, 2, P)
    g = _forest(arrays, P)
    d, m = _images(rng, 3, 17, 33, P)
    g.score_reset()
    g.score_images(d, m)
    before = g.score_get()
    assert before.conf.sum() > 500
    bad = m.copy()
    bad[2, 16, 32] = P                                           # one byte, in the last image of the batch
    with pytest.raises(capi.AvtError, match="num_parts"):
        g.score_images(d, bad)
    with pytest.raises(ValueError, match="num_parts"):
        rs.confusion(arrays, d, bad)
    after = g.score_get()
    assert after.conf.tobytes() == before.conf.tobytes() and (after.n_images, after.n_pixels) == (before.n_images, before.n_pixels)
    g.score_images(d, m)                                         # the forest goes on working
    assert np.array_equal(g.score_get().conf, 2 * before.conf)
    # P = 127: 254 is refused, 255 is "none"
    arrays = _trees(rng, 1, 127)
    g = _forest(arrays, 127)
    d, m = _images(rng, 1, 17, 33, 127)
    m[0, 3, 3] = 255
    ok = _score(g, d, m)
    assert np.array_equal(ok.conf, rs.confusion(arrays, d, m)[0])
    m[0, 3, 3] = 254
    with pytest.raises(capi.AvtError, match="num_parts"):
        g.score_images(d, m)
    assert g.score_get().conf.tobytes() == ok.conf.tobytes()


# ------------------------------------------------------------------------------------------------ 6. wide counts
def test_counts_beyond_2_to_the_24():
    """4100 x 4100 = 16 810 000 pixels in one cell: a float32 or a narrow accumulator loses some of them"""
    n = 4100
    g = _forest([_leaf([1.0])], 1)
    depth = np.full((1, n, n), 1.5, np.float32)
    got = _score(g, depth, np.zeros((1, n, n), np.uint8))
    assert n * n == 16810000 > 2 ** 24 and got.conf.tolist() == [[n * n, 0], [0, 0]] and got.n_pixels == n * n
    got = _score(g, depth, np.full((1, n, n), 255, np.uint8))
    assert got.conf.tolist() == [[0, 0], [n * n, 0]]
    got = _score(g, depth, np.zeros((1, n, n), np.uint8), 3)     # 1367 x 1367 selected
    assert got.conf.tolist() == [[1367 * 1367, 0], [0, 0]] and got.n_pixels == 1367 * 1367


# ------------------------------------------------------------------------------------------------ 7. resident state untouched
def test_scoring_leaves_the_resident_images_and_labels_alone():
    rng = np.random.default_rng(47)
    P = 9
    arrays = _trees(rng, 2, P)
    g = _forest(arrays, P)
    d, _ = _images(rng, 3, 37, 53, P)
    d = np.nan_to_num(np.abs(d))
    g.upload_images(d)
    g.predict_resident_boxes(2, [(0, 0, -1, -1)] * 3)
    labels = g.download_all_labels()
    assert (labels != 255).sum() > 500
    d2, m2 = _images(rng, 4, 64, 90, P)                          # other images, more pixels than are resident
    assert np.array_equal(_score(g, d2, m2).conf, rs.confusion(arrays, d2, m2)[0])
    assert g.download_all_labels().tobytes() == labels.tobytes()
    g.predict_resident_boxes(1, [(0, 0, -1, -1)] * 3, False)     # the resident depth is still there
    again = g.download_all_labels()
    for i in range(3):
        assert again[i].tobytes() == rr.predict_best(arrays, d[i], 1, fill_in_gaps=False).tobytes()


# ------------------------------------------------------------------------------------------------ 8. hand-over from the renderer
@pytest.fixture(scope="module")
def toy():
    t = rtree.RTree(None, device=-1)
    assert t.loadFile(GOLD)
    return [(t.feature, t.links, t.leafData)]


def _posed(gmodel, smpl, seeds):
    rend = render.Renderer(gmodel, SMALL[0], SMALL[1], SMALL_INTRIN, max_images=len(seeds))
    rend.set_part_map(synth.identity_part_map())
    rend.upload(np.stack([synth.pose_vertices(smpl, *synth.sample_ground_truth(smpl, s)) for s in seeds]))
    rend.run(render.DEPTH | render.PART_MASK)
    imgs = [rend.download(i, render.DEPTH | render.PART_MASK) for i in range(len(seeds))]
    return rend, np.stack([x["depth"] for x in imgs]), np.stack([x["mask"] for x in imgs])


def test_score_rendered_reads_the_renderers_images(gmodel, smpl, toy):
    g = rforest.RForest([GOLD])
    rend, d, m = _posed(gmodel, smpl, (700, 701, 702))
    assert (m != 255).sum() > 300 and (d > 0).sum() > 300
    for stride in (1, 2):
        g.score_reset()
        g.score_rendered(rend, stride)
        got = g.score_get()
        host = _score(g, d, m, stride)
        ref, npx = rs.confusion(toy, d, m, stride)
        assert np.array_equal(got.conf, host.conf) and np.array_equal(got.conf, ref), stride
        assert got.n_images == 3 and got.n_pixels == host.n_pixels == npx
    assert np.trace(ref[:24, :24]) > 0
    # the renderer runs again at once, and a second score adds up
    g.score_reset()
    g.score_rendered(rend)
    first = g.score_get()
    rend.upload(np.stack([synth.pose_vertices(smpl, *synth.sample_ground_truth(smpl, s)) for s in (703, 704)]))
    rend.run(render.DEPTH | render.PART_MASK)
    g.score_rendered(rend)
    d2 = np.stack([rend.download(i, render.DEPTH)["depth"] for i in range(2)])
    m2 = np.stack([rend.download(i, render.PART_MASK)["mask"] for i in range(2)])
    total = g.score_get()
    assert total.n_images == 5 and np.array_equal(total.conf, first.conf + rs.confusion(toy, d2, m2)[0])
    # a last run without the part mask: the renderer's own message, and the totals stay
    rend.run(render.DEPTH)
    with pytest.raises(capi.AvtError, match="rendered no depth and part mask"):
        g.score_rendered(rend)
    with pytest.raises(capi.AvtError, match="stride"):
        g.score_rendered(rend, 0)
    assert np.array_equal(g.score_get().conf, total.conf)


# ------------------------------------------------------------------------------------------------ 9. scoreFromAvatar
def test_score_from_avatar_does_not_depend_on_the_batch(gmodel):
    g = rforest.RForest([GOLD])
    kw = dict(num_images=5, first_image=7, seed=3, stride=2)
    a = g.scoreFromAvatar(gmodel, SMALL_INTRIN, SMALL, batch=2, **kw)
    b = g.scoreFromAvatar(gmodel, SMALL_INTRIN, SMALL, batch=5, **kw)
    assert np.array_equal(a.conf, b.conf) and (a.n_images, a.n_pixels) == (b.n_images, b.n_pixels) == (5, 5 * 80 * 45)
    # the same five avatars by hand: randomize(idx ^ xor_key), update, render, download, score from the host images
    key = rtree_train.xor_key(3)
    ava = api.Avatar(gmodel)
    rend = render.Renderer(gmodel, SMALL[0], SMALL[1], SMALL_INTRIN, max_images=5)
    rend.set_part_map(g.partMap)
    clouds = []
    for idx in range(7, 12):
        ava.randomize(True, True, True, (idx ^ key) & 0xFFFFFFFF)
        ava.update()
        clouds.append(ava.cloud.copy())
    rend.upload(np.stack(clouds))
    rend.run(render.DEPTH | render.PART_MASK)
    imgs = [rend.download(i, render.DEPTH | render.PART_MASK) for i in range(5)]
    d, m = np.stack([x["depth"] for x in imgs]), np.stack([x["mask"] for x in imgs])
    host = _score(g, d, m, 2)
    assert np.array_equal(a.conf, host.conf) and a.conf.sum() > 100
    assert a.accuracy == rforest.score_metrics(a.conf)["accuracy"]


# ------------------------------------------------------------------------------------------------ 10. C++ facade
def _read_demo(path, P):
    raw = open(path, "rb").read()
    cells = (P + 1) * (P + 1)
    ints = np.frombuffer(raw[:8 * (cells + 4)], np.int64)
    dbl = np.frombuffer(raw[8 * (cells + 4):], np.float64)
    assert len(dbl) == 2 + 3 * P
    return ints[:cells].reshape(P + 1, P + 1), ints[cells:], dbl


def _check_metrics(conf, tail, dbl, P):
    want = rforest.score_metrics(conf)
    assert tail[2] == want["missed"] and tail[3] == want["spurious"]
    for got, key in ((dbl[0:1], "accuracy"), (dbl[1:2], "mean_iou"), (dbl[2:2 + P], "recall"), (dbl[2 + P:2 + 2 * P], "precision"), (dbl[2 + 2 * P:], "iou")):
        assert np.array_equal(got, np.atleast_1d(want[key]), equal_nan=True), key


def test_cpp_facade_scores_like_the_restatement(toy, tmp_path):
    exe = os.path.join(HERE, "cpp", "rforest_score_demo")
    assert os.path.exists(exe), "tests/cpp/rforest_score_demo not built (make -C avatar_amd/csrc facade)"
    rng = np.random.default_rng(53)
    d, m = _images(rng, 3, 37, 53, 24)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        np.array([37, 53, 3, 2], np.int32).tofile(fh)
        d.tofile(fh)
        m.tofile(fh)
    r = subprocess.run([exe, inp, outp, GOLD], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    conf, tail, dbl = _read_demo(outp, 24)
    ref, npx = rs.confusion(toy, d, m, 2)
    assert np.array_equal(conf, ref) and tail[0] == 3 and tail[1] == npx and ref.sum() > 300
    _check_metrics(conf, tail, dbl, 24)


def test_cpp_score_from_avatar(smpl, tmp_path):
    """RForest::scoreFromAvatar in batches of 2 and 5 and the same avatars through Avatar::update + AvatarRenderer +
    scoreRendered: the demo exits 1 unless the three matrices are equal"""
    from test_gpu_facade import write_model_dir
    mdir, outp = str(tmp_path / "model"), str(tmp_path / "out.bin")
    write_model_dir(smpl, mdir)
    exe = os.path.join(HERE, "cpp", "rforest_score_demo")
    r = subprocess.run([exe, "avatar", mdir, outp, "160", "90", "5", "7", "3", "1", GOLD], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    conf, tail, dbl = _read_demo(outp, 24)
    assert tail[0] == 5 and tail[1] == 5 * 160 * 90 and conf[:24].sum() > 300 and conf[24, 24] == 0
    _check_metrics(conf, tail, dbl, 24)
