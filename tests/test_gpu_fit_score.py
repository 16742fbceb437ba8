"""GPU tests of the fit score (include/avt_fitscore.h; k_fit_score in avatar_amd/csrc/avt_fitscore.hip): the (P + 1) x 7 tables of
model depth and part mask against observed depth through the C ABI, from host images, from the renderer's images on the device
and from the background subtractor's, equal entry for entry to the numpy restatement (tests/fit_score_restatement.py).  The
entries are integers: every comparison is np.array_equal on int64, none is within a tolerance.  The kernel takes one path for
every P, stride and source; a workgroup covers 64 x 16 pixels of the stride grid, four rows per lane, so 1 x 40, 17 x 33, 37 x 53
and 5 x 130 stand inside one tile, across tile rows (also at stride 2) and across tile columns."""
import os
import subprocess

import numpy as np
import pytest

import fit_score_cases as fc
import fit_score_restatement as fr
from avatar_amd import bgsub, capi, fitscore, render, rtree, synth
from avatar_amd.depth import CameraIntrin
from avatar_amd.fitscore import AGREE, IN_FRONT, BEHIND, MODEL_ONLY, DATA_ONLY, ABS_UM, ABS_UM_AGREE
from avatar_amd.tracker import MultiFrameTracker

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "forest_small.srtr")
DEMO = os.path.join(HERE, "cpp", "fit_score_demo")
SMALL_INTRIN = dict(fx=75.805, fy=75.794, cx=79.662, cy=45.874)      # the 160 x 90 camera of test_gpu_rforest_score.py
SMALL = (160, 90)
F = np.float32


# ------------------------------------------------------------------------------------------------ 1. random batches, exact
@pytest.mark.parametrize("P", fc.PARTS)
def test_random_batches_exact(P):
    rng = np.random.default_rng(100 + P)
    s = fitscore.FitScorer(P, 8)
    tols = (0.0, 0.05, np.inf, 0.08)
    k = 0
    for H, W, n in fc.BATCHES:
        R, M, D = fc.images(rng, n, H, W, P)
        bx = fc.boxes(rng, n, H, W)
        if H * W > 1:                                            # the values of D the rule names, and D == R bit for bit
            with np.errstate(invalid="ignore"):
                assert (D == 0).any() and (D < 0).any() and np.isnan(D).any() and np.isinf(D).any() and (D == fc.DENORMAL).any()
                assert ((D == R) & (R > 0)).any() and (R == 255).any() and np.isnan(R).any()
                assert ((M == 255) & (R > 0)).any() and ((M < P) & (R == 0)).any()
        for stride in fc.STRIDES:
            for boxes in (None, bx):
                tol = tols[k % len(tols)]
                k += 1
                ref = fr.tables(R, M, D, boxes, tol, stride, P)
                got = s.score_images(R, M, D, boxes, tol, stride)
                assert got.dtype == np.int64 and got.shape == (n, P + 1, 7) and np.array_equal(got, ref), (H, W, stride, tol, boxes is None)
                assert np.array_equal(s.get(), ref)
                if stride == 1000:
                    assert ref[:, :, :5].sum() <= n
    # the last, largest batches hold every class, on part rows and on row P
    ref = fr.tables(R, M, D, None, 0.05, 1, P)
    assert (ref[:, :P, :4].sum((0, 1)) > 0).all() and (ref[:, P, :5].sum(0) > 0).all() and ref[:, :P, DATA_ONLY].sum() == 0
    assert ref[:, :, ABS_UM].sum() > ref[:, :, ABS_UM_AGREE].sum() > 0


# ------------------------------------------------------------------------------------------------ 2. by hand, the tolerance's edge
def test_hand_case_and_the_tolerance_edge():
    s = fitscore.FitScorer(fc.HAND_P, 2)
    args = (fc.HAND_R, fc.HAND_M, fc.HAND_D)
    for want, kw in ((fc.HAND_TABLE, {}), (fc.HAND_TABLE_STRIDE2, dict(stride=2)), (fc.HAND_TABLE_TOL_QUARTER, dict(tol=0.25)),
                     (fc.HAND_TABLE_TOL_ZERO, dict(tol=0.0)), (fc.HAND_TABLE_TOL_INF, dict(tol=np.inf)), (fc.HAND_TABLE_WHOLE, dict(boxes=[(0, 0, -1, -1)])),
                     (fc.HAND_TABLE_WHOLE, dict(boxes=None)), (fc.HAND_TABLE_WHOLE, dict(boxes=[(5, 7, -1, 0)]))):
        kw = dict(dict(boxes=[fc.HAND_BOX], tol=fc.HAND_TOL), **kw)
        assert np.array_equal(s.score_images(*args, **kw)[0], want), kw
    # just below |delta| = 0.25 of pixel (0, 1) it is IN_FRONT again
    below = float(np.nextafter(F(0.25), F(0)))
    assert np.array_equal(s.score_images(*args, boxes=[fc.HAND_BOX], tol=below)[0], fc.HAND_TABLE)
    # +inf against +inf, the ties of the rounding, a denormal on both sides: one pixel each, as the restatement has them
    R = np.array([np.inf, 1.0, 1.0, 1.0, 1e-40, 255.0], F).reshape(6, 1, 1)
    D = np.array([np.inf, 1.0078125, 1.0234375, 1.0 + 2.0 ** -21, 1e-40, 1.0], F).reshape(6, 1, 1)
    M = np.zeros((6, 1, 1), np.uint8)
    s = fitscore.FitScorer(1, 6)
    got = s.score_images(R, M, D, tol=0.05)
    assert np.array_equal(got, fr.tables(R, M, D, None, 0.05, 1, 1))
    assert got[:, 0, ABS_UM].tolist() == [10 ** 9, 7812, 23438, 0, 0, 254000000] and got[:, 0, BEHIND].tolist() == [1, 0, 0, 0, 0, 1]


# ------------------------------------------------------------------------------------------------ 3. boxes
def test_boxes_inclusive_edges_empty_outside_and_per_image():
    P, H, W = 24, 17, 33
    rng = np.random.default_rng(31)
    R, M, _ = fc.images(rng, 7, H, W, P)
    D = np.full((7, H, W), 2.0, F)                               # data everywhere: only the box decides
    R[:] = 0                                                     # and no model: every counted pixel is DATA_ONLY
    bx = np.array([(0, 0, -1, -1), (3, 2, 30, 11), (32, 16, 32, 16), (0, 0, W - 1, H - 1), (10, 4, 9, 12), (3, 2, W, 11), (-1, 2, 30, 11)], np.int32)
    s = fitscore.FitScorer(P, 7)
    got = s.score_images(R, M, D, bx, 0.05, 1)
    assert np.array_equal(got, fr.tables(R, M, D, bx, 0.05, 1, P))
    assert got[:, P, DATA_ONLY].tolist() == [H * W, 28 * 10, 1, H * W, 0, 0, 0] and got.sum() == got[:, P, DATA_ONLY].sum()
    got = s.score_images(R, M, D, bx, 0.05, 3)                   # the grid counts from the image origin, not from the box
    assert got[:, P, DATA_ONLY].tolist() == [6 * 11, len(range(3, 31, 3)) * len(range(3, 12, 3)), 0, 6 * 11, 0, 0, 0]
    assert np.array_equal(got, fr.tables(R, M, D, bx, 0.05, 3, P))


# ------------------------------------------------------------------------------------------------ 4. 64-bit sums
@pytest.mark.parametrize("P", [1, 254])
def test_micrometre_sums_do_not_wrap_at_32_bits(P):
    s = fitscore.FitScorer(P, 2)
    for H, W in ((1, 5), (16, 64), (32, 128), (37, 53)):         # five pixels; one full workgroup; four; three partial ones
        R = np.ones((2, H, W), F)
        D = np.full((2, H, W), np.inf, F)
        M = np.full((2, H, W), P - 1, np.uint8)
        M[1] = 255
        for tol, col in ((0.05, IN_FRONT), (np.inf, AGREE)):
            got = s.score_images(R, M, D, tol=tol)
            want = np.zeros((2, P + 1, 7), np.int64)
            for i, row in ((0, P - 1), (1, P)):
                want[i, row, col] = H * W
                want[i, row, ABS_UM] = H * W * 10 ** 9
                want[i, row, ABS_UM_AGREE] = H * W * 10 ** 9 if col == AGREE else 0
            assert H * W * 10 ** 9 > 2 ** 32 and np.array_equal(got, want), (H, W, tol)
            assert np.array_equal(got, fr.tables(R, M, D, None, tol, 1, P))


# ------------------------------------------------------------------------------------------------ 5. a bad label
def test_a_bad_label_fails_the_call_only_where_it_is_selected():
    P = 24
    rng = np.random.default_rng(37)
    R, M, D = fc.images(rng, 3, 17, 33, P)
    s = fitscore.FitScorer(P, 3)
    good = s.score_images(R, M, D)
    for value, at in ((P, (2, 16, 32)), (254, (0, 0, 0)), (P, (1, 5, 7))):
        bad = M.copy()
        bad[at] = value
        R2 = R.copy()
        if at[1] == 5:
            R2[at] = 0                                           # whatever R is
        with pytest.raises(capi.AvtError, match="num_parts"):
            s.score_images(R2, bad, D)
        with pytest.raises(ValueError, match="num_parts"):
            fr.tables(R2, bad, D, None, 0.05, 1, P)
        with pytest.raises(capi.AvtError, match="no score"):
            s.get()
    assert np.array_equal(s.score_images(R, M, D), good)         # the scorer goes on working
    bad = M.copy()
    bad[1, 5, 7] = P                                             # an odd column: stride 2 does not select it
    assert np.array_equal(s.score_images(R, bad, D, stride=2), fr.tables(R, M, D, None, 0.05, 2, P))
    with pytest.raises(capi.AvtError, match="num_parts"):
        s.score_images(R, bad, D, stride=1)
    s254 = fitscore.FitScorer(254, 3)                            # P = 254: no byte is out of range
    M[0, 3, 3] = 253
    assert np.array_equal(s254.score_images(R, M, D), fr.tables(R, M, D, None, 0.05, 1, 254))


# ------------------------------------------------------------------------------------------------ 6. split independence, chunks of 65535
def test_a_batch_is_its_images_one_by_one():
    P = 24
    rng = np.random.default_rng(41)
    s = fitscore.FitScorer(P, 5)
    for H, W, n in fc.BATCHES[2:]:
        R, M, D = fc.images(rng, n, H, W, P)
        bx = fc.boxes(rng, n, H, W)
        for stride in (1, 2):
            whole = s.score_images(R, M, D, bx, 0.05, stride)
            parts = np.concatenate([s.score_images(R[i], M[i], D[i], bx[i:i + 1], 0.05, stride) for i in range(n)])
            assert np.array_equal(whole, parts) and np.array_equal(whole, fr.tables(R, M, D, bx, 0.05, stride, P))
            back = s.score_images(R[::-1], M[::-1], D[::-1], bx[::-1], 0.05, stride)
            assert np.array_equal(back, whole[::-1])
    with pytest.raises(capi.AvtError, match="created for 5"):
        s.score_images(np.zeros((6, 2, 2), F), np.zeros((6, 2, 2), np.uint8), np.zeros((6, 2, 2), F))


def test_more_images_than_one_launch_holds():
    n = 65535 + 3                                                # blockIdx.z is the image: two launches
    s = fitscore.FitScorer(1, n)
    R = np.ones((n, 1, 1), F)
    D = (np.arange(n) % 2 == 0).astype(F).reshape(n, 1, 1)       # even images agree, odd ones have no data
    M = np.where(np.arange(n) % 3 == 0, 255, 0).astype(np.uint8).reshape(n, 1, 1)
    got = s.score_images(R, M, D)
    want = np.zeros((n, 2, 7), np.int64)
    i = np.arange(n)
    want[i, np.where(i % 3 == 0, 1, 0), np.where(i % 2 == 0, AGREE, MODEL_ONLY)] = 1
    assert np.array_equal(got, want)
    for j in (0, 1, 2, 3, 65534, 65535, 65536, n - 1):
        assert np.array_equal(got[j], fr.table(R[j], M[j], D[j], None, 0.05, 1, 1)), j


# ------------------------------------------------------------------------------------------------ 7. the renderer's images
def _render(gmodel, clouds):
    rend = render.Renderer(gmodel, SMALL[0], SMALL[1], SMALL_INTRIN, max_images=len(clouds))
    rend.set_part_map(synth.identity_part_map())
    rend.upload(np.stack(clouds))
    rend.run(render.DEPTH | render.PART_MASK)
    imgs = [rend.download(i, render.DEPTH | render.PART_MASK) for i in range(len(clouds))]
    return rend, np.stack([x["depth"] for x in imgs]), np.stack([x["mask"] for x in imgs])


def test_a_rendered_avatar_against_its_own_depth(gmodel, smpl):
    P = 24
    clouds = [synth.pose_vertices(smpl, *synth.sample_ground_truth(smpl, seed)) for seed in (700, 701)]
    rend, R, M = _render(gmodel, clouds)
    covered = (R > 0).sum((1, 2))
    assert (covered > 100).all() and (R[R > 0] > 0.5).all() and ((M == 255) & (R > 0)).any()
    s = fitscore.FitScorer(P, 2)

    def score(D, tol, stride=1, boxes=None):
        got = s.score_rendered(rend, D, boxes, tol, stride)
        assert np.array_equal(got, fr.tables(R, M, D, boxes, tol, stride, P)), (tol, stride)
        assert np.array_equal(got, s.score_images(R, M, D, boxes, tol, stride))
        return got

    own = score(R, 0.0)                                          # D equal to R bit for bit, at tol 0
    assert (own[:, :, [IN_FRONT, BEHIND, MODEL_ONLY, DATA_ONLY, ABS_UM, ABS_UM_AGREE]] == 0).all()
    assert np.array_equal(own[:, :, AGREE].sum(1), covered)
    assert all(m["iou"] == 1.0 and m["agree"] == 1.0 and m["violation"] == 0.0 for m in fitscore.metrics(own))
    far = score(np.where(R > 0, R + F(0.1), 0).astype(F), 0.02)  # the surface 0.1 m behind the model: free space violated
    assert np.array_equal(far[:, :, IN_FRONT].sum(1), covered) and (far[:, :, [AGREE, BEHIND, MODEL_ONLY, DATA_ONLY]] == 0).all()
    near = score(np.where(R > 0, R - F(0.1), 0).astype(F), 0.02)
    assert np.array_equal(near[:, :, BEHIND].sum(1), covered) and (near[:, :, [AGREE, IN_FRONT, MODEL_ONLY, DATA_ONLY]] == 0).all()
    assert (abs(far[:, :, ABS_UM].sum(1) - covered * 100000) <= covered).all()       # 0.1 m each, to float32's rounding of R +- 0.1
    score(R, 0.05, 3, [(40, 10, 120, 80), (0, 0, -1, -1)])
    # the avatar moved 0.3 m in x against the same observation: both kinds of uncovered pixel, per part
    own_depth = R.copy()
    rend, R, M = _render(gmodel, [c + np.array([0.3, 0.0, 0.0]) for c in clouds])
    moved = score(own_depth, 0.05)
    assert (moved[:, :, MODEL_ONLY].sum(1) > 0).all() and (moved[:, P, DATA_ONLY] > 0).all()
    assert all(m["iou"] < 1.0 for m in fitscore.metrics(moved))
    # the renderer runs again at once; a last run without the part mask is refused with the renderer's own message
    rend.run(render.DEPTH)
    with pytest.raises(capi.AvtError, match="rendered no depth and part mask"):
        s.score_rendered(rend, R)
    with pytest.raises(capi.AvtError, match="no score"):
        s.get()
    rend.run(render.DEPTH | render.PART_MASK)
    with pytest.raises(capi.AvtError, match="created for 1"):
        fitscore.FitScorer(P, 1).score_rendered(rend, R)
    assert np.array_equal(s.score_rendered(rend, own_depth), moved)


# ------------------------------------------------------------------------------------------------ 8. from the background subtraction
@pytest.fixture(scope="module")
def scenes(smpl):
    """the depth-in tests' synthetic scenes: two streams, two steps at 480 x 640, as depth images with their camera"""
    from test_gpu_label_batch import tracker_inputs
    bgs, steps = tracker_inputs(smpl)
    rows, cols = bgs.shape[1:3]
    k = synth.K4A_INTRIN
    cam = CameraIntrin(k["fx"], k["fy"], k["cx"] - (k["width"] - cols) // 2, k["cy"] - (k["height"] - rows) // 2)
    return np.ascontiguousarray(bgs[..., 2]), [np.ascontiguousarray(s[..., 2]) for s in steps], cam


def _tracker(gmodel, bgz, cam):
    from test_gpu_bgsub import LIVE
    from test_gpu_label_batch import _policy
    rows, cols = bgz.shape[1:]
    A = MultiFrameTracker.create(gmodel, 2, 24, synth.identity_part_map(), max_points=rows * cols // 16 + 1, beta_pose=0.05, beta_shape=0.12, **_policy())
    front = bgsub.BGSubtractor(np.zeros(bgz.shape + (3,), F))
    for i in range(len(bgz)):
        front.set_background_depth(bgz[i], cam, i)
    front.nnDistThreshRel, front.neighbThreshRel = LIVE
    A.attach_front_end(front, rtree.RTree(GOLD), rtree_interval=2, dist_to_pre_weight=0.001)
    return A, front


def _reference(A, front, order, size, cam, tol, stride, whole=False):
    """the only path there was: download the renders, the masked depth and the boxes, and count on the host"""
    pm = synth.identity_part_map()
    imgs = A.render(order, size, cam, render.DEPTH | render.PART_MASK, pm)
    R, M = np.stack([x["depth"] for x in imgs]), np.stack([x["mask"] for x in imgs])
    D = np.stack([front.download(s).masked_depth for s in order])
    boxes = None if whole else [A.boxes[s][0] + A.boxes[s][1] for s in order]
    return fr.tables(R, M, D, boxes, tol, stride, 24), R, D


def test_fit_score_of_a_tracker_step(gmodel, smpl, scenes):
    bgz, steps, cam = scenes
    rows, cols = bgz.shape[1:]
    A, front = _tracker(gmodel, bgz, cam)
    size, pm = (cols, rows), synth.identity_part_map()
    posed = synth.pose_vertices(smpl, *synth.sample_ground_truth(smpl, 700))
    with pytest.raises(RuntimeError, match="no step"):
        A.fit_score([0, 1], size, cam)
    with pytest.raises(capi.AvtError, match="no run behind"):
        fitscore.FitScorer(24, 2).score_rendered_from_bgsub(_render(gmodel, [posed])[0], front)
    assert A.process_depth_images(steps[0], cam) == [True, True]
    first = {}
    for order, tol, stride in (([1, 0], 0.05, 1), ([0, 1], 0.02, 2), ([1], 0.05, 3), ([0, 0], np.inf, 1)):
        got = A.fit_score(order, size, cam, tol, stride, pm)
        ref, R, D = _reference(A, front, order, size, cam, tol, stride)
        assert got.shape == (len(order), 25, 7) and np.array_equal(got, ref), (order, tol, stride)
        first[tuple(order)] = got
    got = first[(1, 0)]
    assert (got[:, :, :3].sum((1, 2)) > 1000).all()              # model and data overlap
    # outside the box the masked depth keeps the raw scene: it counts nothing, though it is there
    ref_whole, R, D = _reference(A, front, [1, 0], size, cam, 0.05, 1, whole=True)
    for i, s in enumerate((1, 0)):
        (tlx, tly), (brx, bry) = A.boxes[s]
        outside = np.ones((rows, cols), bool)
        outside[tly:bry + 1, tlx:brx + 1] = False
        assert (D[i][outside] > 0).sum() > 10000
        assert ref_whole[i, 24, DATA_ONLY] - got[i, 24, DATA_ONLY] == ((D[i] > 0) & ~(R[i] > 0) & outside).sum() > 10000
    # without a tolerance of its own the facade's default applies
    assert np.array_equal(A.fit_score([1, 0], size, cam, part_map=pm), got)
    # the next step: the score sees the new images (stream 1 now sees its empty room: no data, its old fit is all MODEL_ONLY)
    fitted = A.process_depth_images(steps[1], cam)
    assert fitted == [True, False]
    second = A.fit_score([1, 0], size, cam, 0.05, 1, pm)
    ref, R, D = _reference(A, front, [1, 0], size, cam, 0.05, 1)
    assert np.array_equal(second, ref) and not np.array_equal(second, got)
    assert second[0, :, [AGREE, IN_FRONT, BEHIND, DATA_ONLY]].sum() == 0 and second[0, :, MODEL_ONLY].sum() == (R[0] > 0).sum() > 1000
    assert fitscore.metrics(second[0])["violation"] == 1.0 and second[1, :, :3].sum() > 1000
    # the hand-over's refusals: an index past the run, another image size
    rend = A._renderer
    sc = fitscore.FitScorer(24, 2)
    with pytest.raises(capi.AvtError, match="obs_index"):
        sc.score_rendered_from_bgsub(rend, front, [0, 2])
    with pytest.raises(capi.AvtError, match="no score"):
        sc.get()
    small, _, _ = _render(gmodel, [posed] * 2)
    with pytest.raises(capi.AvtError, match="160 x 90"):
        sc.score_rendered_from_bgsub(small, front)
    assert np.array_equal(sc.score_rendered_from_bgsub(rend, front, [1, 0]), second)      # both handles go on working


# ------------------------------------------------------------------------------------------------ 9. C++ facade
def test_cpp_scorer_on_host_images(tmp_path):
    assert os.path.exists(DEMO), "tests/cpp/fit_score_demo not built (make -C avatar_amd/csrc facade)"
    rng = np.random.default_rng(53)
    P, (H, W, n) = 24, fc.BATCHES[3]
    R, M, D = fc.images(rng, n, H, W, P)
    bx = fc.boxes(rng, n, H, W)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for boxes, tol, stride in ((bx, 0.05, 1), (None, 0.0, 2)):
        with open(inp, "wb") as fh:
            np.array([n, H, W, P, stride, boxes is not None], np.int32).tofile(fh)
            np.array([tol], F).tofile(fh)
            R.tofile(fh), M.tofile(fh), D.tofile(fh)
            if boxes is not None:
                boxes.tofile(fh)
        r = subprocess.run([DEMO, "images", inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(outp, np.int64).reshape(n, P + 1, 7)
        assert np.array_equal(got, fr.tables(R, M, D, boxes, tol, stride, P)) and got.sum() > 1000


def test_cpp_tracker_fit_score_matches_python(smpl, gmodel, scenes, tmp_path):
    """ark::MultiFrameTracker::fitScore after every step of tests/cpp/fit_score_demo's tracker, streams in descending order: the
    tables of MultiFrameTracker.fit_score on the same inputs"""
    from test_gpu_bgsub import LIVE
    from test_gpu_facade import write_model_dir
    from test_gpu_label_batch import _policy
    bgz, steps, cam = scenes
    rows, cols = bgz.shape[1:]
    pol = _policy()
    tol, stride = 0.05, 2
    mdir, inp, outp = str(tmp_path / "model"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_model_dir(smpl, mdir)
    with open(inp, "wb") as fh:
        np.array([2, len(steps), rows, cols, pol["interval"], pol["frame_icp_iters"], pol["reinit_icp_iters"], pol["reinit_cnz"], 2, stride], np.int32).tofile(fh)
        np.array(list(LIVE) + [tol], F).tofile(fh)
        np.tile(cam.as_array(), 2).tofile(fh)
        bgz.tofile(fh)
        for depths in steps:
            depths.tofile(fh)
    r = subprocess.run([DEMO, "tracker", mdir, GOLD, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    A, _ = _tracker(gmodel, bgz, cam)
    off = 0
    for t, depths in enumerate(steps):
        fitted = A.process_depth_images(depths, cam)
        fit = np.frombuffer(raw, np.int32, 2, off); off += 8
        tables = np.frombuffer(raw, np.int64, 2 * 25 * 7, off).reshape(2, 25, 7); off += 8 * 2 * 25 * 7
        assert [bool(v) for v in fit] == fitted, t
        assert np.array_equal(tables, A.fit_score([1, 0], (cols, rows), cam, tol, stride, synth.identity_part_map())), t
        assert tables.sum() > 1000
    assert off == len(raw)
