"""The image side that a tree and a forest share (avatar_amd/csrc/avt_label.cpp, avatar_amd/labelhandle.py): one call sequence
on a random tree and on the one-tree forest made from it.  Labels are bytes and the centres of mass are doubles from exact
integer sums, so at every step the two kinds are compared with np.array_equal, and both with the restatements
(tests/rforest_restatement.py for the labelling, tests/post_grid_restatement.py for the device post-processing).  3 images of
37 x 53 (no multiple of the 16 x 16 tile, more than one block), intervals 1 and 3, one whole-image box (br.x == -1), one empty box
and one that ends on the last row and column."""
import numpy as np
import pytest

import post_grid_restatement as pgr
import rforest_restatement as rr
from avatar_amd import bgsub, capi, rforest, rtree
from test_rforest_cpu import _image, _random_tree

pytestmark = pytest.mark.gpu
PARTS, N, ROWS, COLS = 5, 3, 37, 53
BOXES = [(0, 0, -1, -1), (10, 10, 5, 5), (20, 15, COLS - 1, ROWS - 1)]
WEIGHT = 0.001


@pytest.fixture(scope="module")
def kinds():
    rng = np.random.default_rng(2024)
    arrays = _random_tree(rng, 6, PARTS)
    tree = rtree.RTree.from_arrays(*arrays, PARTS, part_map=np.arange(PARTS))
    forest = rforest.RForest([tree])
    depth = np.stack([_image(rng, ROWS, COLS) for _ in range(N)])
    return arrays, (tree, forest), depth


def _both(handles, call):
    """the call's result on the tree, after asserting that the forest gives the same bytes"""
    a, b = (call(h) for h in handles)
    if isinstance(a, tuple):
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
    elif a is not None:
        assert np.array_equal(a, b) and a.dtype == b.dtype
    return a


@pytest.mark.parametrize("interval", [1, 3])
def test_one_sequence_on_both_kinds(kinds, interval):
    arrays, handles, depth = kinds
    _both(handles, lambda h: h.upload_images(depth))
    _both(handles, lambda h: h.predict_resident_boxes(interval, BOXES))
    labels = _both(handles, lambda h: h.download_all_labels())
    for i in range(N):
        assert np.array_equal(labels[i], rr.predict_best_box_on_device([arrays], depth[i], BOXES[i] if i else (0, 0, COLS - 1, ROWS - 1), interval)), i
    assert (labels[0] != 255).sum() > 100 and (labels[1] == 255).all() and (labels[2][:15] == 255).all() and (labels[2][ROWS - 1] != 255).any()
    # the labels come back as another classifier's; every slot starts not sized
    _both(handles, lambda h: h.com_pre_set(0, np.zeros((N, 2, PARTS)), [False] * N))
    _both(handles, lambda h: h.upload_labels(labels))
    _both(handles, lambda h: h.post_process_resident(interval, BOXES, WEIGHT))
    post = _both(handles, lambda h: h.download_all_labels())
    com, valid = _both(handles, lambda h: h.com_pre_get(0, N))
    assert valid.all()
    for i in range(N):
        want, want_com = pgr.post_process(labels[i], BOXES[i], interval, None, WEIGHT, PARTS, 0)
        assert np.array_equal(post[i], want) and np.array_equal(com[i], want_com), i
    assert (post[0] != labels[0]).any() and np.array_equal(post[1], labels[1]) and (com[1][0] == -1).all()
    # the memory round trip, slot 1 put back to "not sized"
    moved = com + 0.5
    _both(handles, lambda h: h.com_pre_set(0, moved, [True, False, True]))
    back, valid = _both(handles, lambda h: h.com_pre_get(0, N))
    assert valid.tolist() == [True, False, True] and np.array_equal(back[0], moved[0]) and np.array_equal(back[2], moved[2])
    for i in range(N):
        assert np.array_equal(_both(handles, lambda h: h.download_labels(i)), post[i]), i


def test_the_hand_over_from_bgsub_on_both_kinds(kinds):
    arrays, handles, _ = kinds
    bg = np.zeros((N, ROWS, COLS, 3), np.float32)
    xyz = np.zeros_like(bg)
    xyz[0, 5:31, 8:46] = (0.1, 0.1, 1.5)                 # one component inside the image
    xyz[1, 12:, 30:] = (0.1, 0.1, 2.5)                   # one that ends on the last row and column; image 2 is empty
    front = bgsub.BGSubtractor(bg)
    front.nnDistThreshRel, front.neighbThreshRel = 0.005, 0.005
    for interval in (1, 3):
        front.upload(xyz)
        front.run_resident()
        _both(handles, lambda h: h.com_pre_set(0, np.zeros((N, 2, PARTS)), [False] * N))
        _both(handles, lambda h: h.predict_from_bgsub(front, interval))
        labels = _both(handles, lambda h: h.download_all_labels())
        _both(handles, lambda h: h.post_process_from_bgsub(front, interval, WEIGHT))
        post = _both(handles, lambda h: h.download_all_labels())
        com, valid = _both(handles, lambda h: h.com_pre_get(0, N))
        assert valid.all()
        for i in range(N):
            res = front.download(i)
            box = res.topLeft + res.botRight
            assert np.array_equal(labels[i], rr.predict_best_box_on_device([arrays], res.masked_depth, box, interval)), (interval, i)
            want, want_com = pgr.post_process(labels[i], box, interval, None, WEIGHT, PARTS, 0)
            assert np.array_equal(post[i], want) and np.array_equal(com[i], want_com), (interval, i)
        assert (labels[0] != 255).sum() > 50 and (labels[1][ROWS - 1] != 255).any() and (labels[2] == 255).all()
    # the handles have no resident depth of their own after the hand-over
    for h in handles:
        with pytest.raises(capi.AvtError, match="no images resident"):
            h.predict_resident_boxes(1, BOXES)
