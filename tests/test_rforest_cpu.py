"""CPU tests of the forest of several trees (include/avt_rforest.h): the numpy restatement (tests/rforest_restatement.py)
anchored bit for bit to the single-tree oracle at T = 1, the exported ABI, the headers, and host-only forests (device = -1):
what is refused at creation, the totals, and inference failing cleanly without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rforest_restatement as rr
from avatar_amd import capi, rforest, rtree
from oracle import rtree_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "forest_small.srtr")


def _random_tree(rng, depth, num_parts):
    """Random full-ish binary tree in parent-before-children order with random probe offsets and thresholds."""
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


def _image(rng, H, W):
    depth = rng.choice([0.0, 0.6, 1.5, 2.5, 7.0], (H, W), p=[0.3, 0.1, 0.3, 0.2, 0.1]).astype(np.float32)
    return depth * (1 + 0.05 * rng.standard_normal((H, W))).astype(np.float32)


def _variants(rng, H, W):
    interval = int(rng.integers(1, 6))
    x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
    x1, y1 = int(rng.integers(x0, W)), int(rng.integers(y0, H))
    return (dict(interval=interval), dict(interval=interval, fill_in_gaps=False), dict(interval=interval, top_left=(x0, y0), bot_right=(x1, y1)),
            dict(interval=1, top_left=(x0, y0), bot_right=(x1, y1), fill_in_gaps=False))


def _host_tree(arrays, num_parts, part_map=None, part_map_type=0):
    f, l, d = arrays
    return rtree.RTree.from_arrays(f, l, d, num_parts, part_map=part_map, part_map_type=part_map_type, device=-1)


# ------------------------------------------------------------------------------------------------ the restatement at T = 1
def test_restatement_equals_the_oracle_on_the_toy_tree():
    o = ro.OracleRTree.load(GOLD)
    tree = (o.feature, o.links, o.leafData)
    assert (o.leafData.max(1) > 0).all()                              # every leaf has a positive entry: arg-max == leafBestMatch
    rng = np.random.default_rng(3)
    for H, W in ((1, 1), (37, 53), (64, 90)):
        depth = _image(rng, H, W)
        for kw in _variants(rng, H, W) + (dict(interval=2), dict(interval=3, fill_in_gaps=False)):
            assert np.array_equal(rr.predict_best([tree], depth, **kw), o.predictBest(depth, **kw)), (H, W, kw)
        a, b = rr.predict([tree], depth), o.predict(depth)
        assert a.tobytes() == b.tobytes(), (H, W)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_the_oracle_on_random_trees(seed):
    rng = np.random.default_rng(seed)
    npp = int(rng.integers(2, 40))
    tree = _random_tree(rng, int(rng.integers(3, 12)), npp)
    o = ro.OracleRTree.from_arrays(*tree, npp)
    for _ in range(5):
        H, W = int(rng.integers(1, 90)), int(rng.integers(1, 120))
        depth = _image(rng, H, W)
        for kw in _variants(rng, H, W):
            assert np.array_equal(rr.predict_best([tree], depth, **kw), o.predictBest(depth, **kw)), (H, W, kw)
        assert rr.predict([tree], depth).tobytes() == o.predict(depth).tobytes(), (H, W)


def test_restatement_rule_by_hand():
    """The sum is tree 0's value + tree 1's + ... in float32, and the arg-max is the first strict improvement over 0."""
    leaf = lambda row: (np.zeros((1, 5), np.float32), np.array([[-1, -1, 0]], np.int32), np.array([row], np.float32))
    depth = np.ones((2, 2), np.float32)
    big = float(2 ** 24)
    trees = [leaf([big, big]), leaf([0, 1]), leaf([0, 1])]
    assert rr.predict(trees, depth)[:, 0, 0].tolist() == [big, big]   # (2^24 + 1) + 1 == 2^24 in float32, in this order only
    assert rr.predict_best(trees, depth, fill_in_gaps=False)[1, 0] == 0
    assert rr.predict_best(trees[::-1], depth, fill_in_gaps=False)[1, 0] == 1          # (1 + 1) + 2^24 = 2^24 + 2
    assert rr.argmax(np.array([[0, 0], [np.nan, -1], [np.nan, 2], [3, 3], [-1, 0]], np.float32)).tolist() == [255, 255, 1, 0, 255]


# ------------------------------------------------------------------------------------------------ ABI and headers
def test_abi_exports_every_symbol_of_avt_rforest_h():
    hdr = open(os.path.join(ROOT, "include", "avt_rforest.h")).read()
    declared = set(re.findall(r"\b(avt_rforest_[a-z_]+)\s*\(", hdr))
    assert declared == set(rforest.RFOREST_SYMBOLS), declared ^ set(rforest.RFOREST_SYMBOLS)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in declared:
        assert hasattr(lib, s), s


def test_public_and_facade_headers_compile(tmp_path):
    inc = os.path.join(ROOT, "include")
    for lang, std, hdr in (("c", "-std=c99", "avt_rforest.h"), ("c++", "-std=c++17", "avt_rforest.h"), ("c++", "-std=c++17", "ark/RForest.h"),
                           ("c++", "-std=c++17", "ark/FrameTracker.h"), ("c++", "-std=c++17", "ark/MultiFrameTracker.h")):
        src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
        src.write_text(f'#include "{hdr}"\n')
        subprocess.check_call(["gcc" if lang == "c" else "g++", std, "-fsyntax-only", "-Wall", "-Werror", "-I", inc, str(src)])


# ------------------------------------------------------------------------------------------------ host-only forests
def _info(forest):
    return forest.numTrees, forest.numParts, len(forest.partMap), forest.partMapType, forest.totalNodes, forest.totalLeafs


def test_host_only_forest_totals():
    rng = np.random.default_rng(11)
    pm = np.arange(7, dtype=np.int32) % 5
    arrays = [_random_tree(rng, d, 5) for d in (0, 3, 6)]
    assert len(arrays[0][1]) == 1                                      # a tree whose root is a leaf
    trees = [_host_tree(a, 5, part_map=pm, part_map_type=1) for a in arrays]
    f = rforest.RForest(trees, device=-1)
    assert _info(f) == (3, 5, 7, 1, sum(len(a[1]) for a in arrays), sum(len(a[2]) for a in arrays))
    assert np.array_equal(f.partMap, pm)
    del trees[:]                                                       # the forest copied them
    assert _info(rforest.RForest([GOLD, GOLD], device=-1))[:4] == (2, 24, 24, 0)
    one = rforest.RForest([GOLD], device=-1)
    o = ro.OracleRTree.load(GOLD)
    assert _info(one) == (1, 24, 24, 0, len(o.links), len(o.leafData))


def test_creation_refuses_bad_forests():
    rng = np.random.default_rng(12)
    t5 = _host_tree(_random_tree(rng, 3, 5), 5, part_map=np.arange(5, dtype=np.int32))
    with pytest.raises(RuntimeError, match="0 trees"):
        rforest.RForest([], device=-1)
    with pytest.raises(RuntimeError, match="17 trees"):
        rforest.RForest([t5] * 17, device=-1)
    assert rforest.RForest([t5] * 16, device=-1).numTrees == 16
    with pytest.raises(RuntimeError, match="tree 1 has num_parts 6, tree 0 has 5"):
        rforest.RForest([t5, _host_tree(_random_tree(rng, 3, 6), 6, part_map=np.arange(5, dtype=np.int32))], device=-1)
    other_map = np.arange(5, dtype=np.int32)[::-1].copy()
    with pytest.raises(RuntimeError, match="tree 2 has another part map"):
        rforest.RForest([t5, t5, _host_tree(_random_tree(rng, 3, 5), 5, part_map=other_map)], device=-1)
    with pytest.raises(RuntimeError, match="tree 1 has another part map"):       # a shorter map is another map
        rforest.RForest([t5, _host_tree(_random_tree(rng, 3, 5), 5, part_map=np.arange(4, dtype=np.int32))], device=-1)
    with pytest.raises(RuntimeError, match="tree 1 has another part-map type"):
        rforest.RForest([t5, _host_tree(_random_tree(rng, 3, 5), 5, part_map=np.arange(5, dtype=np.int32), part_map_type=1)], device=-1)
    lib = capi.load_library()
    h = ctypes.c_void_p()
    assert lib.avt_rforest_create(None, 1, -1, ctypes.byref(h)) != 0 and b"null" in lib.avt_last_error()
    assert lib.avt_rforest_info(None, None, None, None, None, None, None) != 0
    with pytest.raises(RuntimeError):
        rforest.RForest([os.path.join(ROOT, "tests", "golden", "no_such_tree.srtr")], device=-1)
    with pytest.raises(ValueError):
        rforest.RForest.train_from_images(17, None, None, 5)
    lib.avt_rforest_destroy(None)                                      # as free(NULL)


def test_inference_on_a_host_only_forest_fails_cleanly():
    f = rforest.RForest([GOLD, GOLD], device=-1)
    img = np.ones((4, 6), np.float32)
    for call in (lambda: f.predictBest(img), lambda: f.predict(img), lambda: f.upload_images(img[None]),
                 lambda: f.predict_resident_boxes(1, [[0, 0, -1, -1]]), lambda: f.sync()):
        with pytest.raises(RuntimeError, match="host-only"):
            call()
    lib = capi.load_library()
    assert lib.avt_rforest_predict_best_from_bgsub(f._h, None, 2, 1) != 0 and b"host-only" in lib.avt_last_error()
    out = np.zeros(24, np.uint8)
    assert lib.avt_rforest_labels_download(f._h, 0, capi.ptr(out, ctypes.c_ubyte)) != 0
    assert lib.avt_rforest_labels_download_all(f._h, capi.ptr(out, ctypes.c_ubyte)) != 0
    # postProcess is host code and works without a device
    lab = np.full((8, 8), 255, np.uint8)
    lab[2:6, 2:6] = 3
    com = f.postProcess(lab, None)
    assert com.shape == (2, 24) and com[0, 3] >= 0
