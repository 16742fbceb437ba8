"""CPU tests of the device post-processing rule: the numpy / scipy restatement the GPU tests compare against is
the reference's RTree::postProcess bit for bit at interval 1, is plain connected components on the interval grid above it, and
the C ABI declares and exports the new entry points."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from avatar_amd import capi, rforest, rtree
from oracle import rtree_oracle as ro

import post_grid_restatement as pgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = 4
NEW = ["labels_upload", "post_process_resident", "post_process_from_bgsub", "com_pre_set", "com_pre_get"]


def blobs(rng, rows=40, cols=56, parts=PARTS, count=14):
    img = np.full((rows, cols), 255, np.uint8)
    for _ in range(count):
        r, c = rng.integers(0, rows - 6), rng.integers(0, cols - 8)
        img[r:r + rng.integers(2, 7), c:c + rng.integers(2, 9)] = rng.integers(0, parts)
    return img


def trees(tmp_path, ptype, parts=PARTS):
    f = np.array([[3, 0, 0, -2, 0.5], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.float32)
    l = np.array([[1, 2, -1], [-1, -1, 0], [-1, -1, 1]], np.int32)
    d = np.zeros((2, parts), np.float32); d[0, 0] = d[1, parts - 1] = 1.0
    path = str(tmp_path / f"t{ptype}.srtr")
    assert ro.OracleRTree.from_arrays(f, l, d, parts).export(path)
    names = " ".join(f"p{i}" for i in range(parts))
    with open(path + ".partmap", "w") as fh:
        fh.write("partmap %s\nsrc %d\n%s\ndest %d\n%s\n%s\n" % ("disjoint" if ptype else "contiguous", parts, names, parts, names,
                                                               "\n".join(f"p{i} p{i}" for i in range(parts))))
    prod = rtree.RTree(None, device=-1)
    assert prod.loadFile(path) and prod.partMapType == ptype
    return ro.OracleRTree.load(path), prod


def test_abi_declares_and_exports_the_device_post_processing():
    lib = capi.load_library()
    for prefix, header, symbols in (("avt_rtree_", "avt_rtree.h", rtree.RTREE_SYMBOLS), ("avt_rforest_", "avt_rforest.h", rforest.RFOREST_SYMBOLS)):
        hdr = open(os.path.join(ROOT, "include", header)).read()
        declared = set(re.findall(r"\b(%s[a-z_]+)\s*\(" % prefix, hdr))
        for name in NEW:
            assert prefix + name in declared and prefix + name in symbols and hasattr(lib, prefix + name), prefix + name
            # every declaration cites the reference function it restates
            decl = hdr.index("int %s%s(" % (prefix, name))
            assert "RTree.cpp:3422-3449" in hdr[hdr.rindex("/*", 0, decl):decl] or name == "labels_upload", name
    for cls in (rtree.RTree, rforest.RForest):
        for m in ("upload_labels", "post_process_resident", "post_process_from_bgsub", "com_pre_get", "com_pre_set"):
            assert callable(getattr(cls, m))


@pytest.mark.parametrize("ptype", [0, 1])
def test_interval_1_is_the_reference_bit_for_bit(ptype, tmp_path):
    """Three-frame sequences with the centre-of-mass memory carried over and a sub-box on the middle frame: the restatement, the
    oracle's RTree::postProcess and the product's host postProcess agree on every label byte and every com_pre double."""
    orc, prod = trees(tmp_path, ptype)
    for seed in range(40):
        rng = np.random.default_rng(1000 * ptype + seed)
        com_o = com_p = com_r = None
        for frame in range(3):
            img = blobs(rng, *((160, 240, PARTS, 150) if ptype else ()))      # disjoint: 0.05 % of the image is 19 pixels
            box = (2, 2, 51, 35) if frame == 1 else (0, 0, -1, -1)
            a, b = img.copy(), img.copy()
            kw = dict(interval=1, dist_to_pre_weight=0.01, top_left=box[:2], bot_right=box[2:])
            com_o = orc.postProcess(a, com_o, **kw)
            com_p = prod.postProcess(b, com_p, **kw)
            c, com_r = pgr.post_process(img, box, 1, com_r, 0.01, PARTS, ptype)
            assert np.array_equal(a, c) and np.array_equal(b, c), (seed, frame)
            assert np.array_equal(com_o, com_r) and np.array_equal(com_p, com_r), (seed, frame)


@pytest.mark.parametrize("interval", [2, 3])
def test_above_interval_1_every_part_keeps_one_grid_component(interval):
    for seed in range(10):
        rng = np.random.default_rng(77 * interval + seed)
        com = None
        for frame, box in enumerate(((0, 0, -1, -1), (3, 5, 50, 36), (0, 0, -1, -1))):
            img = blobs(rng)
            out, com = pgr.post_process(img, box, interval, com, 0.01, PARTS, 0)
            b = (0, 0, 55, 39) if box[2] == -1 else box
            g = pgr.grid_of(out, b, interval)
            for part in range(PARTS):
                assert ndimage.label(g == part)[1] <= 1
                assert (com[0, part] >= 0) == bool((g == part).any())
            # what is not a grid pixel's cell stays, and the cells repeat their grid pixel
            assert np.array_equal(out[:b[1]], img[:b[1]]) and np.array_equal(out[b[3] + 1:], img[b[3] + 1:])
            for a in range(1, g.shape[0]):
                r = b[1] + a * interval
                for rr in range(r, min(r + interval, b[3] + 1)):
                    assert np.array_equal(out[rr, b[0]:b[2] + 1][:g.shape[1] * interval], np.repeat(g[a], interval)[:b[2] + 1 - b[0]])


@pytest.mark.parametrize("ptype", [0, 1])
@pytest.mark.parametrize("interval", [2, 3])
def test_above_interval_1_is_the_host_rule_on_the_decimated_box(interval, ptype, tmp_path):
    """On the grid pixels the rule is the host postProcess(interval = 1) of the decimated box image.  The centres of mass live in
    different coordinates, so frames are checked without memory, and with memory at weight 0."""
    _, prod = trees(tmp_path, ptype)
    for seed in range(10):
        rng = np.random.default_rng(5 * interval + seed)
        com_r = com_h = None
        for frame, box in enumerate(((0, 0, 55, 39), (3, 5, 50, 36), (1, 0, 55, 38))):
            img = blobs(rng, 160, 240, PARTS, 200) if ptype else blobs(rng, count=30)
            if ptype:
                box = (box[0], box[1], box[2] + 180, box[3] + 120)
            out, com_r = pgr.post_process(img, box, interval, com_r, 0.0, PARTS, ptype)
            dec = np.ascontiguousarray(pgr.grid_of(img, box, interval))
            if ptype == 1:      # the threshold is taken from the image the rule is applied to: pad the decimated image to its size
                want = int((img.size // (interval * interval)) * 0.0005)
                assert want >= 2
                rows = next(r for r in range(dec.shape[0], 10 * img.shape[0]) if int(r * dec.shape[1] * 0.0005) == want)
                pad = np.full((rows, dec.shape[1]), 255, np.uint8)
                pad[:dec.shape[0]] = dec
                com_h = prod.postProcess(pad, com_h, interval=1, dist_to_pre_weight=0.0)
                dec = pad[:dec.shape[0]]
            else:
                com_h = prod.postProcess(dec, com_h, interval=1, dist_to_pre_weight=0.0)
            assert np.array_equal(pgr.grid_of(out, box, interval), dec), (seed, frame)
            assert np.array_equal(com_r[0] >= 0, com_h[0] >= 0)


def test_rule_corner_cases():
    img = np.full((6, 9), 255, np.uint8)
    img[1, 1:3] = 0; img[4, 5:7] = 0                       # two equal components: the earlier wins ...
    out, com = pgr.post_process(img, (0, 0, -1, -1), 1, None, 0.5, 1, 0)
    assert (out[1, 1:3] == 0).all() and (out[4] == 255).all() and com[:, 0].tolist() == [1.5, 1.0]
    out, com = pgr.post_process(img, (0, 0, -1, -1), 1, np.array([[5.5], [4.0]]), 0.5, 1, 0)      # ... unless the memory is on the later
    assert (out[4, 5:7] == 0).all() and (out[1] == 255).all() and com[:, 0].tolist() == [5.5, 4.0]
    out, com = pgr.post_process(img, (0, 0, -1, -1), 1, np.array([[500.0], [7.0]]), 0.5, 1, 0)    # every score <= 0
    assert (out == 255).all() and com[:, 0].tolist() == [-1.0, 7.0]
    out, com = pgr.post_process(img, (8, 5, 0, 0), 1, np.array([[3.0], [7.0]]), 0.5, 1, 0)        # an empty box
    assert np.array_equal(out, img) and com[:, 0].tolist() == [-1.0, 7.0]
    with pytest.raises(ValueError):
        pgr.post_process(np.full((3, 3), 1, np.uint8), (0, 0, -1, -1), 1, None, 0.5, 1, 0)
