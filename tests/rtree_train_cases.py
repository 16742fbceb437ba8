"""Seeded, named inputs that take the forest trainer on the GPU (avatar_amd/csrc/avt_rtree_train.hip: k_rt_img_scan, k_rt_crop, k_rt_select,
k_rt_count, k_rt_search<64> / <256>, k_rt_choose, k_rt_partition, k_rt_transfer, driven by avt_rtree_train.cpp) to the sizes at which its
kernels change behaviour: the scan's 256-stride, the ballot's 64-wide chunks, the partition's 256-wide tiles, the 2048-sample switch
between the two search forms, more than one feature per (node, chunk) workgroup, the LDS limit, the 15-bit coordinate packing, crops of
zero area, and probe offsets that leave int32.  A helper module of the tests, not a test file; no GPU is needed to build a case.

A case is a dict: name, group, depth (n, rows, cols) float32, mask (n, rows, cols) uint8, params (the Trainer's arguments: P, k, F, M,
min_samples, depth, T, seed), batches (how the images are split into add_images calls), train (False: only the samples are compared),
refuse (None, or for a refusal case a dict with the bad depth / mask batch and the pattern of the error) and promise: what the case says
about itself, written by hand.  measure(case) computes the same quantities from the arrays and the CPU restatement;
tests/test_rtree_train_edges_cpu.py compares the two, tests/test_gpu_rtree_train_edges.py runs the cases on the device."""
from __future__ import annotations

import functools

import numpy as np

import rtree_train_restatement as rst

F32 = np.float32
BASE_SEED = 20261018
LARGE = 2048                                            # train(): a node of n >= 2048 samples takes k_rt_search<256>
TARGET = {"wave": 8192, "wg": 2048}                     # workgroups per level aimed at by chunking() in train()


# ---- restated host arithmetic -----------------------------------------------------------------------------------------------------------
def lds_ints(P, T, BS):
    """rt_search_lds_ints of avt_rtree_train.hip: hist P*T | tot P | plist P | btot T | pad | gains T doubles | min, max per wave | misc 4"""
    n = P * T + 2 * P + T
    n += n & 1
    return n + 2 * T + 2 * (BS // 64) + 4


def lds_bytes(P, T, large=True):
    return 4 * lds_ints(P, T, 256 if large else 64)


def chunking(F, cnt, target):
    """(nchunks, fchunk) as train() gives them to `cnt` searched nodes of one form"""
    nch = max(1, min(F, (target + cnt - 1) // cnt)) if cnt else 1
    fch = (F + nch - 1) // nch
    return (F + fch - 1) // fch, fch


def form_of(n):
    return "wg" if n >= LARGE else "wave"


def pack_xy(x, y):
    return int(x) | (int(y) << 16)


def unpack_xy(xy):
    return xy & 0xffff, xy >> 16


def x86_int32(q):
    """(int32_t)std::round(q) of a float32 array as x86 converts: INT_MIN when the value leaves int32 or is NaN"""
    q = np.asarray(q, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.trunc(q + np.copysign(0.5, q))            # exact in double for every float32 below 2^52; beyond, q is an integer already
        r = np.where(np.abs(q) >= 2.0 ** 52, q, r)
        ok = (r >= -2.0 ** 31) & (r < 2.0 ** 31)          # NaN: False
    return np.where(ok, r, -2.0 ** 31).astype(np.int64)


def score_np(img, x, y, sd, feat):
    """scoreByFeature (RTree.cpp:52-68) in numpy for samples (x, y, sd) of one image: float32 quotients, round half away from zero,
    x86's int32 conversion, int32 wrap-around of the sum, BACKGROUND_DEPTH outside the image and on zero depth"""
    rows, cols = img.shape
    x, y, sd = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(sd, F32)

    def probe(fx, fy):
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            px = x86_int32(F32(fx) / sd) + x
            py = x86_int32(F32(fy) / sd) + y
        px = (px + 2 ** 31) % 2 ** 32 - 2 ** 31
        py = (py + 2 ** 31) % 2 ** 32 - 2 ** 31
        inside = (px >= 0) & (py >= 0) & (px < cols) & (py < rows)
        z = np.where(inside, img[np.clip(py, 0, rows - 1), np.clip(px, 0, cols - 1)], F32(20.0)).astype(F32)
        return np.where(z == 0, F32(20.0), z).astype(F32)

    with np.errstate(invalid="ignore", over="ignore"):
        s = (probe(feat[0], feat[1]) - probe(feat[2], feat[3])).astype(F32)
    return np.where(sd == 0, F32(0.0), s).astype(F32)


# ---- building blocks --------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([BASE_SEED, 41, *key])


def banded(rng, n, rows, cols, parts, zeros=0.2):
    """n images whose label is the row-major band of the pixel (parts bands), depth uniform(0.5, 4) + 0.7 label, `zeros` of them 0:
    labels correlate with depth and position, so trees split"""
    idx = np.arange(rows * cols).reshape(rows, cols)
    lab = (idx * parts // (rows * cols)).astype(np.uint8)
    m = np.broadcast_to(lab, (n, rows, cols)).copy()
    d = (rng.uniform(0.5, 4.0, (n, rows, cols)) + 0.7 * m).astype(F32)
    d[rng.random((n, rows, cols)) < zeros] = 0
    return d, m


def _params(P=4, k=64, F=8, M=30.0, min_samples=1, depth=4, T=20, seed=1):
    return dict(P=P, k=k, F=F, M=float(M), min_samples=min_samples, depth=depth, T=T, seed=seed)


def _case(name, group, d, m, params, batches=None, train=True, refuse=None, **promise):
    d = np.ascontiguousarray(d, F32)
    m = np.ascontiguousarray(m, np.uint8)
    if d.ndim == 2:
        d, m = d[None], m[None]
    assert d.shape == m.shape and d.ndim == 3
    batches = list(batches or [len(d)])
    assert sum(batches) == len(d)
    return dict(name=name, group=group, depth=d, mask=m, params=params, batches=batches, train=train, refuse=refuse, promise=promise)


def args_of(case):
    """the positional arguments shared by rtree_train.Trainer and rst.train"""
    p = case["params"]
    return (p["P"], p["k"], p["F"], p["M"], p["min_samples"], p["depth"], p["T"])


# ---- what a case is, computed -----------------------------------------------------------------------------------------------------------
_REF = {}


def reference(case):
    """the restatement's samples and (for a training case) tree of a case, computed once and shared; treat as read-only"""
    if case["name"] not in _REF:
        _REF[case["name"]] = rst.train(case["depth"], case["mask"], *args_of(case), seed=case["params"]["seed"], nthreads=8, train=case["train"])
    return _REF[case["name"]]


def levels_of(links):
    """internal nodes per level of a tree in the reference's numbering"""
    out, level = [], [0] if len(links) else []
    while level:
        inner = [i for i in level if links[i, 2] < 0]
        out.append(len(inner))
        level = [c for i in inner for c in (links[i, 0], links[i, 1])]
    return out


def box_of(d):
    ys, xs = np.nonzero(d != 0)
    return None if not len(xs) else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def measure(case):
    d, m, p = case["depth"], case["mask"], case["params"]
    out = dict(pixels=int(d.shape[1] * d.shape[2]), candidates=[int((x != 255).sum()) for x in m], boxes=[box_of(x) for x in d])
    if case["refuse"] is not None:
        return out
    ref = reference(case)
    n = len(ref["img"])
    out.update(samples=n, root_form=form_of(n) if n else None, max_x=int(ref["x"].max()) if n else -1, max_y=int(ref["y"].max()) if n else -1,
               zero_depth_samples=int((d[ref["img"], ref["y"], ref["x"]] == 0).sum()) if n else 0, lds_bytes=lds_bytes(p["P"], p["T"], n >= LARGE))
    if case["train"] and n:
        links = ref["links"]
        out.update(nodes=len(links), near=ref["near"])
        lv = levels_of(links)
        # fchunk from the internal nodes per level: a lower bound of the searched nodes, and fchunk grows with them.  A level below
        # the root is counted with the one-wave target (8192): the larger target of the two, so still a lower bound.
        out["fchunk_root"] = chunking(p["F"], 1, TARGET[form_of(n)])[1] if lv and lv[0] else 0
        out["fchunk"] = max([chunking(p["F"], c, TARGET[form_of(n)] if i == 0 else TARGET["wave"])[1] for i, c in enumerate(lv) if c] or [0])
        if len(links) > 1:
            f = ref["feature"][0]
            sc = np.concatenate([score_np(d[i], ref["x"][ref["img"] == i], ref["y"][ref["img"] == i],
                                          d[i][ref["y"][ref["img"] == i], ref["x"][ref["img"] == i]], f[:4]) for i in range(len(d))])
            with np.errstate(invalid="ignore"):
                left = int((sc < f[4]).sum())
            out["children"] = (left, n - left)
            out["on_threshold"] = int((sc == f[4]).sum())
            out["child_forms"] = tuple(sorted({form_of(left), form_of(n - left)}))
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def _scan_cases():
    cs = []
    for rows, cols in ((1, 1), (15, 17), (16, 16), (1, 257)):
        d, m = banded(_rng(1, rows, cols), 1, rows, cols, 3, zeros=0.0 if rows * cols == 1 else 0.2)
        cs.append(_case(f"scan_pixels_{rows * cols}", "scan", d, m, _params(P=3, k=300, depth=4), pixels=rows * cols, samples=rows * cols))
    # the bounding box of non-zero depth: every pixel is labelled, the depth is non-zero only inside the box, so but for `whole` labelled
    # pixels of zero depth lie outside the box and are samples (they score 0)
    R = 48
    boxes = dict(corner_tl=(0, 0, 0, 0), corner_tr=(R - 1, 0, R - 1, 0), corner_bl=(0, R - 1, 0, R - 1), corner_br=(R - 1, R - 1, R - 1, R - 1),
                 one_row=(0, 17, R - 1, 17), one_col=(29, 0, 29, R - 1), whole=(0, 0, R - 1, R - 1), inner=(10, 12, 30, 33))
    for i, (nm, (x0, y0, x1, y1)) in enumerate(boxes.items()):
        d, m = banded(_rng(2, i), 1, R, R, 4, zeros=0.0)
        keep = np.zeros((R, R), bool)
        keep[y0:y1 + 1, x0:x1 + 1] = True
        d[0][~keep] = 0
        pr = dict(zero_depth_samples=0) if nm == "whole" else {}
        cs.append(_case(f"scan_box_{nm}", "scan", d, m, _params(k=400, depth=4), boxes=[(x0, y0, x1, y1)], samples=400, **pr))
    # labelled pixels, every depth zero: the crop is 0 x 0, every score is 0, no feature has a valid threshold, the root is a leaf
    d, m = banded(_rng(3), 1, 20, 24, 4)
    d[:] = 0
    cs.append(_case("scan_zero_area_crop", "scan", d, m, _params(k=100, depth=5), boxes=[None], samples=100, zero_depth_samples=100, nodes=1))
    d, m = banded(_rng(4), 1, 32, 32, 4, zeros=0.0)
    d[0, 5, 7] = -0.0
    m[0] = 255
    m[0, 4:20, 4:20] = (np.arange(256).reshape(16, 16) // 64).astype(np.uint8)
    cs.append(_case("scan_negative_zero_depth", "scan", d, m, _params(k=256, depth=4), samples=256, zero_depth_samples=1))
    # 15-bit coordinates: labelled non-zero pixels in the first 5 and the last 40 positions, x (or y) reaches 32766
    for nm, shape in (("wide", (1, 32767)), ("tall", (32767, 1))):
        rng = _rng(5, shape[0])
        d = np.zeros(shape, F32)
        m = np.full(shape, 255, np.uint8)
        pos = np.r_[0:5, 32727:32767]
        lab = (np.arange(45) * 3 // 45).astype(np.uint8)
        d.reshape(-1)[pos] = (rng.uniform(0.5, 4.0, 45) + 0.7 * lab).astype(F32)
        m.reshape(-1)[pos] = lab
        far = dict(max_x=32766, max_y=0) if nm == "wide" else dict(max_x=0, max_y=32766)
        cs.append(_case(f"scan_15bit_{nm}", "scan", d, m, _params(P=3, k=64, M=60.0, depth=4), samples=45, pixels=32767, **far))
    # refusals: a good image first, then the refused batch; the trainer is what it was, and the next good image gets index 1
    good_d, good_m = banded(_rng(6), 1, 12, 12, 3)

    def refusal(nm, bd, bm, pattern):
        return _case(f"scan_refuse_{nm}", "scan", good_d, good_m, _params(P=3, k=50), train=False, refuse=dict(depth=bd, mask=bm, match=pattern),
                     candidates=[144])

    cs.append(refusal("32768_cols", np.ones((1, 1, 32768), F32), np.zeros((1, 1, 32768), np.uint8), "32768"))
    cs.append(refusal("32768_rows", np.ones((1, 32768, 1), F32), np.zeros((1, 32768, 1), np.uint8), "32768"))
    for nm, v in (("nan", np.nan), ("minus_one", -1.0), ("plus_inf", np.inf)):
        bd, bm = banded(_rng(7), 2, 12, 12, 3)
        bd[1, 11, 11] = v                                 # the last pixel of the second image, unlabelled or not: the depth itself is refused
        cs.append(refusal(f"depth_{nm}", bd, bm, "finite"))
    bd, bm = banded(_rng(8), 2, 12, 12, 3)
    bm[1, 0, 3] = 3
    cs.append(refusal("label_num_parts", bd, bm, "num_parts"))
    return cs


def _select_cases():
    cs = []
    for k, counts in ((5, (0, 1, 4, 5, 6)), (1, (0, 1, 2))):
        for c in counts:
            rng = _rng(10, k, c)
            d, m = banded(rng, 1, 9, 11, 3)
            keep = rng.permutation(99)[:c]
            mm = np.full(99, 255, np.uint8)
            mm[keep] = m.reshape(-1)[keep]
            cs.append(_case(f"select_k{k}_c{c}", "select", d, mm.reshape(1, 9, 11), _params(P=3, k=k), train=False, candidates=[c], samples=min(c, k)))
    for n in (63, 64, 65, 129):
        d, m = banded(_rng(11, n), 1, 1, n, 3)
        for k in (40, 200):                              # more candidates than k: the Fisher-Yates draw; no more than k: raster order
            cs.append(_case(f"select_{n}px_all_k{k}", "select", d, m, _params(P=3, k=k), train=False, candidates=[n], samples=min(n, k), pixels=n))
        for nm, pix in (("p63_p64", [p for p in (63, 64) if p < n]), ("last", [n - 1])):
            mm = np.full_like(m, 255)
            mm[0, 0, pix] = m[0, 0, pix]
            for k in ((1, 4) if len(pix) == 2 else (4,)):
                cs.append(_case(f"select_{n}px_{nm}_k{k}", "select", d, mm, _params(P=3, k=k), train=False, candidates=[len(pix)],
                                samples=min(len(pix), k), pixels=n))
    d, m = banded(_rng(12), 4, 48, 48, 4)
    m[2][m[2] == 1] = 255
    m[2].reshape(-1)[60:] = 255                          # image 2: fewer candidates than k, so the offsets of image 3 are not 3 k
    for nm, b in (("1_2_1", [1, 2, 1]), ("4", [4])):
        cs.append(_case(f"select_batches_{nm}", "select", d, m, _params(k=100), batches=b, train=False, samples=300 + int((m[2] != 255).sum())))
    return cs


def _nodes_cases():
    cs = []
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049):
        d, m = banded(_rng(20, n), 1, 48, 48, 4)
        cs.append(_case(f"nodes_root_{n}", "nodes", d, m, _params(k=n, F=16, depth=5, seed=n), samples=n, root_form=form_of(n), near=0))
    d, m = banded(_rng(21), 2, 48, 48, 4)
    cs.append(_case("nodes_both_forms_in_one_level", "nodes", d, m, _params(k=2250, F=16, depth=3, seed=BOTH_FORMS_SEED), samples=4500, root_form="wg",
                    child_forms=("wave", "wg"), near=0))
    for T in (1, 2, 63, 64, 65, 300):
        d, m = banded(_rng(22, T), 1, 48, 48, 3)
        cs.append(_case(f"nodes_T{T}", "nodes", d, m, _params(P=3, k=600, F=16, depth=4, T=T, seed=T), samples=600, near=0))
    d, m = banded(_rng(23), 1, 48, 48, 1)
    cs.append(_case("nodes_P1", "nodes", d, m, _params(P=1, k=500, F=16, depth=6), samples=500, nodes=3, near=0))
    d, m = banded(_rng(24), 1, 48, 48, 2)
    cs.append(_case("nodes_P2", "nodes", d, m, _params(P=2, k=500, F=16, depth=5), samples=500, near=0))
    d, m = banded(_rng(25), 1, 48, 48, 127)
    cs.append(_case("nodes_P127_T64_wg", "nodes", d, m, _params(P=127, k=2100, F=16, depth=4, T=64), samples=2100, root_form="wg", lds_bytes=34344, near=0))
    cs.append(_case("nodes_P127_T64_wave", "nodes", d, m, _params(P=127, k=100, F=16, depth=4, T=64), samples=100, root_form="wave", near=0))
    for P, T, nbytes in ((1, 8192, 131128), (2, 4096, 81984), (3, 2730, 65592)):
        d, m = banded(_rng(26, P), 1, 48, 48, P)
        cs.append(_case(f"nodes_lds_P{P}_T{T}_wg", "nodes", d, m, _params(P=P, k=2100, F=8, depth=3, T=T), samples=2100, root_form="wg", lds_bytes=nbytes,
                        near=0))
        cs.append(_case(f"nodes_lds_P{P}_T{T}_wave", "nodes", d, m, _params(P=P, k=100, F=8, depth=3, T=T), samples=100, root_form="wave",
                        lds_bytes=nbytes - 24, near=0))
    # small integer depths: scores are integers in [-19, 19]; FLT_EPSILON is lost in the range 38, so with T + 1 = 4 the step is exactly 9.5
    # and the root's threshold -19 + 2 x 9.5 is the 0 that every zero-depth sample (and every pair of equal probes) scores: such a sample
    # is in the bucket above the threshold and goes to the right
    rng = _rng(28)
    d, m = banded(rng, 1, 48, 48, 4)
    d = np.where(d == 0, 0, 1 + m + rng.integers(0, 2, d.shape)).astype(F32)
    cs.append(_case("nodes_scores_on_the_threshold", "nodes", d, m, _params(k=1200, F=16, depth=5, T=3), samples=1200, on_threshold=509, near=0))
    d, m = banded(_rng(27), 1, 48, 48, 4)
    cs.append(_case("nodes_min_samples_n", "nodes", d, m, _params(k=300, F=16, depth=5, min_samples=300), samples=300, nodes=1))
    cs.append(_case("nodes_min_samples_n_minus_1", "nodes", d, m, _params(k=300, F=16, depth=5, min_samples=299), samples=300, nodes=3, near=0))
    return cs


def _chunks_cases():
    """more than one feature per (node, chunk) workgroup.  `fchunk_root` is exact (one searched node); `fchunk` is the largest value over the
    levels computed from the restatement tree's internal nodes per level, a lower bound of what the device reaches"""
    cs = []
    d, m = banded(_rng(30), 1, 48, 48, 4)
    cs.append(_case("chunks_F8200_wave", "chunks", d, m, _params(k=64, F=8200, depth=3), samples=64, root_form="wave", fchunk_root=2, fchunk=3, near=0))
    cs.append(_case("chunks_F2049_wg", "chunks", d, m, _params(k=2048, F=2049, depth=2), samples=2048, root_form="wg", fchunk_root=2, fchunk=2, near=0))
    d, m = banded(_rng(31), 1, 40, 40, 5)
    cs.append(_case("chunks_F2001_deep", "chunks", d, m, _params(P=5, k=1600, F=2001, depth=9, seed=7), samples=1600, root_form="wave", fchunk_root=1,
                    fchunk=8, near=0))
    # one part: every valid threshold of every feature has the gain -0.0, so the lowest feature with a valid threshold must win: across
    # chunks (k_rt_choose; F = 2001 on one node is one feature per chunk) and inside a chunk (k_rt_search; two features per chunk)
    d, m = banded(_rng(32), 1, 40, 40, 1)
    cs.append(_case("chunks_F2001_P1_bit_equal_gains", "chunks", d, m, _params(P=1, k=1600, F=2001, depth=9), samples=1600, nodes=3, fchunk_root=1,
                    near=0))
    d, m = banded(_rng(33), 1, 48, 48, 1)
    cs.append(_case("chunks_F8200_P1_wave", "chunks", d, m, _params(P=1, k=64, F=8200, depth=3), samples=64, root_form="wave", nodes=3, fchunk_root=2,
                    near=0))
    cs.append(_case("chunks_F2049_P1_wg", "chunks", d, m, _params(P=1, k=2048, F=2049, depth=3), samples=2048, root_form="wg", nodes=3, fchunk_root=2,
                    near=0))
    return cs


ODD_DEPTHS = (1e-30, 1e-40, 3e38)                       # the quotient offset / depth leaves int32 (1e-40 is subnormal: it is infinite)


def score_images():
    """(train depth, train mask, inference depth): an ordinary image with ODD_DEPTHS mixed in under labels and beside them; the
    inference image also holds a negative and an infinite depth, which the trainer refuses"""
    rng = _rng(40)
    d, m = banded(rng, 2, 40, 44, 4)
    pos = rng.permutation(40 * 44)[:90]
    for j, p in enumerate(pos):
        d[j % 2].reshape(-1)[p] = F32(ODD_DEPTHS[j % 3])
    inf = d[1].copy()
    for j, p in enumerate(rng.permutation(40 * 44)[:40]):
        inf.reshape(-1)[p] = F32((-1.5, np.inf)[j % 2])
    return d, m, inf


def _score_cases():
    d, m, _ = score_images()
    return [_case("score_quotient_leaves_int32", "score", d, m, _params(k=1200, F=24, M=120.0, depth=6, seed=3), samples=2400, root_form="wg", near=0)]


BOTH_FORMS_SEED = 1


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_scan_cases() + _select_cases() + _nodes_cases() + _chunks_cases() + _score_cases())


def by_name(name):
    return next(c for c in cases() if c["name"] == name)
