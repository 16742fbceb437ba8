"""`ark::RForest` over the C ABI of include/avt_rforest.h: several trained trees run as one forest, as the reference's tools
run any number of models (rtree-run-dataset.cpp:98-159): RTree::predict per model, the distributions added in model order in
float32, the arg-max per pixel (first part whose sum exceeds a running best that starts at 0; 255 when none does).

An RForest carries the method names the trackers call on a tree, so `FrameTracker(rtree=forest)` and
`MultiFrameTracker.attach_front_end(bgsub, forest)` work as they do with an rtree.RTree.  Inference runs on the GPU
(avatar_amd/csrc/avt_rforest.hip); there is no CPU fallback: without libavatar_hip.so every call raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .labelhandle import LabelHandle
from .rtree import RTree

RFOREST_SYMBOLS = [
    "avt_rforest_create", "avt_rforest_destroy", "avt_rforest_info", "avt_rforest_predict", "avt_rforest_predict_best",
    "avt_rforest_images_upload", "avt_rforest_predict_best_resident_boxes", "avt_rforest_predict_best_from_bgsub",
    "avt_rforest_labels_download", "avt_rforest_labels_download_all", "avt_rforest_sync",
    "avt_rforest_score_reset", "avt_rforest_score_images", "avt_rforest_score_rendered", "avt_rforest_score_get",
    "avt_rforest_labels_upload", "avt_rforest_post_process_resident", "avt_rforest_post_process_from_bgsub",
    "avt_rforest_com_pre_set", "avt_rforest_com_pre_get",
]
MAX_TREES = 16       # AVT_RFOREST_MAX_TREES


class RForest(LabelHandle):
    """`trees_or_paths`: rtree.RTree objects and / or tree files, in forest order.  The forest copies the trees; `self.trees`
    keeps the members (host-only copies for paths) for postProcess and for inspection.  Inference, the resident batch and the
    device post-processing are LabelHandle's."""
    _PREFIX = "avt_rforest"

    def __init__(self, trees_or_paths, device: int = 0):
        self._lib = capi.load_library()
        self._h = C.c_void_p()
        self.device = device
        self.trees = []
        for t in trees_or_paths:
            if isinstance(t, RTree):
                self.trees.append(t)
            else:
                tree = RTree(None, device=-1)       # members only: the forest holds the device image
                if not tree.loadFile(str(t)):
                    raise RuntimeError("RForest failed to load %s: %s" % (t, self._lib.avt_last_error().decode()))
                self.trees.append(tree)
        handles = (C.c_void_p * max(1, len(self.trees)))(*[t._h for t in self.trees])
        capi.check(self._lib.avt_rforest_create(handles, C.c_int(len(self.trees)), C.c_int(device), C.byref(self._h)))
        nt, npp, pml, pmt, nn, nl = (C.c_int() for _ in range(6))
        capi.check(self._lib.avt_rforest_info(self._h, C.byref(nt), C.byref(npp), C.byref(pml), C.byref(pmt), C.byref(nn), C.byref(nl)))
        self.numTrees, self.numParts, self.partMapType = nt.value, npp.value, pmt.value
        self.totalNodes, self.totalLeafs = nn.value, nl.value
        self.partMap = self.trees[0].partMap.copy()

    # ---- training on the GPU: tree t is what the tree's own helper gives with seed + t (mod 2^64) ----
    @classmethod
    def train_from_images(cls, n_trees, depth, part_mask, num_parts, *args, seed=0, device=0, **kw):
        """`n_trees` runs of RTree.train_from_images on the same images; the other arguments are that function's.  Tree 0 is the
        tree `RTree.train_from_images(..., seed=seed)` gives."""
        if "return_stats" in kw:
            raise TypeError("RForest.train_from_images: return_stats is the single tree's")
        return cls([RTree.train_from_images(depth, part_mask, num_parts, *args, seed=(seed + t) % (1 << 64), device=device, **kw)
                    for t in range(_count(n_trees))], device)

    @classmethod
    def trainFromAvatar(cls, n_trees, model, intrin, image_size, *args, seed=0, device=0, **kw):
        """`n_trees` runs of RTree.trainFromAvatar; tree t is trained with seed + t (mod 2^64)."""
        return cls([RTree.trainFromAvatar(model, intrin, image_size, *args, seed=(seed + t) % (1 << 64), device=device, **kw)
                    for t in range(_count(n_trees))], device)

    def postProcess(self, image, com_pre=None, interval=1, num_threads=1, top_left=(0, 0), bot_right=(-1, -1), dist_to_pre_weight=0.001):
        """RTree::postProcess through the first member tree: host code that depends on numParts and the part-map type only."""
        return self.trees[0].postProcess(image, com_pre, interval, num_threads, top_left, bot_right, dist_to_pre_weight)

    # ---- the score: a confusion matrix against ground-truth part masks (include/avt_rforest.h, THE SCORE) ----
    def score_reset(self):
        capi.check(self._lib.avt_rforest_score_reset(self._h))

    def score_images(self, depth, part_mask, stride=1):
        """Adds depth (n, rows, cols) float32 / part_mask (n, rows, cols) uint8 (255 = none), or one (rows, cols) pair, to the
        totals: every pixel of the stride grid, walked by the distribution form's rule.  A mask byte >= numParts that is not 255
        fails the call and leaves the totals as they were."""
        from .rtree_train import _images
        d, m = _images(depth, part_mask)
        capi.check(self._lib.avt_rforest_score_images(self._h, C.c_int(d.shape[0]), C.c_int(d.shape[1]), C.c_int(d.shape[2]), capi.ptr(d, C.c_float),
                                                      capi.ptr(m, C.c_ubyte), C.c_int(stride)))

    def score_rendered(self, renderer, stride=1):
        """Adds the depth and part-mask images of renderer's (render.Renderer) last DEPTH | PART_MASK run, read where they lie on
        the device; the renderer may run again as soon as this returns."""
        capi.check(self._lib.avt_rforest_score_rendered(self._h, renderer.h, C.c_int(stride)))

    def score_get(self):
        """The totals since the last reset as a Score."""
        conf = np.zeros((self.numParts + 1, self.numParts + 1), np.int64)
        ni, npx = C.c_longlong(), C.c_longlong()
        capi.check(self._lib.avt_rforest_score_get(self._h, capi.ptr(conf, C.c_longlong), C.byref(ni), C.byref(npx)))
        return Score(conf, ni.value, npx.value)

    def scoreFromAvatar(self, model, intrin, image_size, num_images=1000, first_image=0, part_map=None, seed=0, batch=64, stride=1):
        """The held-out loop, RTree.trainFromAvatar's with the score in the trainer's place: image idx in [first_image,
        first_image + num_images) is `model`'s avatar posed by Avatar.randomize(True, True, True, idx ^ xor_key(seed)), rendered
        on the GPU with `part_map` (None: the forest's own) and scored device to device, `batch` images at a time.  With the
        training run's seed and first_image = its num_images the poses are ones the forest never saw, from the same
        distribution.  Starts from a reset; returns the Score, which does not depend on `batch`."""
        from . import api, render, rtree_train
        pm = np.asarray(self.partMap if part_map is None else part_map, np.int32)
        if len(pm) == 0:
            pm = np.arange(model.numJoints(), dtype=np.int32)
        if num_images < 1 or batch < 1 or first_image < 0:
            raise ValueError("RForest.scoreFromAvatar: num_images, batch >= 1 and first_image >= 0")
        W, H = image_size
        xor_key = rtree_train.xor_key(seed)
        rend = render.Renderer(model, W, H, intrin, max_images=batch, device=self.device)
        rend.set_part_map(pm)
        ava = api.Avatar(model)
        self.score_reset()
        for i0 in range(first_image, first_image + num_images, batch):
            clouds = []
            for idx in range(i0, min(i0 + batch, first_image + num_images)):
                ava.randomize(True, True, True, (idx ^ xor_key) & 0xFFFFFFFF)
                ava.update()
                clouds.append(ava.cloud.copy())
            rend.upload(np.stack(clouds))
            rend.run(render.DEPTH | render.PART_MASK)
            self.score_rendered(rend, stride)         # device to device: the images never leave the GPU
        return self.score_get()


def score_metrics(conf):
    """The derived figures of a (P + 1, P + 1) confusion matrix conf[truth][predicted] (index P = none), in float64 from the
    integers.  A figure with a zero denominator is NaN; mean_iou is over the parts whose IoU is not NaN (NaN when there is none)."""
    c = np.asarray(conf, np.int64)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 2:
        raise ValueError("score_metrics: a square (num_parts + 1, num_parts + 1) matrix")
    P = c.shape[0] - 1
    diag = np.diagonal(c)[:P].astype(np.float64)
    row, col = c[:P].sum(1).astype(np.float64), c[:, :P].sum(0).astype(np.float64)

    def ratio(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return np.divide(a, b, out=np.full(np.shape(a), np.nan), where=b != 0)

    iou = ratio(diag, row + col - diag)
    total, count = 0.0, 0
    for v in iou.tolist():                    # added in part order, as ark::ForestScore adds them: the same double
        if v == v:
            total, count = total + v, count + 1
    return dict(accuracy=float(ratio(diag.sum(), row.sum())), recall=ratio(diag, row), precision=ratio(diag, col), iou=iou,
                mean_iou=total / count if count else float("nan"), missed=int(c[:P, P].sum()), spurious=int(c[P, :P].sum()))


class Score:
    """What score_get returns: `conf` (P + 1, P + 1) int64, n_images, n_pixels (those the stride selected), and score_metrics'
    figures as attributes (accuracy, recall, precision, iou, mean_iou, missed, spurious)."""

    def __init__(self, conf, n_images, n_pixels):
        self.conf, self.n_images, self.n_pixels = conf, int(n_images), int(n_pixels)
        self.__dict__.update(score_metrics(conf))


def _count(n_trees):
    if not 1 <= n_trees <= MAX_TREES:
        raise ValueError(f"RForest: {n_trees} trees: a forest has 1 to {MAX_TREES}")
    return n_trees
