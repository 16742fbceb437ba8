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
from .rtree import RTree

RFOREST_SYMBOLS = [
    "avt_rforest_create", "avt_rforest_destroy", "avt_rforest_info", "avt_rforest_predict", "avt_rforest_predict_best",
    "avt_rforest_images_upload", "avt_rforest_predict_best_resident_boxes", "avt_rforest_predict_best_from_bgsub",
    "avt_rforest_labels_download", "avt_rforest_labels_download_all", "avt_rforest_sync",
]
MAX_TREES = 16       # AVT_RFOREST_MAX_TREES


class RForest:
    """`trees_or_paths`: rtree.RTree objects and / or tree files, in forest order.  The forest copies the trees; `self.trees`
    keeps the members (host-only copies for paths) for postProcess and for inspection."""

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

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.avt_rforest_destroy(self._h)
            self._h = C.c_void_p()

    def predictBest(self, depth, num_threads=0, interval=1, top_left=(0, 0), bot_right=(-1, -1), fill_in_gaps=True):
        """RTree::predictBest's walk per tree (RTree.cpp:3184-3262), labels from the summed distributions; points are (x, y)."""
        d = np.ascontiguousarray(depth, np.float32)
        out = np.empty(d.shape, np.uint8)
        capi.check(self._lib.avt_rforest_predict_best(self._h, capi.ptr(d, C.c_float), C.c_int(d.shape[0]), C.c_int(d.shape[1]), C.c_int(interval),
                                                      C.c_int(top_left[0]), C.c_int(top_left[1]), C.c_int(bot_right[0]), C.c_int(bot_right[1]),
                                                      C.c_int(1 if fill_in_gaps else 0), capi.ptr(out, C.c_ubyte)))
        return out

    def predict(self, depth):
        """(numParts, H, W) float32: the trees' distributions added in tree order (0 where depth <= 0); not divided by the
        number of trees (rtree-run-dataset.cpp:124-138)."""
        d = np.ascontiguousarray(depth, np.float32)
        out = np.empty((self.numParts,) + d.shape, np.float32)
        capi.check(self._lib.avt_rforest_predict(self._h, capi.ptr(d, C.c_float), C.c_int(d.shape[0]), C.c_int(d.shape[1]), capi.ptr(out, C.c_float)))
        return out

    def postProcess(self, image, com_pre=None, interval=1, num_threads=1, top_left=(0, 0), bot_right=(-1, -1), dist_to_pre_weight=0.001):
        """RTree::postProcess through the first member tree: host code that depends on numParts and the part-map type only."""
        return self.trees[0].postProcess(image, com_pre, interval, num_threads, top_left, bot_right, dist_to_pre_weight)

    # ---- resident batch ----
    def upload_images(self, depth_stack):
        d = np.ascontiguousarray(depth_stack, np.float32)
        capi.check(self._lib.avt_rforest_images_upload(self._h, C.c_int(d.shape[0]), C.c_int(d.shape[1]), C.c_int(d.shape[2]), capi.ptr(d, C.c_float)))
        self._shape = d.shape

    def predict_resident_boxes(self, interval, boxes, fill_in_gaps=True):
        """The resident images, image i inside boxes[i] = (tl.x, tl.y, br.x, br.y), inclusive: br.x == -1 is the whole image, an
        empty box (tl > br) leaves its image all 255."""
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        n = getattr(self, "_shape", (0,))[0]
        if n and len(b) != n:
            raise ValueError(f"RForest.predict_resident_boxes: {len(b)} boxes for {n} resident images")
        capi.check(self._lib.avt_rforest_predict_best_resident_boxes(self._h, C.c_int(interval), capi.ptr(b, C.c_int), C.c_int(1 if fill_in_gaps else 0)))

    def predict_from_bgsub(self, bg, interval, fill_in_gaps=True):
        """Labels every image of `bg`'s (bgsub.BGSubtractor) last run_resident inside the box that run found, reading the masked
        depth and the boxes on the device: no copy of the depth, no host wait."""
        capi.check(self._lib.avt_rforest_predict_best_from_bgsub(self._h, bg._h, C.c_int(interval), C.c_int(1 if fill_in_gaps else 0)))
        self._shape = (bg._n,) + tuple(bg._shape[:2])

    def sync(self):
        capi.check(self._lib.avt_rforest_sync(self._h))

    def download_all_labels(self):
        out = np.empty(self._shape, np.uint8)
        capi.check(self._lib.avt_rforest_labels_download_all(self._h, capi.ptr(out, C.c_ubyte)))
        return out

    def download_labels(self, image):
        out = np.empty(self._shape[1:], np.uint8)
        capi.check(self._lib.avt_rforest_labels_download(self._h, C.c_int(image), capi.ptr(out, C.c_ubyte)))
        return out


def _count(n_trees):
    if not 1 <= n_trees <= MAX_TREES:
        raise ValueError(f"RForest: {n_trees} trees: a forest has 1 to {MAX_TREES}")
    return n_trees
