"""`ark::RTree` (RTree.h:12-184) over the C ABI of include/avt_rtree.h: the body-part forest that labels a foreground
depth image right before AvatarOptimizer::optimize() (demo.cpp:196-268).  SURVEY.md §8 row f4.

Inference runs on the GPU (avatar_amd/csrc/avt_rtree.hip); there is no CPU fallback: without libavatar_hip.so every
call raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .labelhandle import LabelHandle

RTREE_SYMBOLS = [
    "avt_rtree_create", "avt_rtree_load", "avt_rtree_export", "avt_rtree_destroy", "avt_rtree_info", "avt_rtree_get",
    "avt_rtree_predict_best", "avt_rtree_predict", "avt_rtree_images_upload", "avt_rtree_predict_best_resident", "avt_rtree_labels_download",
    "avt_rtree_sync", "avt_rtree_post_process", "avt_rtree_predict_best_resident_boxes", "avt_rtree_predict_best_from_bgsub",
    "avt_rtree_labels_download_all", "avt_rtree_labels_upload", "avt_rtree_post_process_resident", "avt_rtree_post_process_from_bgsub",
    "avt_rtree_com_pre_set", "avt_rtree_com_pre_get",
]


class RTreeDesc(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("n_leafs", C.c_int), ("num_parts", C.c_int), ("feature", C.POINTER(C.c_float)),
                ("links", C.POINTER(C.c_int)), ("leaf_data", C.POINTER(C.c_float)), ("part_map_len", C.c_int),
                ("part_map", C.POINTER(C.c_int)), ("part_map_type", C.c_int)]


class RTree(LabelHandle):
    """Same members and call protocol as the reference class: numParts, partMap, nodes / leafData (as arrays),
    loadFile, exportFile, predictBest, postProcess.  Inference, the resident batch and the device post-processing are
    LabelHandle's."""
    _PREFIX = "avt_rtree"

    def __init__(self, path: str | None = None, device: int = 0):
        self._lib = capi.load_library()
        self._h = C.c_void_p()
        self.device = device
        self.numParts = 0
        self.partMap = np.zeros(0, np.int32)
        self.partMapType = 0
        if path is not None and not self.loadFile(path):
            raise RuntimeError("RTree failed to initialize from %s" % path)     # RTree.cpp:2961-2965

    @classmethod
    def from_arrays(cls, feature, links, leaf_data, num_parts, part_map=None, part_map_type=0, device=0):
        """feature (n,5) float32 [u.x u.y v.x v.y thresh], links (n,3) int32 [lnode rnode leafid], leaf_data (nl, num_parts)."""
        self = cls(None, device)
        f = np.ascontiguousarray(feature, np.float32); l = np.ascontiguousarray(links, np.int32)
        d = np.ascontiguousarray(leaf_data, np.float32).reshape(-1, num_parts)
        pm = np.ascontiguousarray(part_map if part_map is not None else np.zeros(0), np.int32)
        desc = RTreeDesc(len(l), len(d), num_parts, capi.ptr(f, C.c_float), capi.ptr(l, C.c_int), capi.ptr(d, C.c_float), len(pm), capi.ptr(pm, C.c_int), part_map_type)
        capi.check(self._lib.avt_rtree_create(C.byref(desc), C.c_int(device), C.byref(self._h)))
        self._refresh()
        return self

    @classmethod
    def _from_handle(cls, handle, device=0):
        self = cls(None, device)
        self._h = handle
        self._refresh()
        return self

    # ---- training on the GPU (include/avt_rtree_train.h, avatar_amd/rtree_train.py) ----
    @classmethod
    def train_from_images(cls, depth, part_mask, num_parts, num_points_per_image=2000, num_features=5000, max_probe_offset=170.0,
                          min_samples=1, max_tree_depth=20, min_samples_per_feature=20, seed=0, part_map=None, part_map_type=0, batch=None,
                          device=0, return_stats=False):
        """RTree::train's V3 trainer (RTree.cpp:2338-2950) on in-memory images: depth (n, rows, cols) float32 metres, part_mask
        (n, rows, cols) uint8 (255 = none).  Defaults: `rtree-train`'s command line.  `batch` images are added per call (the tree
        does not depend on it)."""
        from . import rtree_train
        tr = rtree_train.Trainer(num_parts, num_points_per_image, num_features, max_probe_offset, min_samples, max_tree_depth,
                                 min_samples_per_feature, seed, device)
        d, m = rtree_train._images(depth, part_mask)
        step = batch or len(d)
        for i in range(0, len(d), step):
            tr.add_images(d[i:i + step], m[i:i + step])
        tree, stats = tr.run(part_map, part_map_type)
        return (tree, stats) if return_stats else tree

    @classmethod
    def trainFromAvatar(cls, model, intrin, image_size, num_threads=0, verbose=False, num_images=30000, num_points_per_image=5000,
                        num_features=2000, num_features_filtered=200, max_probe_offset=225, min_samples=100, max_tree_depth=20,
                        min_samples_per_feature=20, frac_samples_per_feature=0.01, threshes_per_feature=15, part_map=None,
                        max_images_loaded=50, mem_limit_mb=12000, train_partial_save_path="", seed=0, batch=64, device=0):
        """RTree::trainFromAvatar (include/RTree.h:112-132, the empty pose-sequence branch) with the reference's defaults: image
        idx is `model`'s avatar posed by Avatar.randomize(True, True, True, idx ^ xor_key), rendered (renderDepth /
        renderPartMask) on the GPU and handed to the trainer device to device.  Python's randomize draws from numpy's generator,
        so the poses differ from the C++ facade's (std::mt19937); xor_key is rtree_train.xor_key(seed) in both.  num_threads, num_features_filtered, frac_samples_per_feature, threshes_per_feature,
        max_images_loaded, mem_limit_mb and train_partial_save_path do not change V3's result and are ignored."""
        from . import api, render, rtree_train
        pm = np.arange(model.numJoints(), dtype=np.int32) if part_map is None else np.asarray(part_map, np.int32)
        num_parts = int(pm.max()) + 1
        W, H = image_size
        tr = rtree_train.Trainer(num_parts, num_points_per_image, num_features, float(max_probe_offset), min_samples, max_tree_depth,
                                 min_samples_per_feature, seed, device)
        xor_key = rtree_train.xor_key(seed)
        rend = render.Renderer(model, W, H, intrin, max_images=batch, device=device)
        rend.set_part_map(pm)
        ava = api.Avatar(model)
        for i0 in range(0, num_images, batch):
            k = min(batch, num_images - i0)
            clouds = []
            for idx in range(i0, i0 + k):
                ava.randomize(True, True, True, (idx ^ xor_key) & 0xFFFFFFFF)
                ava.update()
                clouds.append(ava.cloud.copy())
            rend.upload(np.stack(clouds))
            rend.run(render.DEPTH | render.PART_MASK)
            tr.add_rendered(rend)                 # device to device: the images never leave the GPU
        tree, _ = tr.run(pm, 0)
        return tree

    def trainTransfer(self, depth, part_mask):
        """RTree::trainTransfer (RTree.cpp:3332-3420) over in-memory images (n, rows, cols): leaves reached by a labelled pixel get
        the integer counts' distribution, the others keep theirs; returns how many were never reached."""
        from . import rtree_train
        return rtree_train.transfer(self, depth, part_mask)

    def _refresh(self):
        n, nl, np_, pml, pmt = (C.c_int() for _ in range(5))
        capi.check(self._lib.avt_rtree_info(self._h, C.byref(n), C.byref(nl), C.byref(np_), C.byref(pml), C.byref(pmt)))
        self.numParts, self.partMapType = np_.value, pmt.value
        self.feature = np.empty((n.value, 5), np.float32); self.links = np.empty((n.value, 3), np.int32)
        self.leafData = np.empty((nl.value, np_.value), np.float32); self.leafBestMatch = np.empty(nl.value, np.uint8)
        self.partMap = np.empty(pml.value, np.int32)
        capi.check(self._lib.avt_rtree_get(self._h, capi.ptr(self.feature, C.c_float), capi.ptr(self.links, C.c_int), capi.ptr(self.leafData, C.c_float), capi.ptr(self.leafBestMatch, C.c_ubyte),
                                           capi.ptr(self.partMap, C.c_int)))

    def loadFile(self, path: str) -> bool:
        if self._h.value:
            self._lib.avt_rtree_destroy(self._h)
            self._h = C.c_void_p()
        if self._lib.avt_rtree_load(path.encode(), C.c_int(self.device), C.byref(self._h)) != 0:
            return False
        self._refresh()
        return True

    def exportFile(self, path: str) -> bool:
        return self._lib.avt_rtree_export(self._h, path.encode()) == 0

    def postProcess(self, image, com_pre=None, interval=1, num_threads=1, top_left=(0, 0), bot_right=(-1, -1), dist_to_pre_weight=0.001):
        """In-place on `image` (H,W) uint8; com_pre (2, numParts) float64 is updated and returned (None: first frame)."""
        assert image.dtype == np.uint8 and image.flags.c_contiguous
        valid = com_pre is not None and com_pre.shape == (2, self.numParts)
        cp = np.ascontiguousarray(com_pre.T, np.float64) if valid else np.zeros((self.numParts, 2))
        capi.check(self._lib.avt_rtree_post_process(self._h, capi.ptr(image, C.c_ubyte), C.c_int(image.shape[0]), C.c_int(image.shape[1]), capi.dptr(cp),
                                                    C.c_int(1 if valid else 0), C.c_int(interval), C.c_int(top_left[0]),
                                                    C.c_int(top_left[1]), C.c_int(bot_right[0]), C.c_int(bot_right[1]),
                                                    C.c_double(dist_to_pre_weight)))
        return np.ascontiguousarray(cp.T)

    # ---- the resident batch with one box for all images (bench.py) ----
    def predict_resident(self, interval=1, top_left=(0, 0), bot_right=(-1, -1), fill_in_gaps=True):
        capi.check(self._lib.avt_rtree_predict_best_resident(self._h, C.c_int(interval), C.c_int(top_left[0]), C.c_int(top_left[1]),
                                                             C.c_int(bot_right[0]), C.c_int(bot_right[1]), C.c_int(1 if fill_in_gaps else 0)))
