"""`ark::RTree` (RTree.h:12-184) over the C ABI of include/avt_rtree.h: the body-part forest that labels a foreground
depth image right before AvatarOptimizer::optimize() (demo.cpp:196-268).  SURVEY.md §8 row f4.

Inference runs on the GPU (avatar_amd/csrc/avt_rtree.hip); there is no CPU fallback: without libavatar_hip.so every
call raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

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


class RTree:
    """Same members and call protocol as the reference class: numParts, partMap, nodes / leafData (as arrays),
    loadFile, exportFile, predictBest, postProcess."""

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

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.avt_rtree_destroy(self._h)
            self._h = C.c_void_p()

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

    def predictBest(self, depth, num_threads=0, interval=1, top_left=(0, 0), bot_right=(-1, -1), fill_in_gaps=True):
        """cv::Mat RTree::predictBest(depth, num_threads, interval, top_left, bot_right, fill_in_gaps); points are (x, y)."""
        d = np.ascontiguousarray(depth, np.float32)
        out = np.empty(d.shape, np.uint8)
        capi.check(self._lib.avt_rtree_predict_best(self._h, capi.ptr(d, C.c_float), C.c_int(d.shape[0]), C.c_int(d.shape[1]), C.c_int(interval),
                                                    C.c_int(top_left[0]), C.c_int(top_left[1]), C.c_int(bot_right[0]),
                                                    C.c_int(bot_right[1]), C.c_int(1 if fill_in_gaps else 0), capi.ptr(out, C.c_ubyte)))
        return out

    def predict(self, depth):
        """std::vector<cv::Mat> RTree::predict(depth): (numParts, H, W) float32 leaf distributions (0 where depth <= 0)."""
        d = np.ascontiguousarray(depth, np.float32)
        out = np.empty((self.numParts,) + d.shape, np.float32)
        capi.check(self._lib.avt_rtree_predict(self._h, capi.ptr(d, C.c_float), C.c_int(d.shape[0]), C.c_int(d.shape[1]), capi.ptr(out, C.c_float)))
        return out

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

    # ---- resident batch (bench.py) ----
    def upload_images(self, depth_stack):
        d = np.ascontiguousarray(depth_stack, np.float32)
        capi.check(self._lib.avt_rtree_images_upload(self._h, C.c_int(d.shape[0]), C.c_int(d.shape[1]), C.c_int(d.shape[2]), capi.ptr(d, C.c_float)))
        self._shape = d.shape

    def predict_resident(self, interval=1, top_left=(0, 0), bot_right=(-1, -1), fill_in_gaps=True):
        capi.check(self._lib.avt_rtree_predict_best_resident(self._h, C.c_int(interval), C.c_int(top_left[0]), C.c_int(top_left[1]),
                                                             C.c_int(bot_right[0]), C.c_int(bot_right[1]), C.c_int(1 if fill_in_gaps else 0)))

    def predict_resident_boxes(self, interval, boxes, fill_in_gaps=True):
        """The resident images, image i inside boxes[i] = (tl.x, tl.y, br.x, br.y), inclusive (demo.cpp:179-204 per stream):
        br.x == -1 is the whole image, an empty box (tl > br) leaves its image all 255."""
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        n = getattr(self, "_shape", (0,))[0]
        if n and len(b) != n:
            raise ValueError(f"RTree.predict_resident_boxes: {len(b)} boxes for {n} resident images")
        capi.check(self._lib.avt_rtree_predict_best_resident_boxes(self._h, C.c_int(interval), capi.ptr(b, C.c_int), C.c_int(1 if fill_in_gaps else 0)))

    def predict_from_bgsub(self, bg, interval, fill_in_gaps=True):
        """Labels every image of `bg`'s (bgsub.BGSubtractor) last run_resident inside the box that run found, reading the masked
        depth and the boxes on the device: no copy of the depth, no host wait.  download_labels / download_all_labels then
        serve these images; the tree's own resident images are gone until the next upload_images."""
        capi.check(self._lib.avt_rtree_predict_best_from_bgsub(self._h, bg._h, C.c_int(interval), C.c_int(1 if fill_in_gaps else 0)))
        self._shape = (bg._n,) + tuple(bg._shape[:2])

    # ---- postProcess for a batch on the device (include/avt_rtree.h: components on the interval grid) ----
    _PREFIX = "avt_rtree"

    def upload_labels(self, labels):
        """(n, rows, cols) uint8 label images (255 = none) become the images of the last labelling call."""
        m = np.ascontiguousarray(labels, np.uint8)
        capi.check(getattr(self._lib, self._PREFIX + "_labels_upload")(self._h, C.c_int(m.shape[0]), C.c_int(m.shape[1]), C.c_int(m.shape[2]), capi.ptr(m, C.c_ubyte)))
        self._shape = m.shape

    def post_process_resident(self, interval=1, boxes=None, dist_to_pre_weight=0.001):
        """postProcess in place on the device on every image of the last labelling call, image i inside boxes[i] = (tl.x, tl.y,
        br.x, br.y), inclusive (None: whole images; br.x == -1: the whole image; tl > br: nothing to do) with memory slot i.
        The rule is connected components on the interval grid: RTree::postProcess bit for bit at interval 1, a documented
        difference above it (include/avt_rtree.h)."""
        b = None if boxes is None else np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        n = getattr(self, "_shape", (0,))[0]
        if b is not None and n and len(b) != n:
            raise ValueError(f"post_process_resident: {len(b)} boxes for {n} images")
        capi.check(getattr(self._lib, self._PREFIX + "_post_process_resident")(self._h, C.c_int(interval), None if b is None else capi.ptr(b, C.c_int),
                                                                             C.c_double(dist_to_pre_weight)))

    def post_process_from_bgsub(self, bg, interval=1, dist_to_pre_weight=0.001):
        """post_process_resident behind predict_from_bgsub(bg, ...): every image inside the box `bg`'s last run left on the device."""
        capi.check(getattr(self._lib, self._PREFIX + "_post_process_from_bgsub")(self._h, bg._h, C.c_int(interval), C.c_double(dist_to_pre_weight)))

    def com_pre_get(self, first=0, n=1):
        """The memory of slots [first, first + n): (com_pre (n, 2, numParts) float64 as postProcess returns it per image,
        valid (n,) bool; a slot that is not sized yet reads x = -1, y = 0)."""
        com = np.empty((n, self.numParts, 2), np.float64)
        valid = np.empty(n, np.uint8)
        capi.check(getattr(self._lib, self._PREFIX + "_com_pre_get")(self._h, C.c_int(first), C.c_int(n), capi.dptr(com), capi.ptr(valid, C.c_ubyte)))
        return np.ascontiguousarray(com.transpose(0, 2, 1)), valid.astype(bool)

    def com_pre_set(self, first, com_pre, valid=None):
        """Installs com_pre (n, 2, numParts) into the slots from `first` on; valid (n,) bool, None = all sized."""
        cp = np.asarray(com_pre, np.float64)
        if cp.ndim != 3 or cp.shape[1:] != (2, self.numParts):
            raise ValueError("com_pre_set: com_pre must be (n, 2, numParts)")
        com = np.ascontiguousarray(cp.transpose(0, 2, 1))
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid, bool), np.uint8)
        capi.check(getattr(self._lib, self._PREFIX + "_com_pre_set")(self._h, C.c_int(first), C.c_int(len(com)), capi.dptr(com),
                                                                   None if v is None else capi.ptr(v, C.c_ubyte)))

    def sync(self):
        capi.check(self._lib.avt_rtree_sync(self._h))

    def download_all_labels(self):
        """(n, rows, cols) uint8: the labels of every image of the last batch call, one copy and one wait."""
        out = np.empty(self._shape, np.uint8)
        capi.check(self._lib.avt_rtree_labels_download_all(self._h, capi.ptr(out, C.c_ubyte)))
        return out

    def download_labels(self, image):
        out = np.empty(self._shape[1:], np.uint8)
        capi.check(self._lib.avt_rtree_labels_download(self._h, C.c_int(image), capi.ptr(out, C.c_ubyte)))
        return out
