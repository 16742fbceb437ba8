"""What rtree.RTree and rforest.RForest share: the image side of a labelling handle (avatar_amd/csrc/avt_label.h) over the C
ABI.  A class names its entry points by `_PREFIX` ("avt_rtree", "avt_rforest"); `self._lib`, `self._h` and `self.numParts` are
the class's own."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


class LabelHandle:
    _PREFIX = None

    def _fn(self, name):
        return getattr(self._lib, self._PREFIX + name)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._fn("_destroy")(self._h)
            self._h = C.c_void_p()

    def predictBest(self, depth, num_threads=0, interval=1, top_left=(0, 0), bot_right=(-1, -1), fill_in_gaps=True):
        """cv::Mat RTree::predictBest(depth, num_threads, interval, top_left, bot_right, fill_in_gaps); points are (x, y).  A forest
        walks every tree (RTree.cpp:3184-3262) and labels from the summed distributions."""
        d = np.ascontiguousarray(depth, np.float32)
        out = np.empty(d.shape, np.uint8)
        capi.check(self._fn("_predict_best")(self._h, capi.ptr(d, C.c_float), C.c_int(d.shape[0]), C.c_int(d.shape[1]), C.c_int(interval),
                                             C.c_int(top_left[0]), C.c_int(top_left[1]), C.c_int(bot_right[0]), C.c_int(bot_right[1]),
                                             C.c_int(1 if fill_in_gaps else 0), capi.ptr(out, C.c_ubyte)))
        return out

    def predict(self, depth):
        """std::vector<cv::Mat> RTree::predict(depth): (numParts, H, W) float32 leaf distributions (0 where depth <= 0).  A forest
        adds its trees' in tree order, not divided by their number (rtree-run-dataset.cpp:124-138)."""
        d = np.ascontiguousarray(depth, np.float32)
        out = np.empty((self.numParts,) + d.shape, np.float32)
        capi.check(self._fn("_predict")(self._h, capi.ptr(d, C.c_float), C.c_int(d.shape[0]), C.c_int(d.shape[1]), capi.ptr(out, C.c_float)))
        return out

    # ---- resident batch ----
    def upload_images(self, depth_stack):
        d = np.ascontiguousarray(depth_stack, np.float32)
        capi.check(self._fn("_images_upload")(self._h, C.c_int(d.shape[0]), C.c_int(d.shape[1]), C.c_int(d.shape[2]), capi.ptr(d, C.c_float)))
        self._shape = d.shape

    def predict_resident_boxes(self, interval, boxes, fill_in_gaps=True):
        """The resident images, image i inside boxes[i] = (tl.x, tl.y, br.x, br.y), inclusive (demo.cpp:179-204 per stream):
        br.x == -1 is the whole image, an empty box (tl > br) leaves its image all 255."""
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        n = getattr(self, "_shape", (0,))[0]
        if n and len(b) != n:
            raise ValueError(f"{type(self).__name__}.predict_resident_boxes: {len(b)} boxes for {n} resident images")
        capi.check(self._fn("_predict_best_resident_boxes")(self._h, C.c_int(interval), capi.ptr(b, C.c_int), C.c_int(1 if fill_in_gaps else 0)))

    def predict_from_bgsub(self, bg, interval, fill_in_gaps=True):
        """Labels every image of `bg`'s (bgsub.BGSubtractor) last run_resident inside the box that run found, reading the masked
        depth and the boxes on the device: no copy of the depth, no host wait.  download_labels / download_all_labels then
        serve these images; the handle's own resident images are gone until the next upload_images."""
        capi.check(self._fn("_predict_best_from_bgsub")(self._h, bg._h, C.c_int(interval), C.c_int(1 if fill_in_gaps else 0)))
        self._shape = (bg._n,) + tuple(bg._shape[:2])

    # ---- postProcess for a batch on the device (include/avt_rtree.h: components on the interval grid) ----
    def upload_labels(self, labels):
        """(n, rows, cols) uint8 label images (255 = none) become the images of the last labelling call."""
        m = np.ascontiguousarray(labels, np.uint8)
        capi.check(self._fn("_labels_upload")(self._h, C.c_int(m.shape[0]), C.c_int(m.shape[1]), C.c_int(m.shape[2]), capi.ptr(m, C.c_ubyte)))
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
        capi.check(self._fn("_post_process_resident")(self._h, C.c_int(interval), None if b is None else capi.ptr(b, C.c_int), C.c_double(dist_to_pre_weight)))

    def post_process_from_bgsub(self, bg, interval=1, dist_to_pre_weight=0.001):
        """post_process_resident behind predict_from_bgsub(bg, ...): every image inside the box `bg`'s last run left on the device."""
        capi.check(self._fn("_post_process_from_bgsub")(self._h, bg._h, C.c_int(interval), C.c_double(dist_to_pre_weight)))

    def com_pre_get(self, first=0, n=1):
        """The memory of slots [first, first + n): (com_pre (n, 2, numParts) float64 as postProcess returns it per image,
        valid (n,) bool; a slot that is not sized yet reads x = -1, y = 0)."""
        com = np.empty((n, self.numParts, 2), np.float64)
        valid = np.empty(n, np.uint8)
        capi.check(self._fn("_com_pre_get")(self._h, C.c_int(first), C.c_int(n), capi.dptr(com), capi.ptr(valid, C.c_ubyte)))
        return np.ascontiguousarray(com.transpose(0, 2, 1)), valid.astype(bool)

    def com_pre_set(self, first, com_pre, valid=None):
        """Installs com_pre (n, 2, numParts) into the slots from `first` on; valid (n,) bool, None = all sized."""
        cp = np.asarray(com_pre, np.float64)
        if cp.ndim != 3 or cp.shape[1:] != (2, self.numParts):
            raise ValueError("com_pre_set: com_pre must be (n, 2, numParts)")
        com = np.ascontiguousarray(cp.transpose(0, 2, 1))
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid, bool), np.uint8)
        capi.check(self._fn("_com_pre_set")(self._h, C.c_int(first), C.c_int(len(com)), capi.dptr(com), None if v is None else capi.ptr(v, C.c_ubyte)))

    def sync(self):
        capi.check(self._fn("_sync")(self._h))

    def download_all_labels(self):
        """(n, rows, cols) uint8: the labels of every image of the last batch call, one copy and one wait."""
        out = np.empty(self._shape, np.uint8)
        capi.check(self._fn("_labels_download_all")(self._h, capi.ptr(out, C.c_ubyte)))
        return out

    def download_labels(self, image):
        out = np.empty(self._shape[1:], np.uint8)
        capi.check(self._fn("_labels_download")(self._h, C.c_int(image), capi.ptr(out, C.c_ubyte)))
        return out
