"""The forest trainer on the GPU over the C ABI of include/avt_rtree_train.h: RTree::trainFromAvatar's V3 trainer
(RTree.cpp:2338-2950) fed with in-memory images, and RTree::trainTransfer (:3332-3420).  `rtree.RTree.train_from_images`,
`RTree.trainFromAvatar` and `RTree.trainTransfer` are the entry points; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

TRAIN_SYMBOLS = [
    "avt_rtree_trainer_create", "avt_rtree_trainer_destroy", "avt_rtree_trainer_add_images", "avt_rtree_trainer_info",
    "avt_rtree_trainer_samples", "avt_rtree_trainer_run", "avt_rtree_transfer_images", "avt_rtree_trainer_add_rendered",
    "avt_rtree_trainer_root_histograms", "avt_rtree_transfer_rendered", "avt_rtree_transfer_finish",
]
M64 = (1 << 64) - 1


def _sm64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def xor_key(seed):
    """avt_rt_xor_key (include/avt_rtree_train.h): trainFromAvatar's xorKey from the seed, Python integers (64-bit wrap)."""
    k = _sm64(_sm64(_sm64(seed & M64) ^ 0x786f726b65792121) ^ 0) >> 32
    return k or 1
MAX_DEPTH = 64


class TrainParams(C.Structure):
    _fields_ = [("num_parts", C.c_int), ("num_points_per_image", C.c_int), ("num_features", C.c_int), ("max_probe_offset", C.c_float),
                ("min_samples", C.c_int), ("max_tree_depth", C.c_int), ("min_samples_per_feature", C.c_int), ("seed", C.c_uint64)]


class TrainStats(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("n_leafs", C.c_int), ("n_levels", C.c_int), ("n_images", C.c_int), ("n_samples", C.c_longlong),
                ("total_ms", C.c_double), ("level_nodes", C.c_int * MAX_DEPTH), ("level_searched", C.c_int * MAX_DEPTH),
                ("level_evals", C.c_longlong * MAX_DEPTH), ("level_ms", C.c_double * MAX_DEPTH), ("level_large", C.c_int * MAX_DEPTH)]

    def as_dict(self):
        L = self.n_levels
        return dict(n_nodes=self.n_nodes, n_leafs=self.n_leafs, n_levels=L, n_images=self.n_images, n_samples=self.n_samples,
                    total_ms=self.total_ms, level_nodes=list(self.level_nodes[:L]), level_searched=list(self.level_searched[:L]),
                    level_evals=list(self.level_evals[:L]), level_ms=list(self.level_ms[:L]), level_large=list(self.level_large[:L]))


def _images(depth, part_mask):
    d = np.ascontiguousarray(depth, np.float32)
    m = np.ascontiguousarray(part_mask, np.uint8)
    if d.ndim == 2:
        d, m = d[None], m[None]
    if d.ndim != 3 or d.shape != m.shape:
        raise ValueError("depth and part_mask must be (n, rows, cols) (or one (rows, cols) image) of the same shape")
    return d, m


class Trainer:
    """One tree's training state on the device: images are added (and sampled) in any batching, run() trains."""

    def __init__(self, num_parts, num_points_per_image=2000, num_features=5000, max_probe_offset=170.0, min_samples=1, max_tree_depth=20,
                 min_samples_per_feature=20, seed=0, device=0):
        self._lib = capi.load_library()
        self._h = C.c_void_p()
        self.num_parts = num_parts
        self.device = device
        self._T = min_samples_per_feature
        p = TrainParams(num_parts, num_points_per_image, num_features, max_probe_offset, min_samples, max_tree_depth, min_samples_per_feature,
                        seed & 0xFFFFFFFFFFFFFFFF)
        capi.check(self._lib.avt_rtree_trainer_create(C.c_int(device), C.byref(p), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.avt_rtree_trainer_destroy(self._h)
            self._h = C.c_void_p()

    def add_images(self, depth, part_mask):
        d, m = _images(depth, part_mask)
        capi.check(self._lib.avt_rtree_trainer_add_images(self._h, C.c_int(d.shape[0]), C.c_int(d.shape[1]), C.c_int(d.shape[2]),
                                                          capi.ptr(d, C.c_float), capi.ptr(m, C.c_ubyte)))

    def add_rendered(self, renderer):
        """the depth and part-mask images of renderer's (render.Renderer) last run, device to device"""
        capi.check(self._lib.avt_rtree_trainer_add_rendered(self._h, renderer.h))

    def root_histograms(self, n_features):
        """(n_features, num_parts, T) int32 bucket histograms of the root's first features as the device counts them, and the
        (n_features, 2) min / max of their scores"""
        T = self._T
        h = np.empty((n_features, self.num_parts, T), np.int32)
        mm = np.empty((n_features, 2), np.float32)
        capi.check(self._lib.avt_rtree_trainer_root_histograms(self._h, C.c_int(n_features), capi.ptr(h, C.c_int),
                                                               capi.ptr(mm, C.c_float)))
        return h, mm

    def info(self):
        ni, ns = C.c_int(), C.c_longlong()
        capi.check(self._lib.avt_rtree_trainer_info(self._h, C.byref(ni), C.byref(ns)))
        return ni.value, ns.value

    def samples(self):
        """(image, x, y, label) arrays in the trainer's order (image-major, in the order each image's samples were chosen)."""
        _, n = self.info()
        img, x, y = (np.empty(n, np.int32) for _ in range(3))
        lab = np.empty(n, np.uint8)
        capi.check(self._lib.avt_rtree_trainer_samples(self._h, capi.ptr(img, C.c_int), capi.ptr(x, C.c_int), capi.ptr(y, C.c_int),
                                                       capi.ptr(lab, C.c_ubyte)))
        return img, x, y, lab

    def run(self, part_map=None, part_map_type=0):
        """(RTree, stats dict): the trained tree on the trainer's device."""
        from .rtree import RTree
        pm = np.ascontiguousarray(part_map if part_map is not None else np.zeros(0), np.int32)
        h = C.c_void_p()
        st = TrainStats()
        capi.check(self._lib.avt_rtree_trainer_run(self._h, C.c_int(len(pm)), capi.ptr(pm, C.c_int), C.c_int(part_map_type),
                                                   C.byref(h), C.byref(st)))
        return RTree._from_handle(h, self.device), st.as_dict()


def transfer(tree, depth, part_mask):
    """RTree::trainTransfer over in-memory images: the tree's leaf distributions are re-fitted in place; returns the number of
    leaves never reached (they keep their weights)."""
    d, m = _images(depth, part_mask)
    z = C.c_int()
    capi.check(tree._lib.avt_rtree_transfer_images(tree._h, C.c_int(d.shape[0]), C.c_int(d.shape[1]), C.c_int(d.shape[2]),
                                                   capi.ptr(d, C.c_float), capi.ptr(m, C.c_ubyte),
                                                   C.byref(z)))
    tree._refresh()
    return z.value


def transfer_rendered(tree, renderer):
    """adds the trainTransfer counts of renderer's last depth + part-mask run (device to device); transfer_finish applies them"""
    capi.check(tree._lib.avt_rtree_transfer_rendered(tree._h, renderer.h))


def transfer_finish(tree):
    z = C.c_int()
    capi.check(tree._lib.avt_rtree_transfer_finish(tree._h, C.byref(z)))
    tree._refresh()
    return z.value
