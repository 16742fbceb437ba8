"""`ark::BGSubtractor` (BGSubtractor.h, BGSubtractor.cpp:10-163) over the C ABI of include/avt_bgsub.h: the background
subtraction that opens every frame of the reference's trackers (demo.cpp:179-192, live-demo.cpp:317-332).

Runs on the GPU (avatar_amd/csrc/avt_bgsub.hip); there is no CPU fallback: without libavatar_hip.so every call raises.
Points are (x, y) as cv::Point; an XYZ map is (rows, cols, 3) float32."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .depth import depth_to_xyz, intrin_array

BGSUB_SYMBOLS = [
    "avt_bgsub_create", "avt_bgsub_destroy", "avt_bgsub_set_background", "avt_bgsub_run", "avt_bgsub_images_upload",
    "avt_bgsub_run_resident", "avt_bgsub_download", "avt_bgsub_sync", "avt_bgsub_depth_upload", "avt_bgsub_run_depth",
    "avt_bgsub_set_background_depth", "avt_bgsub_xyz_download",
]
MAX_COMPS = 254
DEVICE_FAULT = 3        # AVT_STATUS_DEVICE_FAULT (include/avt.h)


class Frame(C.Structure):
    """avt_bgsub_frame"""
    _fields_ = [("top_left", C.c_int * 2), ("bot_right", C.c_int * 2), ("capped", C.c_int), ("fg_count", C.c_int), ("n_comps", C.c_int),
                ("comps", (C.c_int * 2) * MAX_COMPS)]


def _xyz(a, shape):
    a = np.ascontiguousarray(a, np.float32)
    if a.shape[-3:] != shape:
        raise ValueError(f"BGSubtractor: image shape {a.shape} does not match the background's {shape}")
    return a


def _depth(a, shape):
    a = np.ascontiguousarray(a, np.float32)
    if a.shape[-2:] != shape[:2]:
        raise ValueError(f"BGSubtractor: depth image shape {a.shape} does not match the background's {shape[:2]}")
    return a


class Result:
    """One image's outputs: mask (rows, cols) uint8, masked_depth (rows, cols) float32, topLeft / botRight (x, y),
    capped, fg_count (live-demo.cpp's subCnz) and comps_by_size [(size, id), ...]."""

    def __init__(self, mask, depth, fr):
        self.mask, self.masked_depth = mask, depth
        self.topLeft = (fr.top_left[0], fr.top_left[1])
        self.botRight = (fr.bot_right[0], fr.bot_right[1])
        self.capped, self.fg_count = bool(fr.capped), fr.fg_count
        self.comps_by_size = [(fr.comps[i][0], fr.comps[i][1]) for i in range(fr.n_comps)]


class BGSubtractor:
    """Same members and call protocol as the reference class: nnDistThreshRel, neighbThreshRel, numThreads (accepted,
    unused), background, topLeft, botRight, run(image, comps_by_size).  After run(), maskedDepth and fgCount hold the
    demos' use of the mask.  `background` may be one XYZ map or a stack of them (the batch form picks per image)."""

    def __init__(self, background, device: int = 0):
        self._lib = capi.load_library()
        self._h = C.c_void_p()
        self.nnDistThreshRel = 0.005
        self.neighbThreshRel = 0.005
        self.numThreads = 1
        self.topLeft = (0, 0)
        self.botRight = (0, 0)
        self.maskedDepth = None
        self.fgCount = 0
        self.capped = False
        bgs = np.ascontiguousarray(background, np.float32)
        if bgs.ndim == 3:
            bgs = bgs[None]
        if bgs.ndim != 4 or bgs.shape[3] != 3:
            raise ValueError("BGSubtractor: background must be (rows, cols, 3) or (n, rows, cols, 3)")
        self._shape = bgs.shape[1:]
        self._bgs = bgs.copy()
        capi.check(self._lib.avt_bgsub_create(C.c_int(device), C.c_int(bgs.shape[0]), C.c_int(bgs.shape[1]), C.c_int(bgs.shape[2]),
                                              capi.ptr(bgs, C.c_float), C.byref(self._h)))
        self._n = 0

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.avt_bgsub_destroy(self._h)
            self._h = C.c_void_p()

    @property
    def background(self):
        return self._bgs[0] if len(self._bgs) == 1 else self._bgs

    @background.setter
    def background(self, xyz):                   # live-demo.cpp:207
        self.set_background(xyz, 0)

    def set_background(self, xyz, index=0):
        a = _xyz(xyz, self._shape)
        capi.check(self._lib.avt_bgsub_set_background(self._h, C.c_int(index), capi.ptr(a, C.c_float)))
        self._bgs[index] = a

    def set_background_depth(self, depth, intrin, index=0):
        """set_background from a depth image (rows, cols) and its camera: expanded on the device (CameraIntrin::depthToXYZ)."""
        a = _depth(depth, self._shape)
        if a.ndim != 2:
            raise ValueError("BGSubtractor.set_background_depth: one (rows, cols) depth image")
        k = intrin_array(intrin, 1)
        capi.check(self._lib.avt_bgsub_set_background_depth(self._h, C.c_int(index), capi.ptr(a, C.c_float), capi.ptr(k, C.c_float)))
        self._bgs[index] = depth_to_xyz(a, k[0])

    def run(self, image, comps_by_size=False, background_index=0):
        """cv::Mat BGSubtractor::run(image, comps_by_size) (BGSubtractor.cpp:159-163): the mask; with comps_by_size
        True returns (mask, [(size, id), ...])."""
        a = _xyz(image, self._shape)
        return self._run(self._lib.avt_bgsub_run, (capi.ptr(a, C.c_float),), comps_by_size, background_index)

    def run_depth(self, depth, intrin, comps_by_size=False, background_index=0):
        """run() on a depth image (rows, cols) and its camera (a depth.CameraIntrin or fx, fy, cx, cy): the XYZ map is
        built on the device, bit for bit depth.depth_to_xyz."""
        a = _depth(depth, self._shape)
        if a.ndim != 2:
            raise ValueError("BGSubtractor.run_depth: one (rows, cols) depth image")
        k = intrin_array(intrin, 1)
        return self._run(self._lib.avt_bgsub_run_depth, (capi.ptr(a, C.c_float), capi.ptr(k, C.c_float)), comps_by_size, background_index)

    def _run(self, entry, source, comps_by_size, background_index):
        mask = np.empty(self._shape[:2], np.uint8)
        depth = np.empty(self._shape[:2], np.float32)
        fr = Frame()
        fr.top_left[:] = self.topLeft
        fr.bot_right[:] = self.botRight
        capi.check(entry(self._h, C.c_int(background_index), *source, C.c_float(self.nnDistThreshRel), C.c_float(self.neighbThreshRel),
                         capi.ptr(mask, C.c_ubyte), capi.ptr(depth, C.c_float), C.byref(fr)))
        self._n = 1
        res = Result(mask, depth, fr)
        self.topLeft, self.botRight, self.maskedDepth, self.fgCount, self.capped = res.topLeft, res.botRight, depth, res.fg_count, res.capped
        return (mask, res.comps_by_size) if comps_by_size else mask

    # ---- resident batch: many streams, or a recorded sequence ----
    def upload(self, images, bg_index=None, prev_boxes=None):
        """images (n, rows, cols, 3); bg_index (n,) background of every image (None: image i against background i);
        prev_boxes (n, 4) tl.x tl.y br.x br.y (None: every slot keeps the box of its previous run)."""
        a = _xyz(images, self._shape)
        n = a.shape[0]
        bi = None if bg_index is None else np.ascontiguousarray(bg_index, np.int32)
        pb = None if prev_boxes is None else np.ascontiguousarray(prev_boxes, np.int32).reshape(n, 4)
        capi.check(self._lib.avt_bgsub_images_upload(self._h, C.c_int(n), capi.ptr(a, C.c_float), capi.ptr(bi, C.c_int),
                                                     capi.ptr(pb, C.c_int)))
        self._n = n

    def upload_depth(self, depth, intrin, bg_index=None, prev_boxes=None):
        """upload() from depth images (n, rows, cols) and `intrin`, one camera for all of them or (n, 4) fx fy cx cy: a
        third of the bytes cross the bus, the XYZ maps are built on the device."""
        a = _depth(depth, self._shape)
        if a.ndim != 3:
            raise ValueError("BGSubtractor.upload_depth: depth images must be (n, rows, cols)")
        n = a.shape[0]
        k = intrin_array(intrin, n)
        bi = None if bg_index is None else np.ascontiguousarray(bg_index, np.int32)
        pb = None if prev_boxes is None else np.ascontiguousarray(prev_boxes, np.int32).reshape(n, 4)
        capi.check(self._lib.avt_bgsub_depth_upload(self._h, C.c_int(n), capi.ptr(a, C.c_float), capi.ptr(k, C.c_float),
                                                    capi.ptr(bi, C.c_int), capi.ptr(pb, C.c_int)))
        self._n = n

    def xyz(self, image):
        """The resident XYZ map (rows, cols, 3) of image `image`, after either kind of upload."""
        out = np.empty(self._shape, np.float32)
        capi.check(self._lib.avt_bgsub_xyz_download(self._h, C.c_int(image), capi.ptr(out, C.c_float)))
        return out

    def run_resident(self):
        capi.check(self._lib.avt_bgsub_run_resident(self._h, C.c_float(self.nnDistThreshRel), C.c_float(self.neighbThreshRel)))

    def sync(self):
        capi.check(self._lib.avt_bgsub_sync(self._h))

    def download(self, image, with_depth=True) -> Result:
        mask = np.empty(self._shape[:2], np.uint8)
        depth = np.empty(self._shape[:2], np.float32) if with_depth else None
        fr = Frame()
        capi.check(self._lib.avt_bgsub_download(self._h, C.c_int(image), capi.ptr(mask, C.c_ubyte),
                                                capi.ptr(depth, C.c_float), C.byref(fr)))
        return Result(mask, depth, fr)

    def info(self, image) -> Result:
        """The record of image `image` alone (box, capped, fg_count, comps): no image is copied."""
        fr = Frame()
        capi.check(self._lib.avt_bgsub_download(self._h, C.c_int(image), None, None, C.byref(fr)))
        return Result(None, None, fr)

    def run_batch(self, images, bg_index=None, prev_boxes=None):
        """upload + run_resident + download of every image: a list of Result."""
        self.upload(images, bg_index, prev_boxes)
        self.run_resident()
        return [self.download(i) for i in range(self._n)]
