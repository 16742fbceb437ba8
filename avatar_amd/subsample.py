"""The trackers' interval subsampling (demo.cpp:216-250) on the device, over the C ABI of include/avt_subsample.h: the labels
behind a forest handle and the XYZ maps behind a background subtractor go straight into a context's frame slots; a table of
counts, the centroids that were asked for and the boxes come back.  api.Context.frames_subsample / frames_commit are the
callers; the rule is in the header.  There is no CPU path here: tracker.subsample is the host's own statement of the rule."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

SUBSAMPLE_SYMBOLS = ["avt_frames_subsample_constants", "avt_frames_subsample_rtree", "avt_frames_subsample_rforest", "avt_frames_subsample_commit"]


def constants():
    """(chunk, scan_width): grid pixels per workgroup of the counting and writing kernels, chunk counts per pass of the scan."""
    c, w = C.c_int(), C.c_int()
    capi.check(capi.load_library().avt_frames_subsample_constants(C.byref(c), C.byref(w)))
    return c.value, w.value


def frames_subsample(ctx, bgsub, forest, intervals, boxes=None, centroid_of=None):
    """Image i of the batch behind `forest` (rtree.RTree or rforest.RForest) and `bgsub` into frame slot i of `ctx`, every
    intervals[i]-th pixel of its box (an int serves all images).  boxes None: the boxes bgsub's last run_resident left on the
    device (the labels must be that run's); else (n, 4) tl.x tl.y br.x br.y, inclusive, br.x == -1 the whole image.
    centroid_of: the images whose centroid is wanted (indices or an (n,) bool array), None: none.
    Returns (counts (n, 1 + num_parts) int32, centroid (n, 3) float64 with NaN rows where none was asked for or the frame is
    empty, boxes (n, 4) int32 as used).  The frames are pending until frames_commit."""
    n = int(forest._shape[0])
    iv = np.ascontiguousarray(np.broadcast_to(np.asarray(intervals, np.int32), (n,)))
    b = None if boxes is None else np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    if b is not None and len(b) != n:
        raise ValueError(f"frames_subsample: {len(b)} boxes for {n} labelled images")
    want = None
    if centroid_of is not None:
        sel = np.asarray(centroid_of)
        want = np.zeros(n, np.uint8)
        if sel.dtype == bool:
            if sel.shape != (n,):
                raise ValueError(f"frames_subsample: centroid_of has {sel.shape} flags for {n} images")
            want[sel] = 1
        elif sel.size:
            want[sel.astype(np.int64)] = 1
    counts = np.zeros((n, 1 + ctx.num_parts), np.int32)
    centroid = np.full((n, 3), np.nan)
    used = np.zeros((n, 4), np.int32)
    entry = getattr(capi.load_library(), "avt_frames_subsample_" + forest._PREFIX[4:])
    capi.check(entry(ctx.h, forest._h, bgsub._h, capi.ptr(b, C.c_int), capi.ptr(iv, C.c_int), capi.ptr(want, C.c_ubyte),
                     capi.ptr(counts, C.c_int), capi.ptr(centroid, C.c_double), capi.ptr(used, C.c_int)))
    return counts, centroid, used


def frames_commit(ctx, keep=None):
    """The pending frames become resident; keep (n,) bool: a frame that is not kept is resident with 0 points (None: all)."""
    k = None if keep is None else np.ascontiguousarray(np.asarray(keep, bool), np.uint8)
    capi.check(capi.load_library().avt_frames_subsample_commit(ctx.h, capi.ptr(k, C.c_ubyte)))
