"""`ark::AvatarRenderer` (AvatarRenderer.h, AvatarRenderer.cpp:11-224) over the C ABI of include/avt_render.h: depth, part mask,
Lambert overlay and face-id images of posed avatars, the projections and the painter order, computed on the GPU
(avatar_amd/csrc/avt_render.hip) with the reference's result pixel for pixel.  There is no CPU fallback.

Renderer is the handle: up to max_images avatars of one model, from host clouds or from the frames of an api.Context after
optimize (no host round trip), rendered by one launch sequence.  AvatarRenderer is the reference's class over it."""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import capi

RENDER_SYMBOLS = [
    "avt_renderer_create", "avt_renderer_destroy", "avt_renderer_set_part_map", "avt_renderer_upload", "avt_renderer_from_ctx",
    "avt_renderer_run", "avt_renderer_download", "avt_renderer_projection", "avt_renderer_vertex_shading", "avt_renderer_sync",
    "avt_renderer_set_ordering",
]
DEPTH, PART_MASK, LAMBERT, FACES = 1, 2, 4, 8          # AVT_RENDER_* (include/avt_render.h)
ALL = DEPTH | PART_MASK | LAMBERT | FACES
ORDER_SORT, ORDER_RANK = 0, 1


def _intrin(intrin):
    """CameraIntrin as a dict (fx, fy, cx, cy) or an object with those attributes"""
    g = (lambda k: intrin[k]) if isinstance(intrin, dict) else (lambda k: getattr(intrin, k))
    return float(g("fx")), float(g("fy")), float(g("cx")), float(g("cy"))


class Renderer:
    """avt_renderer: images of width x height for up to max_images posed avatars of `model` (api.AvatarModel)."""

    def __init__(self, model, width, height, intrin, max_images=1, device=0):
        self._lib = capi.load_library()
        self.model, self.width, self.height, self.max_images = model, int(width), int(height), int(max_images)
        self.V, self.J, self.F = model.numPoints(), model.numJoints(), model.numFaces()
        self.h = C.c_void_p()
        fx, fy, cx, cy = _intrin(intrin)
        capi.check(self._lib.avt_renderer_create(C.c_int(device), model.h, C.c_int(self.width), C.c_int(self.height), C.c_float(fx), C.c_float(fy),
                                                 C.c_float(cx), C.c_float(cy), C.c_int(self.max_images), C.byref(self.h)))
        self.n = 0

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            self._lib.avt_renderer_destroy(self.h)
            self.h = C.c_void_p()

    def set_part_map(self, part_map=None):
        """renderPartMask's part_map (joint -> part); None: the joint id"""
        pm = None if part_map is None or len(part_map) == 0 else np.ascontiguousarray(part_map, np.int32)
        capi.check(self._lib.avt_renderer_set_part_map(self.h, C.c_int(0 if pm is None else len(pm)), capi.ptr(pm, C.c_int)))

    def set_ordering(self, ordering):
        capi.check(self._lib.avt_renderer_set_ordering(self.h, C.c_int(ordering)))

    def upload(self, clouds, joints=None):
        """clouds (n, V, 3) or (V, 3); joints (n, J, 3), (J, 3) or None"""
        c = np.ascontiguousarray(clouds, np.float64).reshape(-1, self.V, 3)
        j = None if joints is None else np.ascontiguousarray(joints, np.float64).reshape(c.shape[0], self.J, 3)
        capi.check(self._lib.avt_renderer_upload(self.h, C.c_int(c.shape[0]), capi.ptr(c, C.c_double), capi.ptr(j, C.c_double)))
        self.n = c.shape[0]

    def from_context(self, ctx, frames=None, n=None):
        """the posed avatars of api.Context `ctx`'s frames (None: frames 0..n-1), copied on the device"""
        fr = None if frames is None else np.ascontiguousarray(frames, np.int32)
        n = len(fr) if fr is not None else int(n)
        capi.check(self._lib.avt_renderer_from_ctx(self.h, ctx.h, C.c_int(n), capi.ptr(fr, C.c_int)))
        self.n = n

    def run(self, what=ALL):
        capi.check(self._lib.avt_renderer_run(self.h, C.c_int(what)))

    def sync(self):
        capi.check(self._lib.avt_renderer_sync(self.h))

    def download(self, image, what=ALL):
        """dict of the selected images of `image`: depth (H, W) float32, mask / lambert uint8, faces int32"""
        H, W = self.height, self.width
        out = {}
        if what & DEPTH: out["depth"] = np.empty((H, W), np.float32)
        if what & PART_MASK: out["mask"] = np.empty((H, W), np.uint8)
        if what & LAMBERT: out["lambert"] = np.empty((H, W), np.uint8)
        if what & FACES: out["faces"] = np.empty((H, W), np.int32)
        capi.check(self._lib.avt_renderer_download(self.h, C.c_int(image), capi.ptr(out.get("depth"), C.c_float), capi.ptr(out.get("mask"), C.c_ubyte),
                                                   capi.ptr(out.get("lambert"), C.c_ubyte), capi.ptr(out.get("faces"), C.c_int)))
        return out

    def projection(self, image, joints=True):
        """dict: points (V, 2), joints (J, 2) float32 (with joints=True), keys (F,) float32 and ordered (F, 3) int32 in painter
        order, pos (F,) the painter position of every face"""
        out = dict(points=np.empty((self.V, 2), np.float32), keys=np.empty(self.F, np.float32), ordered=np.empty((self.F, 3), np.int32),
                   pos=np.empty(self.F, np.int32))
        if joints: out["joints"] = np.empty((self.J, 2), np.float32)
        capi.check(self._lib.avt_renderer_projection(self.h, C.c_int(image), capi.ptr(out["points"], C.c_float), capi.ptr(out.get("joints"), C.c_float),
                                                     capi.ptr(out["keys"], C.c_float), capi.ptr(out["ordered"], C.c_int), capi.ptr(out["pos"], C.c_int)))
        return out


    def vertex_shading(self, image):
        """(vertex normals (V, 3) float64, per-vertex Lambert values (V,) float32) of renderLambert; the last run must include LAMBERT"""
        n, lam = np.empty((self.V, 3)), np.empty(self.V, np.float32)
        capi.check(self._lib.avt_renderer_vertex_shading(self.h, C.c_int(image), capi.ptr(n, C.c_double), capi.ptr(lam, C.c_float)))
        return n, lam


class AvatarRenderer:
    """The reference's class: AvatarRenderer(ava, intrin) over an api.Avatar (cloud (V, 3), jointPos (J, 3)).  Projections and the
    painter order are cached until update(), as in the reference; sizes are (width, height) like cv::Size."""

    def __init__(self, ava, intrin, device=0):
        self.ava, self.intrin, self.device = ava, intrin, device
        self._r = None
        self._fresh = False
        self._cache = None

    def update(self):
        """Forgets the projections, the painter order and the uploaded cloud: the next call works on the avatar as it is now."""
        self._fresh = False
        self._cache = None

    def _empty(self):
        return len(self.ava.cloud) == 0

    def _ensure(self, size):
        W, H = int(size[0]), int(size[1])
        if self._r is None or (self._r.width, self._r.height) != (W, H):
            self._r = Renderer(self.ava.model, W, H, self.intrin, 1, self.device)
            self._fresh = False
        if not self._fresh:
            jp = self.ava.jointPos if len(self.ava.jointPos) else None
            self._r.upload(self.ava.cloud, jp)
            self._fresh = True
        return self._r

    def _projection(self):
        if self._cache is None:
            r = self._ensure((1, 1) if self._r is None else (self._r.width, self._r.height))
            r.run(0)
            self._cache = r.projection(0, joints=len(self.ava.jointPos) > 0)
        return self._cache

    @staticmethod
    def _warn():
        print("WARNING: AvatarRenderer: the avatar has no posed cloud yet (run its update()); nothing rendered", file=sys.stderr)

    def getProjectedPoints(self):
        if self._empty():
            return np.zeros((self.ava.model.numPoints(), 2), np.float32)
        return self._projection()["points"]

    def getProjectedJoints(self):
        if len(self.ava.jointPos) == 0:
            return np.zeros((self.ava.model.numJoints(), 2), np.float32)
        return self._projection()["joints"]

    def getOrderedFaces(self):
        """The painter order: (keys (F,) float32, vertex ids (F, 3) int32), deepest mean vertex depth first, equal keys by face id"""
        if self._empty():
            self._warn()
            return np.zeros(self.ava.model.numFaces(), np.float32), np.ascontiguousarray(self.ava.model.smpl["f"], np.int32).reshape(-1, 3)
        p = self._projection()
        return p["keys"], p["ordered"]

    def _render(self, size, what, part_map=None):
        r = self._ensure(size)
        if what & PART_MASK:
            r.set_part_map(part_map)
        r.run(what)
        return r.download(0, what)

    def renderDepth(self, size):
        if self._empty():
            self._warn()
            return np.zeros((0, 0), np.float32)
        return self._render(size, DEPTH)["depth"]

    def renderLambert(self, size):
        if self._empty():
            self._warn()
            return np.zeros((0, 0), np.uint8)
        return self._render(size, LAMBERT)["lambert"]

    def renderPartMask(self, size, part_map=None):
        if self._empty():
            self._warn()
            return np.zeros((0, 0), np.uint8)
        return self._render(size, PART_MASK, part_map)["mask"]

    def renderFaces(self, size, num_threads=1):
        """face painter positions, -1 = background (num_threads has no counterpart)"""
        if self._empty():
            self._warn()                          # the reference paints nothing: every face projects to (0, 0)
            return np.full((int(size[1]), int(size[0])), -1, np.int32)
        return self._render(size, FACES)["faces"]


def stream_renderer(tracker, n, size, intrin):
    """The renderer a tracker.MultiFrameTracker keeps for its own streams: re-created when the size, the camera or the stream
    count outgrows it."""
    r = getattr(tracker, "_renderer", None)
    W, H = int(size[0]), int(size[1])
    if r is None or (r.width, r.height) != (W, H) or r.max_images < n or _intrin(r._intrin) != _intrin(intrin):
        r = Renderer(tracker.ctx.model, W, H, intrin, max(n, 1), getattr(tracker.ctx, "device", 0))
        r._intrin = intrin
        tracker._renderer = r
    return r


def render_streams(tracker, streams, size, intrin, what=LAMBERT, part_map=None, download=True):
    """The last fit of the given streams of a tracker.MultiFrameTracker rendered on the device in one run: a list of download()
    dicts, or with download=False the renderer itself, its images left on the device for a consumer that reads them there."""
    r = stream_renderer(tracker, len(streams), size, intrin)
    if what & PART_MASK:
        r.set_part_map(part_map)
    r.from_context(tracker.ctx, list(streams))
    r.run(what)
    return [r.download(i, what) for i in range(len(streams))] if download else r
