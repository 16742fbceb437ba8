"""The fit score over the C ABI of include/avt_fitscore.h: the overlay a person looks at in the reference (live-demo.cpp:428-445:
the avatar rendered over the camera image) as integers.  Per image a (P + 1, 7) int64 table: per body part (row P: no part) the
pixels where the rendered avatar and the observed depth AGREE within `tol`, where the model stands IN_FRONT of the surface the
camera saw (free space violated), BEHIND it, where there is MODEL_ONLY or DATA_ONLY, and the absolute depth differences in
micrometres (ABS_UM over all pixels with both, ABS_UM_AGREE over the agreeing ones).  The header states the rule.

The counting runs on the GPU (avatar_amd/csrc/avt_fitscore.hip); there is no CPU fallback: without libavatar_hip.so every call
raises.  `metrics` is host arithmetic on the integers.  DEFAULT_TOL is a choice, not a measurement: 5 cm is about the depth noise
plus the mesh-to-body error one may expect of a consumer depth camera and SMPL, and nobody has measured what a good or a bad
fit scores on real data, so no threshold on any figure is offered either."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

FITSCORE_SYMBOLS = [
    "avt_fitscore_create", "avt_fitscore_destroy", "avt_fitscore_images", "avt_fitscore_rendered", "avt_fitscore_rendered_from_bgsub",
    "avt_fitscore_get", "avt_fitscore_sync",
]
AGREE, IN_FRONT, BEHIND, MODEL_ONLY, DATA_ONLY, ABS_UM, ABS_UM_AGREE = range(7)       # AVT_FITSCORE_* (include/avt_fitscore.h)
COLUMNS = ("AGREE", "IN_FRONT", "BEHIND", "MODEL_ONLY", "DATA_ONLY", "ABS_UM", "ABS_UM_AGREE")
DEFAULT_TOL = 0.05


def _boxes(boxes, n):
    if boxes is None:
        return None
    b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    if len(b) != n:
        raise ValueError(f"FitScorer: {len(b)} boxes for {n} images")
    return b


class FitScorer:
    """avt_fitscore: tables of up to max_images images per call, `num_parts` parts (1 to 254).  Every scoring call returns the
    (n, num_parts + 1, 7) int64 tables of its images and replaces the previous result; a part-mask byte >= num_parts that is not
    255 at a selected pixel fails the call (capi.AvtError naming num_parts), and get() then fails too."""

    def __init__(self, num_parts, max_images=64, device=0):
        self._lib = capi.load_library()
        self._h = C.c_void_p()
        self.numParts, self.max_images, self.device = int(num_parts), int(max_images), device
        capi.check(self._lib.avt_fitscore_create(C.c_int(device), C.c_int(self.numParts), C.c_int(self.max_images), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.avt_fitscore_destroy(self._h)
            self._h = C.c_void_p()

    def score_images(self, model_depth, model_mask, observed, boxes=None, tol=DEFAULT_TOL, stride=1):
        """Host images: model_depth (n, rows, cols) float32 (renderDepth: 0 = no model), model_mask uint8 (renderPartMask: 255 =
        none), observed float32, or one (rows, cols) image of each; boxes (n, 4) tl.x tl.y br.x br.y inclusive (br.x == -1: the
        whole image; None: whole images)."""
        r = np.ascontiguousarray(model_depth, np.float32)
        m = np.ascontiguousarray(model_mask, np.uint8)
        d = np.ascontiguousarray(observed, np.float32)
        if r.ndim == 2:
            r, m, d = r[None], m[None], d[None]
        if r.ndim != 3 or m.shape != r.shape or d.shape != r.shape:
            raise ValueError(f"FitScorer.score_images: shapes {r.shape}, {m.shape}, {d.shape}: three stacks of (n, rows, cols)")
        b = _boxes(boxes, r.shape[0])
        capi.check(self._lib.avt_fitscore_images(self._h, C.c_int(r.shape[0]), C.c_int(r.shape[1]), C.c_int(r.shape[2]), capi.ptr(r, C.c_float),
                                                 capi.ptr(m, C.c_ubyte), capi.ptr(d, C.c_float), capi.ptr(b, C.c_int), C.c_float(tol), C.c_int(stride)))
        return self.get()

    def score_rendered(self, renderer, observed, boxes=None, tol=DEFAULT_TOL, stride=1):
        """The model side is renderer's (render.Renderer) last DEPTH | PART_MASK run, read where it lies; `observed` (n, height,
        width) float32 and `boxes` are host arrays, one per rendered image.  The renderer may run again as soon as this returns."""
        d = np.ascontiguousarray(observed, np.float32)
        if d.ndim == 2:
            d = d[None]
        if d.shape != (renderer.n, renderer.height, renderer.width):
            raise ValueError(f"FitScorer.score_rendered: observed {d.shape} for {renderer.n} rendered images of {renderer.height} x {renderer.width}")
        b = _boxes(boxes, renderer.n)
        capi.check(self._lib.avt_fitscore_rendered(self._h, renderer.h, capi.ptr(d, C.c_float), capi.ptr(b, C.c_int), C.c_float(tol), C.c_int(stride)))
        return self.get()

    def score_rendered_from_bgsub(self, renderer, bg, obs_index=None, tol=DEFAULT_TOL, stride=1):
        """Both sides where they lie: image i of renderer's last run against image obs_index[i] (None: i) of `bg`'s
        (bgsub.BGSubtractor) last run_resident, its masked depth inside the box that run found.  No image is copied."""
        oi = None if obs_index is None else np.ascontiguousarray(obs_index, np.int32).reshape(-1)
        if oi is not None and len(oi) != renderer.n:
            raise ValueError(f"FitScorer.score_rendered_from_bgsub: {len(oi)} indices for {renderer.n} rendered images")
        capi.check(self._lib.avt_fitscore_rendered_from_bgsub(self._h, renderer.h, bg._h, capi.ptr(oi, C.c_int), C.c_float(tol), C.c_int(stride)))
        return self.get()

    def get(self):
        """(n, num_parts + 1, 7) int64 of the last call; capi.AvtError "no score" after a failed or missing one."""
        n = C.c_int()
        capi.check(self._lib.avt_fitscore_get(self._h, None, C.byref(n)))
        out = np.empty((n.value, self.numParts + 1, 7), np.int64)
        capi.check(self._lib.avt_fitscore_get(self._h, capi.ptr(out, C.c_longlong), None))
        return out

    def sync(self):
        capi.check(self._lib.avt_fitscore_sync(self._h))


def _ratio(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.divide(a, b, out=np.full(np.shape(a), np.nan), where=b != 0)


def metrics(table):
    """The derived figures of one (P + 1, 7) table, as ark::FitScore::derive computes them: integer sums first, each converted to
    float64 once, then one division (and for the errors one multiplication by 1e-6); NaN on a zero denominator.  The keys iou,
    agree, violation, unexplained, mean_abs_err, mean_abs_err_agree are floats of the column sums; part_agree, part_violation,
    part_mean_abs_err, part_mean_abs_err_agree are (P + 1,) arrays of the rows (iou and unexplained have no per-part form:
    DATA_ONLY has no part).  A (n, P + 1, 7) stack gives a list."""
    t = np.asarray(table, np.int64)
    if t.ndim == 3:
        return [metrics(x) for x in t]
    if t.ndim != 2 or t.shape[1] != 7 or t.shape[0] < 2:
        raise ValueError("metrics: a (num_parts + 1, 7) table")

    def figures(c):
        both = c[..., AGREE] + c[..., IN_FRONT] + c[..., BEHIND]
        return dict(iou=_ratio(both, both + c[..., MODEL_ONLY] + c[..., DATA_ONLY]), agree=_ratio(c[..., AGREE], both),
                    violation=_ratio(c[..., IN_FRONT] + c[..., MODEL_ONLY], both + c[..., MODEL_ONLY]),
                    unexplained=_ratio(c[..., BEHIND] + c[..., DATA_ONLY], both + c[..., DATA_ONLY]),
                    mean_abs_err=_ratio(c[..., ABS_UM], both) * 1e-6, mean_abs_err_agree=_ratio(c[..., ABS_UM_AGREE], c[..., AGREE]) * 1e-6)

    out = {k: float(v) for k, v in figures(t.sum(0)).items()}
    rows = figures(t)
    for k in ("agree", "violation", "mean_abs_err", "mean_abs_err_agree"):
        out["part_" + k] = rows[k]
    return out
