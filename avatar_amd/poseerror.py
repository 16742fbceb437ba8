"""The pose error over the C ABI of include/avt_poseerr.h: how far fitted avatars are from the avatars that made the data, as the
field's standard figures in metres: per-vertex error (PVE / V2V), mean per-joint position error (MPJPE), its root-relative form and
the Procrustes-aligned forms (PA-MPJPE, PA-PVE), with per-part sums and maxima.  Both sides of a pair may be read where they lie,
in a context on the device; what comes back is one small table per pair.  The header states the rule.

The scoring runs on the GPU (avatar_amd/csrc/avt_poseerr.hip); there is no CPU fallback: without libavatar_hip.so every call
raises.  `metrics` is host arithmetic on the table.  No threshold on any figure is offered, no per-vertex error comes down, the
alignment always includes the scale, and nothing in the trackers calls this by default."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

POSEERR_SYMBOLS = [
    "avt_poseerr_create", "avt_poseerr_create_for_model", "avt_poseerr_destroy", "avt_poseerr_upload", "avt_poseerr_from_ctx", "avt_poseerr_run",
    "avt_poseerr_get", "avt_poseerr_part_sizes", "avt_poseerr_sync",
]
# AVT_POSEERR_* (include/avt_poseerr.h)
V_SUM, V_SQ, V_MAX, VPA_SUM, VPA_SQ, VPA_SCALE, J_SUM, J_MAX, JR_SUM, JPA_SUM, JPA_SQ, JPA_SCALE = range(12)
COLUMNS = ("V_SUM", "V_SQ", "V_MAX", "VPA_SUM", "VPA_SQ", "VPA_SCALE", "J_SUM", "J_MAX", "JR_SUM", "JPA_SUM", "JPA_SQ", "JPA_SCALE")
ESTIMATE, TRUTH = 0, 1
V_ARGMAX, J_ARGMAX = 0, 1
BAD_INPUT, NO_CONVERGENCE = 1, 2


class PoseError:
    """avt_poseerr: up to max_pairs (estimate, truth) pairs per run of V vertices and J joints (J == 0: no joint figures) with
    `num_parts` parts (1 to 254).  vertex_part: V ints in [0, num_parts), None: one part.  for_model() takes them from a model."""

    def __init__(self, V, J, num_parts=1, vertex_part=None, max_pairs=64, device=0, _model=None, _part_map=None):
        self._lib = capi.load_library()
        self._h = C.c_void_p()
        self.max_pairs, self.device = int(max_pairs), device
        if _model is not None:
            pm = None if _part_map is None else np.ascontiguousarray(_part_map, np.int32).reshape(-1)
            if pm is not None and len(pm) < _model.numJoints():
                raise ValueError("PoseError.for_model: part_map needs one entry per joint")
            capi.check(self._lib.avt_poseerr_create_for_model(C.c_int(device), _model.h, C.c_int(int(num_parts)), capi.ptr(pm, C.c_int), C.c_int(self.max_pairs),
                                                              C.byref(self._h)))
        else:
            vp = None if vertex_part is None else np.ascontiguousarray(vertex_part, np.int32).reshape(-1)
            if vp is not None and len(vp) != int(V):
                raise ValueError(f"PoseError: {len(vp)} vertex_part entries for V = {V}")
            capi.check(self._lib.avt_poseerr_create(C.c_int(device), C.c_int(int(V)), C.c_int(int(J)), C.c_int(int(num_parts)), capi.ptr(vp, C.c_int),
                                                    C.c_int(self.max_pairs), C.byref(self._h)))
        v, j, p = C.c_int(), C.c_int(), C.c_int()
        capi.check(self._lib.avt_poseerr_part_sizes(self._h, None, C.byref(v), C.byref(j), C.byref(p)))
        self.V, self.J, self.numParts = v.value, j.value, p.value
        self.part_sizes = np.empty(self.numParts, np.int32)
        capi.check(self._lib.avt_poseerr_part_sizes(self._h, capi.ptr(self.part_sizes, C.c_int), None, None, None))

    @classmethod
    def for_model(cls, model, num_parts, part_map=None, max_pairs=64, device=0):
        """model: api.AvatarModel; vertex_part[v] = part_map[main joint of v] (None: the joint itself)"""
        return cls(0, 0, num_parts, None, max_pairs, device, _model=model, _part_map=part_map)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.avt_poseerr_destroy(self._h)
            self._h = C.c_void_p()

    def upload(self, side, clouds, joints=None):
        """One side of n pairs from the host: clouds (n, V, 3), joints (n, J, 3) (None only if J == 0), float64."""
        c = np.ascontiguousarray(clouds, np.float64)
        if c.ndim == 2:
            c = c[None]
        if c.ndim != 3 or c.shape[1:] != (self.V, 3):
            raise ValueError(f"PoseError.upload: clouds {c.shape}, not (n, {self.V}, 3)")
        j = None
        if joints is not None and self.J > 0:
            j = np.ascontiguousarray(joints, np.float64)
            if j.ndim == 2:
                j = j[None]
            if j.shape != (c.shape[0], self.J, 3):
                raise ValueError(f"PoseError.upload: joints {j.shape}, not ({c.shape[0]}, {self.J}, 3)")
        capi.check(self._lib.avt_poseerr_upload(self._h, C.c_int(side), C.c_int(c.shape[0]), capi.ptr(c, C.c_double), capi.ptr(j, C.c_double)))

    def from_context(self, side, ctx, frames=None, n=None):
        """One side from api.Context `ctx`'s frames (None: frames 0 .. n - 1), copied on the device; indices may repeat."""
        fr = None if frames is None else np.ascontiguousarray(frames, np.int32).reshape(-1)
        n = len(fr) if fr is not None else int(n)
        capi.check(self._lib.avt_poseerr_from_ctx(self._h, C.c_int(side), ctx.h, C.c_int(n), capi.ptr(fr, C.c_int)))

    def run(self):
        capi.check(self._lib.avt_poseerr_run(self._h))

    def get(self):
        """The last run's result: dict(summary (n, 12) float64 [COLUMNS], per_joint (n, 2, J) [raw, aligned], per_part (n, 2, P)
        [PART_SUM, PART_MAX], argmax (n, 2) int32 [vertex, joint], status (n,) uint32); capi.AvtError "no result" without one."""
        n = C.c_int()
        capi.check(self._lib.avt_poseerr_get(self._h, None, None, None, None, None, C.byref(n)))
        n = n.value
        out = dict(summary=np.empty((n, len(COLUMNS))), per_joint=np.empty((n, 2, self.J)), per_part=np.empty((n, 2, self.numParts)),
                   argmax=np.empty((n, 2), np.int32), status=np.empty(n, np.uint32))
        capi.check(self._lib.avt_poseerr_get(self._h, capi.ptr(out["summary"], C.c_double), capi.ptr(out["per_joint"], C.c_double) if self.J else None,
                                             capi.ptr(out["per_part"], C.c_double), capi.ptr(out["argmax"], C.c_int), capi.ptr(out["status"], C.c_uint), None))
        return out

    def score(self, est_clouds, est_joints, truth_clouds, truth_joints):
        """upload both sides, run, get"""
        self.upload(ESTIMATE, est_clouds, est_joints)
        self.upload(TRUTH, truth_clouds, truth_joints)
        self.run()
        return self.get()

    def sync(self):
        capi.check(self._lib.avt_poseerr_sync(self._h))

    def metrics(self, result=None):
        """metrics() of the given result (None: get()) with this handle's V, J and part sizes"""
        return metrics(self.get() if result is None else result, self.V, self.J, self.part_sizes)


def metrics(result, V, J, part_sizes):
    """The derived figures as ark::PoseErrorResult::derive computes them, one division each (and one root), NaN where the
    denominator is 0: dict(pve, pve_rms, pve_max, pa_pve, pa_pve_scale, mpjpe, mpjpe_max, mpjpe_root, pa_mpjpe, pa_mpjpe_scale),
    each (n,) float64, and pve_part (n, P) (NaN for an empty part).  `result`: what get() returns, or its summary / per_part pair."""
    s = np.asarray(result["summary"], np.float64).reshape(-1, len(COLUMNS))
    psum = np.asarray(result["per_part"], np.float64).reshape(len(s), 2, -1)[:, 0]
    nq = np.asarray(part_sizes, np.float64).reshape(-1)
    Vd, Jd = np.float64(V), np.float64(J)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(pve=s[:, V_SUM] / Vd, pve_rms=np.sqrt(s[:, V_SQ] / Vd), pve_max=s[:, V_MAX].copy(), pa_pve=s[:, VPA_SUM] / Vd,
                    pa_pve_scale=s[:, VPA_SCALE].copy(), mpjpe=s[:, J_SUM] / Jd, mpjpe_max=s[:, J_MAX].copy(), mpjpe_root=s[:, JR_SUM] / Jd,
                    pa_mpjpe=s[:, JPA_SUM] / Jd, pa_mpjpe_scale=s[:, JPA_SCALE].copy(),
                    pve_part=np.where(nq[None] == 0, np.nan, psum / np.where(nq == 0, 1.0, nq)[None]))
