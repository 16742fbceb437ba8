"""ctypes binding of tests/cpp/avatar_renderer_restatement.cpp: the reference's AvatarRenderer (AvatarRenderer.cpp:11-224) restated
on the CPU, compiled on first use with g++ -ffp-contract=off into a temporary directory.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "avatar_renderer_restatement.cpp")
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tempfile.mkdtemp(prefix="avatar_render_rst"), "librender_rst.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC])
        _lib = C.CDLL(so)
    return _lib


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def render(cloud, mesh, intrin, width, height, vertex_part=None, joints=None, stable=True):
    """dict of every output of AvatarRenderer for posed vertices `cloud` (V, 3): depth (H, W) float32, mask / lambert uint8,
    faces int32, points (V, 2) / joints (J, 2) float32, keys (F,) float32 and ordered (F, 3) int32 (getOrderedFaces),
    vnormal (V, 3) and lambert_v (V,) of renderLambert.  stable=True orders equal keys by face id (the GPU's order)."""
    cloud = np.ascontiguousarray(cloud, np.float64).reshape(-1, 3)
    mesh = np.ascontiguousarray(mesh, np.int32).reshape(-1, 3)
    V, F = cloud.shape[0], mesh.shape[0]
    vp = np.ascontiguousarray(np.zeros(V, np.int32) if vertex_part is None else vertex_part, np.int32)
    jt = None if joints is None else np.ascontiguousarray(joints, np.float64).reshape(-1, 3)
    J = 0 if jt is None else jt.shape[0]
    out = dict(depth=np.empty((height, width), np.float32), mask=np.empty((height, width), np.uint8),
               lambert=np.empty((height, width), np.uint8), faces=np.empty((height, width), np.int32),
               points=np.empty((V, 2), np.float32), joints=np.empty((max(J, 1), 2), np.float32), keys=np.empty(F, np.float32),
               ordered=np.empty((F, 3), np.int32), vnormal=np.empty((V, 3), np.float64), lambert_v=np.empty(V, np.float32))
    f, d, i, u = C.c_float, C.c_double, C.c_int, C.c_ubyte
    lib().rst_render(i(V), i(F), i(J), _p(cloud, d), _p(jt, d), _p(mesh, i), _p(vp, i), f(intrin["fx"]), f(intrin["fy"]), f(intrin["cx"]),
                     f(intrin["cy"]), i(width), i(height), i(1 if stable else 0), _p(out["depth"], f), _p(out["mask"], u),
                     _p(out["lambert"], u), _p(out["faces"], i), _p(out["points"], f), _p(out["joints"], f), _p(out["keys"], f),
                     _p(out["ordered"], i), _p(out["vnormal"], d), _p(out["lambert_v"], f))
    out["joints"] = out["joints"][:J]
    return out
