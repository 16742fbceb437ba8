"""Expected visibility flags of the render occlusion (include/avt.h, avt_set_occlusion_render) on the CPU.  TEST INFRASTRUCTURE ONLY.

visible[v] = 1 iff some face f contains v, f passes the back-face test of AvatarOptimizer.cpp:1349-1367 and f's painter position is the
value of at least one pixel of AvatarRenderer::renderFaces.  The face image and the painter order are the restatement's
(tests/avatar_render_restatement.py: `faces`, `ordered`); the back-face test is numpy doubles, multiply and subtract as separate
operations (numpy fuses nothing)."""
from __future__ import annotations

import numpy as np

import avatar_render_restatement as rst


def front_facing(cloud, tri):
    """the back-face test on vertex triples `tri` (n, 3): ((p2 - p1) x (p1 - p3)).z > 1e-4"""
    c = np.asarray(cloud, np.float64).reshape(-1, 3)
    p1, p2, p3 = c[tri[:, 0]], c[tri[:, 1]], c[tri[:, 2]]
    ax, ay = p2[:, 0] - p1[:, 0], p2[:, 1] - p1[:, 1]
    bx, by = p1[:, 0] - p3[:, 0], p1[:, 1] - p3[:, 1]
    m1 = ax * by
    m2 = ay * bx
    return (m1 - m2) > 1e-4


def backface(cloud, mesh):
    """the flags of the back-face test alone (k_visibility)"""
    mesh = np.asarray(mesh, np.int64).reshape(-1, 3)
    vis = np.zeros(len(np.asarray(cloud).reshape(-1, 3)), np.uint8)
    vis[mesh[front_facing(cloud, mesh)].reshape(-1)] = 1
    return vis


def visible(cloud, mesh, intrin, width, height):
    """the flags of the render occlusion for posed vertices `cloud` (V, 3), faces `mesh` (F, 3), a camera dict (fx, fy, cx, cy)"""
    cloud = np.ascontiguousarray(cloud, np.float64).reshape(-1, 3)
    out = rst.render(cloud, mesh, intrin, width, height)
    img = out["faces"]
    seen = np.unique(img[img >= 0])                      # painter positions that own a pixel
    tri = out["ordered"][seen].astype(np.int64)          # their vertex triples, in the mesh's slot order
    vis = np.zeros(len(cloud), np.uint8)
    vis[tri[front_facing(cloud, tri)].reshape(-1)] = 1
    return vis
