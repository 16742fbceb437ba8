"""Plain restatements of what the kernels at the head of an ICP iteration compute (avatar_amd/csrc/avt_kernels.hip), in numpy alone: the
yardstick of tests/test_gpu_head_edges.py.  A helper module of the tests, not a test file.  (Nearest neighbours: tests/nn_restatement.py.)

  update(model, w, p, R)        Avatar::update (Avatar.cpp:22-75) in numpy.longdouble: shaped cloud, regressed joints, forward kinematics
                                down the tree, t_j = o_j - R_j * jointPos_j, blend.  Returns cloud (V, 3), joint positions (J, 3) and the
                                column-major 3 x 4 joint transforms (J, 12), as long doubles.
  update_q(model, p, q, w)      the same from quaternions (x, y, z, w): Eigen's Quaternion::toRotationMatrix, no normalisation.
  visibility(mesh, cloud, en)   back-face test (AvatarOptimizer.cpp:1349-1367) in float64, (ax * by) - (ay * bx) > 1e-4 with the products
                                and the difference rounded separately (numpy does not fuse them; the kernels use __dmul_rn / __dsub_rn).
  finalise(corr, V)             (cnt = matches per vertex, M = vertices matched, T = matches) of a correspondence array.

tests/test_head_edges_cpu.py ties update, update_q and visibility to the CPU oracle on every model of tests/head_models.py."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

L = np.longdouble


def _weights(model):
    W = model["weights"]
    return np.asarray(W.toarray() if sp.issparse(W) else W, np.float64)


def _parents(model):
    p = np.asarray(model["kintree_table"])[0].astype(np.int64).copy()
    p[0] = -1
    return p


def update(model, w, p, R):
    J = np.asarray(model["kintree_table"]).shape[1]
    return _update(model, w, p, np.asarray(R, np.float64).reshape(J, 3, 3).astype(L))


def _update(model, w, p, R):
    """R: (J, 3, 3) long doubles."""
    vt = np.asarray(model["v_template"], np.float64).astype(L)
    sd = np.asarray(model["shapedirs"], np.float64).astype(L)
    Jr = np.asarray(model["J_regressor"], np.float64)
    parent = _parents(model)
    J = len(parent)
    w = np.asarray(w, np.float64).astype(L); p = np.asarray(p, np.float64).astype(L)
    shaped = vt + sd @ w                                             # (V, 3)
    jp = np.zeros((J, 3), L)
    for j in range(J):                                               # the regressor's stored entries only
        nz = np.nonzero(Jr[j])[0]
        r = Jr[j, nz].astype(L)
        jp[j] = r @ vt[nz] + np.einsum("v,vck->ck", r, sd[nz]) @ w
    Rw = np.zeros((J, 3, 3), L); o = np.zeros((J, 3), L)
    Rw[0], o[0] = R[0], p
    for j in range(1, J):
        pa = parent[j]
        Rw[j] = Rw[pa] @ R[j]
        o[j] = o[pa] + Rw[pa] @ (jp[j] - jp[pa])
    T = np.zeros((J, 12), L)
    for j in range(J):
        T[j, :9] = Rw[j].T.reshape(9)                                # column-major
        T[j, 9:] = o[j] - Rw[j] @ jp[j]
    PT = _weights(model).astype(L) @ T                               # (V, 12)
    cloud = PT[:, 0:3] * shaped[:, 0:1] + PT[:, 3:6] * shaped[:, 1:2] + PT[:, 6:9] * shaped[:, 2:3] + PT[:, 9:12]
    return cloud, o, T


def quat_to_rot(q):
    q = np.asarray(q, np.float64).reshape(-1, 4).astype(L)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    out = np.empty((len(q), 3, 3), L)
    out[:, 0, 0] = 1 - (tyy + tzz); out[:, 0, 1] = txy - twz; out[:, 0, 2] = txz + twy
    out[:, 1, 0] = txy + twz; out[:, 1, 1] = 1 - (txx + tzz); out[:, 1, 2] = tyz - twx
    out[:, 2, 0] = txz - twy; out[:, 2, 1] = tyz + twx; out[:, 2, 2] = 1 - (txx + tyy)
    return out


def update_q(model, p, q, w):
    return _update(model, w, p, quat_to_rot(q))      # (the rotation matrices stay long doubles)


def visibility(mesh, cloud, enable=True):
    cloud = np.asarray(cloud, np.float64)
    V = len(cloud)
    if not enable:
        return np.ones(V, np.uint8)
    vis = np.zeros(V, np.uint8)
    mesh = np.asarray(mesh).astype(np.int64).reshape(-1, 3)
    if len(mesh) == 0:
        return vis
    p1, p2, p3 = cloud[mesh[:, 0]], cloud[mesh[:, 1]], cloud[mesh[:, 2]]
    ax = p2[:, 0] - p1[:, 0]; ay = p2[:, 1] - p1[:, 1]
    bx = p1[:, 0] - p3[:, 0]; by = p1[:, 1] - p3[:, 1]
    m1 = ax * by
    m2 = ay * bx
    z = m1 - m2
    vis[mesh[z > 1e-4].reshape(-1)] = 1
    return vis


def finalise(corr, V):
    corr = np.asarray(corr)
    cnt = np.bincount(corr[corr >= 0], minlength=V).astype(np.int32)
    return cnt, int((cnt > 0).sum()), int(cnt.sum())
