"""Hand-made scenes for the render occlusion (include/avt.h, avt_set_occlusion_render), with the flags written out by hand.
TEST INFRASTRUCTURE ONLY: tests/test_occlusion_cpu.py holds tests/occlusion_restatement.py to them, tests/test_gpu_occlusion.py the GPU.

Camera: avatar_render_cases.cam(32, 24) (f = 128, principal point (16, 12)).  A triangle whose vertices go right, then down (clockwise
in the image, whose y points down) is front-facing: ((p2 - p1) x (p1 - p3)).z > 0 in camera space, whose y points up.  A quad is its
corners TL, TR, BR, BL with the faces (TL, TR, BR), (TL, BR, BL); `reversed` swaps the last two of each."""
from __future__ import annotations

import numpy as np

import avatar_render_cases as rc

K32, S32 = rc.cam(32, 24)


def quad(x0, y0, x1, y1, z):
    return [rc.at(K32, x0, y0, z), rc.at(K32, x1, y0, z), rc.at(K32, x1, y1, z), rc.at(K32, x0, y1, z)]


def quad_faces(base, reversed=False):
    b = base
    return [[b, b + 2, b + 1], [b, b + 3, b + 2]] if reversed else [[b, b + 1, b + 2], [b, b + 2, b + 3]]


def _scene(name, verts, mesh, visible, backface, why):
    verts, mesh = np.asarray(verts, np.float64), np.asarray(mesh, np.int32)
    assert len(visible) == len(backface) == len(verts) and mesh.max() < len(verts)
    return dict(name=name, cloud=verts, mesh=mesh, visible=np.asarray(visible, np.uint8), backface=np.asarray(backface, np.uint8), why=why)


def scenes():
    """name -> dict(cloud (V, 3), mesh (F, 3), visible: the flags with the render occlusion on, backface: with the back-face test alone)"""
    far = quad(4, 4, 28, 20, 3.0)
    out = [
        _scene("near-covers-far", far + quad(2, 2, 30, 22, 2.0), quad_faces(0) + quad_faces(4),
               [0, 0, 0, 0, 1, 1, 1, 1], [1] * 8, "two parallel front-facing quads, the near one two pixels larger on every side"),
        _scene("near-covers-half", far + quad(2, 2, 16, 22, 2.0), quad_faces(0) + quad_faces(4),
               [1] * 8, [1] * 8, "the near quad ends at column 16: both faces of the far quad keep pixels right of it"),
        _scene("back-facing-cover", far + quad(2, 2, 30, 22, 2.0), quad_faces(0) + quad_faces(4, reversed=True),
               [0] * 8, [1, 1, 1, 1, 0, 0, 0, 0], "a pixel won by a back-facing face marks nothing and hides what lies behind it"),
        # The reference's row fill floors the first and ceils the last vertex, so every face whose projection has an extent in rows
        # paints some pixel, however small it is; a face that owns no pixel inside the image is one whose projection lies on one row
        # line: y = 21 for all three vertices (the fill returns at ay == cy).  Its depths differ, so it is no sliver in space.
        _scene("no-pixel", rc._tri(K32, [(4, 3), (20, 3), (4, 19)]) + rc._tri(K32, [(16, 21), (10, 21), (4, 21)], [2.0, 3.0, 2.0]),
               [[0, 1, 2], [3, 4, 5]], [1, 1, 1, 0, 0, 0], [1] * 6, "a front-facing face that owns no pixel"),
        # left of the image; wholly behind the camera with a projection right of the image; one vertex on the camera plane (its
        # projection is not finite: the fill paints nothing)
        _scene("outside-behind-on-the-plane", rc._tri(K32, [(4, 3), (14, 3), (4, 13)]) + rc._tri(K32, [(-30, 4), (-7, 10), (-28, 20)])
               + rc._tri(K32, [(40, 4), (70, 10), (42, 20)], -2.0) + rc._tri(K32, [(18, 14), (30, 14)]) + [[0.25, -0.25, 0.0]],
               [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]], [1, 1, 1] + [0] * 9, [1] * 12,
               "front-facing faces outside the image, with z < 0 and with a vertex at z = 0 beside a visible face"),
        _scene("shared-vertex", rc._tri(K32, [(4, 4), (16, 4), (4, 16)], 3.0) + quad(2, 2, 18, 18, 2.0) + rc._tri(K32, [(22, 4), (30, 12)], 3.0),
               [[0, 1, 2]] + quad_faces(3) + [[1, 7, 8]], [0, 1, 0, 1, 1, 1, 1, 1, 1], [1] * 9,
               "vertex 1 belongs to a face hidden behind the quad and to a face seen right of it"),
    ]
    return {s["name"]: s for s in out}


def behind_but_painted():
    """NOT one of the six: a front-facing face with a vertex behind the camera whose mirrored projection owns pixels.  renderFaces
    culls nothing by depth, so by the rule (pixel for pixel that image) its vertices ARE visible."""
    return _scene("behind-but-painted", rc._tri(K32, [(4, 3), (14, 3), (4, 13)]) + rc._tri(K32, [(18, 3), (30, 3)]) + [[0.25, -0.25, -1.0]],
                  [[0, 1, 2], [3, 4, 5]], [1] * 6, [1] * 6, "renderFaces paints a face with a vertex at z < 0: the rule follows the image")
