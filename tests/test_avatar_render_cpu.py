"""CPU: the restatement of the reference's AvatarRenderer (tests/cpp/avatar_renderer_restatement.cpp) on hand-built meshes with
known answers, the symbol set of include/avt_render.h and compile checks of the new headers."""
import ctypes
import os
import re
import subprocess

import numpy as np

import avatar_render_restatement as rst

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INTR = dict(fx=100.0, fy=100.0, cx=10.0, cy=40.0)
MAIN, BACK = np.array([0.8, 1.5, -1.2]), np.array([-0.2, -1.5, 0.4])


def _lambert(p, n):
    """AvatarRenderer.cpp:146-164 for one vertex: float(main . n * 0.8 + back . n * 0.2) * 255, at least 0"""
    m = (MAIN - p) / np.sqrt(((MAIN - p) ** 2).sum())
    b = (BACK - p) / np.sqrt(((BACK - p) ** 2).sum())
    return max(np.float32(m @ n * 0.8 + b @ n * 0.2) * np.float32(255), np.float32(0))


def test_one_triangle_facing_the_camera():
    # projections land on whole pixels: (10, 40), (35, 40), (10, 15)
    cl = np.array([[0, 0, 2.0], [0.5, 0, 2.0], [0, 0.5, 2.0]])
    o = rst.render(cl, [[0, 1, 2]], INTR, 40, 48)
    assert np.array_equal(o["points"], np.array([[10, 40], [35, 40], [10, 15]], np.float32))
    assert np.array_equal(o["keys"], np.float32([2.0])) and np.array_equal(o["ordered"], [[0, 1, 2]])
    n = np.array([0.0, 0.0, -1.0])                         # (b - a) x (c - a) = +z, turned to face the camera
    assert np.array_equal(o["vnormal"], np.tile(n, (3, 1)))
    lv = [_lambert(p, n) for p in cl]
    assert np.array_equal(o["lambert_v"], np.float32(lv))
    # at a vertex pixel the barycentric value is that vertex's value, truncated
    assert o["lambert"][15, 10] == int(lv[2]) and o["lambert"][40, 10] == int(lv[0])
    assert o["depth"][30, 15] == np.float32(2.0)
    # faces: the end-exclusive fill paints position 0 inside, -1 elsewhere; the Lambert fill includes the last column
    assert o["faces"][30, 12] == 0 and o["faces"][5, 5] == -1 and o["faces"].max() == 0
    lit, painted = o["lambert"] > 0, o["faces"] >= 0
    assert lit.sum() > painted.sum() and not (painted & ~lit).any()


def test_two_overlapping_faces_nearer_wins():
    far = [[0, 0, 3.0], [0.9, 0, 3.0], [0, 0.9, 3.0]]           # projects to a larger triangle behind
    near = [[0, 0, 2.0], [0.3, 0, 2.0], [0, 0.3, 2.0]]
    cl = np.array(far + near)
    o = rst.render(cl, [[3, 4, 5], [0, 1, 2]], INTR, 48, 48)
    assert np.array_equal(o["ordered"], [[0, 1, 2], [3, 4, 5]])   # decreasing depth: far first
    assert o["faces"][35, 12] == 1 and o["faces"][15, 12] == 0
    assert abs(o["depth"][35, 12] - 2.0) < 1e-5 and abs(o["depth"][15, 12] - 3.0) < 1e-5


def test_shared_vertex_quad_averages_normals():
    cl = np.array([[0, 0, 2.0], [0.4, 0, 2.0], [0, 0.4, 2.0], [0.4, 0.4, 2.3]])
    mesh = [[0, 1, 2], [1, 3, 2]]
    o = rst.render(cl, mesh, INTR, 64, 64)

    def fn(a, b, c):
        n = np.cross(cl[b] - cl[a], cl[c] - cl[a])
        return n / np.sqrt((n ** 2).sum())
    n0, n1 = fn(0, 1, 2), fn(1, 3, 2)
    for v, ns in ((0, [n0]), (1, [n0, n1]), (2, [n0, n1]), (3, [n1])):
        s = sum(ns)
        s = s / np.sqrt((s ** 2).sum())
        s = -s if s[2] > 0 else s
        assert np.allclose(o["vnormal"][v], s, rtol=0, atol=1e-15), v
    assert not np.allclose(o["vnormal"][1], o["vnormal"][0])      # the shared vertices carry the average
    assert (o["lambert"] > 0).sum() > 100


def test_face_almost_edge_on_is_not_lit():
    # a face beside the optical axis, almost parallel to the viewing direction: |n_z| = 0.005 of a unit normal is under
    # renderLambert's 1e-2 rule (and edge-on for renderDepth's 0.1), yet its projection has an area
    u = 0.005 / np.sqrt(1 - 0.005 ** 2)
    cl = np.array([[1.0, 0, 2.0], [1.0, 0.5, 2.0], [1.0 + u, 0, 3.0]])
    n = np.cross(cl[1] - cl[0], cl[2] - cl[0]); n = n / np.sqrt((n ** 2).sum())
    assert abs(abs(n[2]) - 0.005) < 1e-12
    o = rst.render(cl, [[0, 1, 2]], INTR, 70, 48)
    assert (o["faces"] >= 0).sum() > 50                           # renderFaces paints every face
    assert (o["lambert"] == 0).all() and (o["depth"] == 0).all()


def test_coincident_faces_with_opposite_winding_give_zero():
    cl = np.array([[0, 0, 2.0], [0.5, 0, 2.0], [0, 0.5, 2.0], [0.6, 0, 2.0], [0.9, 0, 2.0], [0.9, 0.3, 2.0]])
    mesh = [[0, 1, 2], [0, 2, 1], [3, 4, 5]]
    o = rst.render(cl, mesh, INTR, 64, 48)
    assert np.isnan(o["vnormal"][:3]).all() and np.isnan(o["lambert_v"][:3]).all()   # the sums are 0: divided by a zero norm
    assert (o["faces"][25:39, 11:20] >= 0).all()                  # both faces are visible and painted ...
    assert (o["lambert"][:, :37] == 0).all()                      # ... NaN gives pixel 0
    assert (o["lambert"][:, 38:] > 0).sum() > 20                  # the third face is lit


def test_face_crossing_the_image_border():
    cl = np.array([[-0.3, 0, 2.0], [0.5, 0.1, 2.2], [0.1, 0.9, 2.1]])
    o = rst.render(cl, [[0, 1, 2]], INTR, 30, 40)
    assert o["points"][0, 0] < 0 and o["points"][1, 0] > 29 and o["points"][2, 1] < 0
    f, g = o["faces"] >= 0, o["lambert"] > 0
    assert f[:, 0].any() and g[:, 0].any() and g[:, -1].any() and g[0, :].any()
    # the same triangle in a wider, taller image: the border image is its crop (up to the clamped last column)
    big = rst.render(cl, [[0, 1, 2]], INTR, 90, 60)
    for k in ("lambert", "depth", "faces", "mask"):
        assert np.array_equal(big[k][:40, :29], o[k][:, :29]), k


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "avt_render.h")).read()
    return set(re.findall(r"\b(avt_renderer_\w+)\s*\(", src))


def test_symbol_set_of_avt_render_h():
    from avatar_amd import render
    declared = _header_symbols()
    assert declared == set(render.RENDER_SYMBOLS), declared ^ set(render.RENDER_SYMBOLS)
    lib = ctypes.CDLL(os.path.join(ROOT, "avatar_amd", "csrc", "libavatar_hip.so"))
    for s in declared:
        getattr(lib, s)


def test_headers_compile(tmp_path):
    inc = os.path.join(ROOT, "include")
    for lang, std, hdr in (("c", "-std=c11", "avt_render.h"), ("c++", "-std=c++17", "avt_render.h"), ("c++", "-std=c++17", "ark/AvatarRenderer.h"),
                           ("c++", "-std=c++17", "ark/MultiFrameTracker.h")):
        src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
        src.write_text(f'#include "{hdr}"\n')
        subprocess.check_call(["gcc" if lang == "c" else "g++", std, "-fsyntax-only", "-Wall", "-Werror", "-I", inc, str(src)])
