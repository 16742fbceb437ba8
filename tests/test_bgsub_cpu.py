"""CPU tests of the background subtraction stage (include/avt_bgsub.h): the two restatements of BGSubtractor::run in
tests/bgsub_restatement.py against each other and against hand-computed known answers, the C ABI's symbol set, and
the C++ facade's header.  No GPU needed."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import bgsub_restatement as R
from avatar_amd import bgsub, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PREV = ((1, 2), (3, 4))


def _both(bg, im, nn_rel=0.005, neighb_rel=0.005, prev_box=PREV):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # inf - inf, NaN arithmetic: the reference's float semantics
        a = R.literal(bg, im, nn_rel, neighb_rel, prev_box)
        b = R.fast(bg, im, nn_rel, neighb_rel, prev_box)
    assert R.same(a, b)
    return a


def _flat(rows, cols, v, bgv=(0, 0, 0)):
    im = np.empty((rows, cols, 3), F)
    im[:] = v
    bg = np.empty((rows, cols, 3), F)
    bg[:] = bgv
    return bg, im


def _random_scene(seed):
    """blocky XYZ maps (components of a few levels), noise, sensor holes, NaN / inf coordinates, a background that
    lies near the image on part of the frame and has holes of its own; thresholds scaled to the image size"""
    rng = np.random.default_rng(seed)
    rows, cols = (int(v) for v in rng.integers(8, 41, 2))
    k = int(rng.integers(2, 12))
    levels = rng.choice([1.0, 1.2, 2.0, 3.0], size=((rows + k - 1) // k + 1, (cols + k - 1) // k + 1, 3)).astype(F)
    im = np.repeat(np.repeat(levels, k, 0), k, 1)[:rows, :cols].copy()
    im += rng.normal(0, rng.choice([0, 0.01, 0.05]), im.shape).astype(F)
    bg = np.full_like(im, 10.0)
    near = rng.random((rows, cols)) < rng.choice([0, 0.1, 0.4])
    bg[near] = im[near] + rng.normal(0, 0.05, (int(near.sum()), 3)).astype(F)
    bg[rng.random((rows, cols)) < 0.1, 2] = 0
    im[rng.random((rows, cols)) < rng.choice([0, 0.03, 0.15]), 2] = 0
    sp = rng.random((rows, cols))
    im[sp < 0.01] = np.nan
    im[(sp > 0.01) & (sp < 0.015), 0] = np.inf
    im[(sp > 0.015) & (sp < 0.02), 2] = -np.inf
    n = rows * cols
    nn, nb = rng.choice([0.001, 0.01, 0.1]), rng.choice([0.001, 0.05, 0.5, 2.0])
    return bg, im, nn * n / 1.2e6, nb * n / 1.2e6


def grid_scene(first_small=True, speck=True):
    """176 x 176: 16 x 16 blocks of 10 x 10 pixels between zero-depth lines, each block its own component (> 254 of
    them); block 0 cut to 5 x 5 (too small), a one-pixel speck in the last gap column, past the cap"""
    im = np.zeros((176, 176, 3), F)
    for bi in range(16):
        for bj in range(16):
            im[11 * bi:11 * bi + 10, 11 * bj:11 * bj + 10] = (0.1 * bj, 0.1 * bi, 1.0 + 0.5 * ((bi + bj) % 2))
    if first_small:
        im[0:10, 5:10, 2] = 0
        im[5:10, 0:5, 2] = 0
    if speck:
        im[170, 175] = (5, 5, 5)
    return np.full_like(im, 0.0), im


@pytest.mark.parametrize("seed", range(300))
def test_literal_and_fast_restatements_agree(seed):
    _both(*_random_scene(seed))


def test_restatements_agree_past_the_cap():
    bg, im = grid_scene()
    a = _both(bg, im)
    assert a["capped"] and a["top_left"] == PREV[0] and a["bot_right"] == PREV[1]
    assert a["comps"] == [(100, i) for i in range(254)]               # id order, unsorted (:124 returns before :153)
    m = a["mask"]
    assert (m[0:10, 0:10][im[0:10, 0:10, 2] != 0] == 255).all()     # the small block before the cap: 255
    assert m[0, 11] == 0 and m[165, 11 * 14] == 253                   # the 254th kept component caps the run ...
    assert (m[165:175, 165:175] == 254).all() and m[170, 175] == 254  # ... later components, the small speck too, stay 254
    assert (m[im[:, :, 2] == 0] == 255).all()
    # exactly 254 kept components cap as well: nothing is left unvisited then but the speck
    bg, im = grid_scene(first_small=False, speck=True)
    im[165:175, 154:175, 2] = 0
    b = _both(bg, im)
    assert b["capped"] and len(b["comps"]) == 254 and b["mask"][170, 175] == 254 and (b["mask"] == 254).sum() == 1


def test_threshold_rounding():
    """double arithmetic on the int pixel count, then rounded to float (:160-161): 12 x 12 at 0.002 gives 16.666668f,
    float arithmetic would give 16.666666f; a squared distance of exactly 16.666666f is near the background"""
    assert R.thresholds(12, 12, 0.002, 0.001) == (F(16.666668), F(8.333334))
    assert F(F(1200000.0 / 144) * F(0.002)) == F(16.666666)
    assert R.thresholds(720, 1280, 0.005, 0.005) == (F(0.0065104165), F(0.0065104165))
    assert R.thresholds(720, 1280, 0.002, 0.001) == (F(0.0026041667), F(0.0013020834))
    bg, im = _flat(12, 12, (0, 0, 5.082483))
    bg[0, 0] = (0, 0, 1)                          # (5.082483 - 1)^2 = 16.666666f exactly
    bg[11, 11] = (0, 0, 1)                        # a corner: the window is clipped, not wrapped
    bg[5, 11] = (0, 0, 1)                         # the right border
    a = _both(bg, im, 0.002, 0.001)
    dead = np.zeros((12, 12), bool)
    dead[0:2, 0:2] = dead[10:12, 10:12] = dead[4:7, 10:12] = True
    assert (a["mask"][dead] == 255).all() and (a["mask"][~dead] == 0).all()
    assert a["comps"] == [(144 - 14, 0)] and a["top_left"] == (0, 0) and a["bot_right"] == (11, 11) and a["fg_count"] == 130
    assert (a["masked_depth"][dead] == 0).all() and (a["masked_depth"][~dead] == F(5.082483)).all()


def test_zero_depth_background_neighbour_is_skipped():
    for bgz, expect in ((0.0, 0), (-0.0, 0), (1e-30, 255)):
        bg, im = _flat(12, 12, (3, 0, 0.001), (3, 0, bgz))
        a = _both(bg, im, 0.002, 0.001)
        assert (a["mask"] == expect).all(), bgz
    bg, im = _flat(12, 12, (3, 0, 0.001))
    im[4, 7, 2] = 0                               # a sensor hole is 255 and splits nothing here
    a = _both(bg, im, 0.002, 0.001)
    assert a["mask"][4, 7] == 255 and (a["mask"] != 255).sum() == 143 and a["comps"] == [(143, 0)]


def test_nan_joins_and_inf_does_not():
    bg, im = _flat(12, 12, (0, 0, 1))
    im[:, 6:] = (0, 0, 9)                         # two halves of 72 pixels, 64 apart: both too small
    a = _both(bg, im, 0.002, 0.001)
    assert (a["mask"] == 255).all() and a["comps"] == [] and a["top_left"] == (11, 11) and a["bot_right"] == (0, 0)
    im[0, 5] = (np.nan, 0, 1)                     # NaN compares false: !(norm > t) joins both halves
    a = _both(bg, im, 0.002, 0.001)
    assert (a["mask"] == 0).all() and a["comps"] == [(144, 0)]
    im[0, 5] = (np.inf, 0, 1)                     # inf - 0 = inf: never joins
    a = _both(bg, im, 0.002, 0.001)
    assert (a["mask"] == 255).all()


def test_min_pts_boundary_and_empty_frames():
    bg, im = _flat(12, 12, (0, 0, 0))
    im[1:11, 1:11] = (0, 0, 1)                    # exactly min_pts = 100 pixels: kept
    a = _both(bg, im)
    assert R.min_points(12, 12) == 100 and R.min_points(720, 1280) == 921 and R.min_points(480, 640) == 307
    assert (a["mask"][1:11, 1:11] == 0).all() and a["comps"] == [(100, 0)] and a["fg_count"] == 100
    assert a["top_left"] == (1, 1) and a["bot_right"] == (10, 10)
    im[5, 5, 2] = 0                               # 99: dropped, the frame is empty
    a = _both(bg, im)
    assert (a["mask"] == 255).all() and a["comps"] == [] and a["top_left"] == (11, 11) and a["bot_right"] == (0, 0) and a["fg_count"] == 0
    assert np.array_equal(a["masked_depth"], im[:, :, 2])
    for v in ((0, 0, 0), (0, 0, 1)):              # 3 x 4: never min_pts pixels
        a = _both(*_flat(3, 4, v))
        assert (a["mask"] == 255).all() and a["top_left"] == (3, 2) and a["bot_right"] == (0, 0)


def test_ids_follow_the_first_pixel_and_ties_sort_by_id():
    bg, im = _flat(20, 20, (0, 0, 9))
    im[1:10, 0:15] = (0, 0, 1)                    # 135 pixels from (1, 0); the rest, mostly below, reaches row 0: id 0
    a = _both(bg, im, 0.005, 0.001)
    assert a["mask"][1, 0] == 1 and a["mask"][0, 0] == 0 and a["mask"][19, 0] == 0
    assert a["comps"] == [(265, 0), (135, 1)]
    im[0:10] = (0, 0, 1)                          # 200 / 200: equal sizes sort by id, descending
    a = _both(bg, im, 0.005, 0.001)
    assert a["comps"] == [(200, 1), (200, 0)]


def test_abi_exports_every_symbol_of_avt_bgsub_h():
    hdr = open(os.path.join(ROOT, "include", "avt_bgsub.h")).read()
    declared = set(re.findall(r"\b(avt_bgsub_[a-z_]+)\s*\(", hdr))
    assert declared == set(bgsub.BGSUB_SYMBOLS), declared ^ set(bgsub.BGSUB_SYMBOLS)
    lib = capi.load_library()
    for s in declared:
        assert hasattr(lib, s), s


def test_frame_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "avt_bgsub.h")).read()
    assert "#define AVT_BGSUB_MAX_COMPS 254" in hdr and bgsub.MAX_COMPS == 254
    import ctypes
    assert ctypes.sizeof(bgsub.Frame) == 4 * (4 + 3 + 2 * 254)


def test_facade_header_compiles(tmp_path):
    src = tmp_path / "inc.cpp"
    src.write_text('#include "ark/BGSubtractor.h"\n'
                   'int main() { ark::ImageXYZ bg(4, 5); ark::BGSubtractor s(bg); return (int)(s.nnDistThreshRel * 0) + s.topLeft.x; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])
