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
import bgsub_scenes as S
from bgsub_scenes import _random_scene
from avatar_amd import bgsub, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PREV = S.PREV


def _both(bg, im, nn_rel=0.005, neighb_rel=0.005, prev_box=PREV):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # inf - inf, NaN arithmetic: the reference's float semantics
        a = R.literal(bg, im, nn_rel, neighb_rel, prev_box)
        b = R.fast(bg, im, nn_rel, neighb_rel, prev_box)
    assert R.same(a, b)
    return a


@pytest.mark.parametrize("seed", range(300))
def test_literal_and_fast_restatements_agree(seed):
    _both(*_random_scene(seed))


def test_restatements_agree_past_the_cap():
    bg, im, _, _, _ = S.cap_scene()
    a = _both(bg, im)
    assert a["capped"] and a["top_left"] == PREV[0] and a["bot_right"] == PREV[1]
    assert a["comps"] == [(100, i) for i in range(254)]               # id order, unsorted (:124 returns before :153)
    m = a["mask"]
    assert (m[0:10, 0:10][im[0:10, 0:10, 2] != 0] == 255).all()     # the small block before the cap: 255
    assert m[0, 11] == 0 and m[165, 11 * 14] == 253                   # the 254th kept component caps the run ...
    assert (m[165:175, 165:175] == 254).all() and m[170, 175] == 254  # ... later components, the small speck too, stay 254
    assert (m[im[:, :, 2] == 0] == 255).all()
    # exactly 254 kept components cap as well: nothing is left unvisited then but the speck
    bg, im, _, _, _ = S.cap_scene(exact=True)
    b = _both(bg, im)
    assert b["capped"] and len(b["comps"]) == 254 and b["mask"][170, 175] == 254 and (b["mask"] == 254).sum() == 1


def test_threshold_rounding():
    """double arithmetic on the int pixel count, then rounded to float (:160-161): 12 x 12 at 0.002 gives 16.666668f,
    float arithmetic would give 16.666666f; a squared distance of exactly 16.666666f is near the background"""
    assert R.thresholds(12, 12, 0.002, 0.001) == (F(16.666668), F(8.333334))
    assert F(F(1200000.0 / 144) * F(0.002)) == F(16.666666)
    assert R.thresholds(720, 1280, 0.005, 0.005) == (F(0.0065104165), F(0.0065104165))
    assert R.thresholds(720, 1280, 0.002, 0.001) == (F(0.0026041667), F(0.0013020834))
    bg, im, nn, nb, _ = S.tie_scene()             # (5.082483 - 1)^2 = 16.666666f at a corner, the right border, inside
    a = _both(bg, im, nn, nb)
    dead = np.zeros((12, 12), bool)
    dead[0:2, 0:2] = dead[10:12, 10:12] = dead[4:7, 10:12] = True
    assert (a["mask"][dead] == 255).all() and (a["mask"][~dead] == 0).all()
    assert a["comps"] == [(144 - 14, 0)] and a["top_left"] == (0, 0) and a["bot_right"] == (11, 11) and a["fg_count"] == 130
    assert (a["masked_depth"][dead] == 0).all() and (a["masked_depth"][~dead] == F(5.082483)).all()


def test_zero_depth_background_neighbour_is_skipped():
    for bgz, expect in ((0.0, 0), (-0.0, 0), (1e-30, 255)):
        bg, im, nn, nb, _ = S.zero_bg_scene(bgz)
        a = _both(bg, im, nn, nb)
        assert (a["mask"] == expect).all(), bgz
    bg, im, nn, nb, _ = S.hole_scene()            # a sensor hole is 255 and splits nothing here
    a = _both(bg, im, nn, nb)
    assert a["mask"][4, 7] == 255 and (a["mask"] != 255).sum() == 143 and a["comps"] == [(143, 0)]


def test_nan_joins_and_inf_does_not():
    bg, im, nn, nb, _ = S.nan_inf_scene()         # two halves of 72 pixels, 64 apart: both too small
    a = _both(bg, im, nn, nb)
    assert (a["mask"] == 255).all() and a["comps"] == [] and a["top_left"] == (11, 11) and a["bot_right"] == (0, 0)
    bg, im, nn, nb, _ = S.nan_inf_scene("nan")    # NaN compares false: !(norm > t) joins both halves
    a = _both(bg, im, nn, nb)
    assert (a["mask"] == 0).all() and a["comps"] == [(144, 0)]
    bg, im, nn, nb, _ = S.nan_inf_scene("inf")    # inf - 0 = inf: never joins
    a = _both(bg, im, nn, nb)
    assert (a["mask"] == 255).all()


def test_min_pts_boundary_and_empty_frames():
    bg, im, _, _, _ = S.min_pts_scene()           # exactly min_pts = 100 pixels: kept
    a = _both(bg, im)
    assert R.min_points(12, 12) == 100 and R.min_points(720, 1280) == 921 and R.min_points(480, 640) == 307
    assert (a["mask"][1:11, 1:11] == 0).all() and a["comps"] == [(100, 0)] and a["fg_count"] == 100
    assert a["top_left"] == (1, 1) and a["bot_right"] == (10, 10)
    bg, im, _, _, _ = S.min_pts_scene(missing=True)   # 99: dropped, the frame is empty
    a = _both(bg, im)
    assert (a["mask"] == 255).all() and a["comps"] == [] and a["top_left"] == (11, 11) and a["bot_right"] == (0, 0) and a["fg_count"] == 0
    assert np.array_equal(a["masked_depth"], im[:, :, 2])
    for v in ((0, 0, 0), (0, 0, 1)):              # 3 x 4: never min_pts pixels
        a = _both(*S.tiny_scene(v)[:2])
        assert (a["mask"] == 255).all() and a["top_left"] == (3, 2) and a["bot_right"] == (0, 0)


def test_ids_follow_the_first_pixel_and_ties_sort_by_id():
    bg, im, nn, nb, _ = S.ids_scene()             # 135 pixels from (1, 0); the rest, mostly below, reaches row 0: id 0
    a = _both(bg, im, nn, nb)
    assert a["mask"][1, 0] == 1 and a["mask"][0, 0] == 0 and a["mask"][19, 0] == 0
    assert a["comps"] == [(265, 0), (135, 1)]
    bg, im, nn, nb, _ = S.ids_scene(equal=True)   # 200 / 200: equal sizes sort by id, descending
    a = _both(bg, im, nn, nb)
    assert a["comps"] == [(200, 1), (200, 0)]


def test_denormal_image_depth_is_a_candidate():
    """z = 1e-40 is nonzero: a candidate, and a background point at the same denormal depth is not skipped"""
    bg, im, nn, nb, _ = S.denormal_scene()
    a = _both(bg, im, nn, nb)
    dead = np.zeros((12, 12), bool)
    dead[4:8, 4:8] = True
    assert (a["mask"][dead] == 255).all() and (a["mask"][~dead] == 0).all() and a["comps"] == [(128, 0)]


# ---- the restatements agree on every generator of the GPU edge tests (tests/test_gpu_bgsub_edges.py), at small sizes

def _agree(scene, prev_box=PREV):
    bg, im, nn, nb = scene[:4]
    return _both(bg, im, nn, nb, prev_box)


@pytest.mark.parametrize("shape", [(1, 1), (1, 200), (200, 1), (31, 33), (32, 32), (33, 31), (64, 64), (65, 97)])
def test_restatements_agree_on_blocky_scenes(shape):
    for seed in range(3):                         # the GPU test's scenes at these sizes
        _agree(S.blocky_scene(*shape, seed=seed, k=100 if min(shape) < 8 else None))
    _agree(S.blocky_scene(*shape, seed=3, k=40))


@pytest.mark.parametrize("name", [n for n, _ in S.hard_shape_scenes(45, 70)])
def test_restatements_agree_on_hard_shapes(name):
    a = _agree(dict(S.hard_shape_scenes(45, 70))[name])
    if name in ("serpentine", "spiral"):
        assert len(a["comps"]) == 1 and a["comps"][0][0] > 1000
    if name == "comb":
        assert len(a["comps"]) == 1
    if name == "checker_1":
        assert a["comps"] == []                   # corner contacts do not join: every pixel alone


def test_hard_shapes_have_their_structure():
    """the shapes at the GPU size: one component for the paths and the comb, the interleaved U shapes ordered by
    their first pixel, corner contacts never joining"""
    sc = dict(S.hard_shape_scenes())
    for name in ("serpentine", "spiral", "comb"):
        bg, im = sc[name][:2]
        a = R.fast(bg, im)
        assert len(a["comps"]) == 1 and a["comps"][0][0] == int((im[:, :, 2] != 0).sum()), name
    a = R.fast(*sc["u"][:2])
    assert a["mask"][0, 120] == 0 and a["mask"][2, 125] == 1 and a["mask"][90, 10] == 0 and a["mask"][95, 5] == 1
    assert len(a["comps"]) == 2
    assert R.fast(*sc["checker_1"][:2])["comps"] == []
    a = R.fast(*sc["checker_11"][:2])
    assert len(a["comps"]) == 50 and all(s == 121 for s, _ in a["comps"])   # the full 11 x 11 squares of 9 x 11, half of them on
    a = R.fast(*sc["staircase"][:2])
    # every staircase of >= 100 pixels (those from column s <= 78) is its own component; the diagonals are specks
    assert len(a["comps"]) == 27 and all(s >= 100 for s, _ in a["comps"]) and a["mask"][5, 0] == 255


def test_restatements_agree_on_near_threshold_fields():
    for seed, shape in ((0, (37, 45)), (1, (64, 96))):
        scene, ks = S.near_background_field(*shape, seed=seed)
        _agree(scene)
        scene, (coff, roff, _, _) = S.near_neighbour_field(*shape, seed=seed)
        assert (np.abs(coff) <= 2).all() and (np.abs(roff) <= 2).all()
        _agree(scene)


def test_near_threshold_fields_have_teeth():
    """most placed pairs sit within 2 ulp of the threshold, many on each side and many exactly on it"""
    for shape in ((720, 1280), (301, 467)):
        (bg, im, nn_rel, _, _), ks = S.near_background_field(*shape)
        nn, _ = R.thresholds(*shape, nn_rel, nn_rel)
        placed = ks != 99
        d = bg - im
        sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        off = sq.view(np.int32).astype(np.int64) - np.array(nn, F).view(np.int32)
        assert np.array_equal(off[placed], ks[placed])
        assert placed.mean() > 0.5 and (ks[placed] < 0).mean() > 0.3 and (ks[placed] >= 0).mean() > 0.5 and (ks == 0).mean() > 0.1
        _, (coff, roff, ccuts, rcuts) = S.near_neighbour_field(*shape)
        assert (np.abs(coff) <= 2).all() and (np.abs(roff) <= 2).all() and len(coff) == len(ccuts) and len(roff) == len(rcuts)
        both = np.concatenate([coff, roff])
        assert (both <= 0).mean() > 0.3 and (both > 0).mean() > 0.2 and (coff == 0).sum() >= 3


@pytest.mark.parametrize("n_kept", [253, 254, 255])
def test_restatements_agree_on_cap_blocks(n_kept):
    bg, im, nn, nb, prev = S.cap_blocks_scene(n_kept)
    a = _both(bg, im, nn, nb, prev)
    assert a["capped"] == (n_kept >= 254) and len(a["comps"]) == min(n_kept, 254)
    assert (a["mask"][10:20, 19] == 255).all() and a["mask"][10, 10] == 255      # small before the cap
    assert a["mask"][90, 250] == 252 and a["mask"][90, 259] == 252                # the 253rd kept block from row 90
    small_after = a["mask"][100, 10 * (n_kept - 253 + 1)]
    assert small_after == (254 if n_kept >= 254 else 255)
    if n_kept >= 254:
        assert a["mask"][100, 0] == 253 and a["top_left"] == PREV[0]
    if n_kept == 255:
        assert a["mask"][100, 10] == 254


@pytest.mark.parametrize("cols", [1009, 1000])
def test_columns_fill_the_kept_list(cols):
    bg, im, nn, nb, _ = S.columns_scene(cols)
    a = R.fast(bg, im, nn, nb, PREV)
    assert R.min_points(100, cols) == 100 and a["capped"] and a["comps"] == [(100, i) for i in range(254)]
    assert np.array_equal(a["mask"][0, :254], np.arange(254)) and (a["mask"][:, 254:] == 254).all()
    b = R.literal(bg[:, :300], im[:, :300], nn * 300 / cols, nb * 300 / cols, PREV)   # the scan agrees on a slice of it
    assert R.same(b, R.fast(bg[:, :300], im[:, :300], nn * 300 / cols, nb * 300 / cols, PREV))


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
