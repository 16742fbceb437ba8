"""The render occlusion without a GPU: the CPU helper (tests/occlusion_restatement.py) against flags written out by hand, and the two
calls of the C ABI the mode adds (include/avt.h: avt_set_occlusion_render, avt_get_visibility) in the library and in the binding."""
import ctypes

import numpy as np
import pytest

import occlusion_cases as oc
import occlusion_restatement as occ

SCENES = oc.scenes()


@pytest.mark.parametrize("name", list(SCENES))
def test_helper_equals_the_flags_written_by_hand(name):
    s = SCENES[name]
    W, H = oc.S32
    assert np.array_equal(occ.backface(s["cloud"], s["mesh"]), s["backface"]), (name, s["why"])
    assert np.array_equal(occ.visible(s["cloud"], s["mesh"], oc.K32, W, H), s["visible"]), (name, s["why"])


def test_helper_follows_the_face_image_behind_the_camera():
    """renderFaces culls nothing by depth: a front-facing face with a vertex at z < 0 whose mirrored projection owns pixels is seen."""
    s = oc.behind_but_painted()
    assert np.array_equal(occ.visible(s["cloud"], s["mesh"], oc.K32, *oc.S32), s["visible"])


def test_helper_marks_a_subset_of_the_back_face_flags():
    import avatar_render_cases as rc
    k, size = rc.cam(33, 17, f=64.0)
    cloud = np.array(rc._soup(k, size, 85, 3))
    mesh = np.arange(255).reshape(85, 3)
    vis, bf = occ.visible(cloud, mesh, k, *size), occ.backface(cloud, mesh)
    assert vis.any() and (vis <= bf).all() and (vis < bf).any()


def test_library_exports_and_binding():
    """fails without the feature: the symbols are new"""
    from avatar_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("avt_set_occlusion_render", "avt_get_visibility"):
        getattr(lib, sym)
        assert sym in capi.SIGNATURES and sym in capi.EXPORTED_SYMBOLS
    assert capi.SIGNATURES["avt_set_occlusion_render"] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_float] * 4
    assert capi.SIGNATURES["avt_get_visibility"] == [ctypes.c_void_p, ctypes.c_int, capi.c_ubyte_p]
    from avatar_amd import api, tracker
    assert hasattr(api.Context, "set_occlusion_render") and hasattr(api.Context, "get_visibility")
    assert "render_occlusion" in tracker.MultiFrameTracker.__init__.__code__.co_varnames
    assert "render_occlusion" in tracker.FrameTracker.__init__.__code__.co_varnames
