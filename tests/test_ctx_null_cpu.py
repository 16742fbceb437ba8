"""A null context through the entry points of avatar_amd/csrc/avt_capi.cpp that take one: each is refused with its text before any
device is touched, so this runs without a GPU.  avt_sync used to dereference the pointer."""
import pytest

CALLS = [
    ("avt_sync", (), "avt_sync: null context"),
    ("avt_state_reset", (), "avt_state_reset: no state resident"),
    ("avt_state_download", (None, None, None, None), "avt_state_download: null context"),
    ("avt_state_upload", (1, None, None, None), "avt_state_upload: null argument"),
    ("avt_frames_upload", (1, None, None, None), "avt_frames_upload: null argument"),
    ("avt_frames_download", (0, None, None), "avt_frames_download: bad argument"),
    ("avt_optimize_resident", (None,), "avt_optimize_resident: null argument"),
    ("avt_optimize_resident_budgets", (None, None), "avt_optimize_resident_budgets: null argument"),
    ("avt_lbs_update", (1, None, None, None, None, None, None), "avt_lbs_update: null argument"),
    ("avt_visibility", (None, 1, None), "avt_visibility: null argument"),
    ("avt_get_correspondences", (0, None), "avt_get_correspondences: bad argument"),
    ("avt_get_cloud", (0, None), "avt_get_cloud: bad argument"),
    ("avt_get_posed", (0, None, None, None), "avt_get_posed: bad argument"),
    ("avt_get_visibility", (0, None), "avt_get_visibility: bad argument"),
    ("avt_get_normal_equations", (0, None, None, None), "avt_get_normal_equations: bad argument"),
    ("avt_debug_mfma_count", (0, None, None, None), "avt_debug_mfma_count: bad argument"),
    ("avt_debug_nn_sums", (0, None, None, None), "avt_debug_nn_sums: bad argument"),
    ("avt_debug_trace", (0, None), "avt_debug_trace: bad argument"),
    ("avt_set_corr_gate", (0, None), "avt_set_corr_gate: null context"),
    ("avt_get_corr_gate", (None,), "avt_get_corr_gate: null argument"),
    ("avt_get_gated", (0, None), "avt_get_gated: bad argument"),
    ("avt_set_corr_trim", (0, None, None, None, 1), "avt_set_corr_trim: null context"),
    ("avt_get_corr_trim", (None, None, None, None), "avt_get_corr_trim: null context"),
    ("avt_get_trimmed", (0, None, None), "avt_get_trimmed: null argument"),
    ("avt_get_trim_thresholds", (0, None), "avt_get_trim_thresholds: null argument"),
    ("avt_set_data_term", (0,), "avt_set_data_term: bad argument"),
    ("avt_set_occlusion_render", (0, 0, 0.0, 0.0, 0.0, 0.0), "avt_set_occlusion_render: null context"),
    ("avt_ctx_get_tuning", (None,), "avt_ctx_get_tuning: null argument"),
    ("avt_ctx_set_tuning", (None,), "avt_ctx_set_tuning: null argument"),
    ("avt_launch_shape", (None, None, None), "avt_launch_shape: no frames resident"),
    ("avt_profile_begin", (), "avt_profile_begin: null context"),
    ("avt_profile_select", (0,), "avt_profile_select: null context"),
    ("avt_profile_end", (None,), "avt_profile_end: null argument"),
]


@pytest.mark.parametrize("name,args,text", CALLS, ids=[c[0] for c in CALLS])
def test_a_null_context_is_refused_with_a_text(name, args, text):
    from avatar_amd import capi
    lib = capi.load_library()
    assert getattr(lib, name)(None, *args) == 1
    assert lib.avt_last_error().decode() == text


def test_the_data_term_of_a_null_context():
    from avatar_amd import capi
    lib = capi.load_library()
    assert lib.avt_get_data_term(None) == -1
    lib.avt_ctx_destroy(None)
