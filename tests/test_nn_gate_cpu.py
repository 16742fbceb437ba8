"""The correspondence gate without a GPU: the three calls the C ABI adds (include/avt.h: avt_set_corr_gate, avt_get_corr_gate,
avt_get_gated) in the library and in the binding, the numpy restatement (tests/nn_gate_restatement.py) on boundary cases written
out by hand, and what the GPU sweep of tests/test_gpu_nn_gate.py rests on: under median_gates every group of tests/nn_cases.py
has a case that both drops and keeps matches, and some match sits exactly on its gate."""
import ctypes

import numpy as np
import pytest

import nn_cases
import nn_gate_restatement as ng
import nn_restatement as nr


def test_library_exports_and_binding():
    """fails without the feature: the symbols are new"""
    from avatar_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("avt_set_corr_gate", "avt_get_corr_gate", "avt_get_gated"):
        getattr(lib, sym)
        assert sym in capi.SIGNATURES and sym in capi.EXPORTED_SYMBOLS
    assert capi.SIGNATURES["avt_set_corr_gate"] == [ctypes.c_void_p, ctypes.c_int, capi.c_double_p]
    assert capi.SIGNATURES["avt_get_corr_gate"] == [ctypes.c_void_p, capi.c_double_p]
    assert capi.SIGNATURES["avt_get_gated"] == [ctypes.c_void_p, ctypes.c_int, capi.c_int_p]
    from avatar_amd import api, tracker
    for name in ("set_corr_gate", "corr_gate", "gated"):
        assert hasattr(api.Context, name)
    assert hasattr(api.AvatarOptimizer, "set_correspondence_gate") and hasattr(api.AvatarOptimizer, "last_gated")
    assert "max_corr_dist" in tracker.MultiFrameTracker.__init__.__code__.co_varnames
    assert "max_corr_dist" in tracker.FrameTracker.__init__.__code__.co_varnames


# ---- boundary cases written out by hand: one model point at the origin -------------------------------------------------
ORIGIN = np.zeros((1, 3))


def _one(query, g):
    corr, n = ng.gate_ref(np.zeros(1, np.int32), ORIGIN, np.array([query], np.float64), np.zeros(1, np.int32), g)
    return int(corr[0]), n


def test_a_match_exactly_on_the_gate_is_kept_and_one_ulp_below_is_dropped():
    assert _one((0.5, 0, 0), 0.5) == (0, 0)                              # d2 = 0.25 == g2
    assert _one((0.5, 0, 0), np.nextafter(0.5, 0)) == (-1, 1)            # g2 < 0.25
    assert _one((0.5, 0, 0), np.nextafter(0.5, 1)) == (0, 0)


def test_gate_zero_keeps_only_distance_zero():
    assert _one((0, 0, 0), 0.0) == (0, 0)
    assert _one((5e-324, 0, 0), 0.0) == (0, 0)                           # d2 underflows to 0: the search's own minimum is 0
    assert _one((1e-150, 0, 0), 0.0) == (-1, 1)                          # d2 = 1e-300
    corr, n = ng.gate_ref(np.zeros(3, np.int32), ORIGIN, np.array([[0, 0, 0], [0, 1e-9, 0], [0, 0, 0]], np.float64), np.zeros(3, np.int32), 0.0)
    assert corr.tolist() == [0, -1, 0] and n == 1


def test_gate_infinity_keeps_the_largest_finite_distance():
    x = np.sqrt(1.79e308)
    m, d2 = ng.matched_d2(np.zeros(1, np.int32), ORIGIN, np.array([[x, 0, 0]]))
    assert np.isfinite(d2[0]) and d2[0] > 1.78e308
    assert _one((x, 0, 0), np.inf) == (0, 0) and _one((x, 0, 0), None) == (0, 0)
    assert _one((x, 0, 0), 1e154) == (-1, 1)                             # g2 = 1e308 < d2


def test_an_unmatched_query_is_not_counted_and_gates_are_per_part():
    cloud = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    data = np.array([[0.3, 0, 0], [1.3, 0, 0], [9.0, 0, 0]])
    corr = np.array([0, 1, -1], np.int32)
    labels = np.array([0, 1, 1], np.int32)
    out, n = ng.gate_ref(corr, cloud, data, labels, [0.1, np.inf])
    assert out.tolist() == [-1, 1, -1] and n == 1
    out, n = ng.gate_ref(corr, cloud, data, labels, [np.inf, 0.1])
    assert out.tolist() == [0, -1, -1] and n == 1
    assert ng.median_gates(corr, cloud, data, labels, 3).tolist() == [np.sqrt(0.3 * 0.3), np.sqrt((1.3 - 1.0) * (1.3 - 1.0)), np.inf]


# ---- the sweep must not hide a kernel that never gates ------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep_counts(smpl):
    """Per group: for every case (name, dropped, kept, on the gate) under median_gates, from the restatement alone."""
    out = {}
    for group in nn_cases.GROUPS:
        rows = []
        for name, pm, npart, cloud, vis, data, labels in nn_cases.cases(smpl, group):
            corr = nr.nn_ref(nn_cases.part_of_vertex(smpl, pm), npart, cloud, vis, data, labels)
            g = ng.median_gates(corr, cloud, data, labels, npart)
            gated, n = ng.gate_ref(corr, cloud, data, labels, g)
            assert n == int(((corr >= 0) & (gated < 0)).sum()) and np.array_equal(gated[gated >= 0], corr[gated >= 0])
            rows.append((name, n, int((gated >= 0).sum()), ng.on_gate(corr, cloud, data, labels, g)))
        out[group] = rows
    return out


@pytest.mark.parametrize("group", list(nn_cases.GROUPS))
def test_every_group_has_a_case_that_drops_and_keeps(sweep_counts, group):
    mixed = [name for name, dropped, kept, _ in sweep_counts[group] if dropped > 0 and kept > 0]
    print(f"{group}: {len(mixed)} of {len(sweep_counts[group])} cases both drop and keep")
    assert mixed, f"{group}: no case both drops and keeps a match under median_gates"


def test_some_match_sits_exactly_on_its_gate(sweep_counts):
    total = sum(n for rows in sweep_counts.values() for _, _, _, n in rows)
    print(f"{total} matched queries with d2 == g2")
    assert total >= 1
