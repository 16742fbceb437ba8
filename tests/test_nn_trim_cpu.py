"""Trimmed ICP without a GPU: the four calls the C ABI adds (include/avt.h: avt_set_corr_trim, avt_get_corr_trim, avt_get_trimmed,
avt_get_trim_thresholds) in the library and in the binding, the numpy restatement (tests/nn_trim_restatement.py) against the
expectations written out by hand (tests/nn_trim_cases.py), and what the GPU tests of tests/test_gpu_nn_trim.py rest on: at rho = 0.5,
kappa = 1 every group of tests/nn_cases.py has parts that both drop and keep, matches sit exactly on their threshold, no case is
skipped, and on the contaminated frame the settings of the fits drop what the fits say they drop and keep point 0."""
import ctypes

import numpy as np
import pytest

import nn_cases
import nn_gate_restatement as ng
import nn_restatement as nr
import nn_trim_cases as tc
import nn_trim_restatement as nt


def test_library_exports_and_binding():
    """fails without the feature: the symbols are new"""
    from avatar_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("avt_set_corr_trim", "avt_get_corr_trim", "avt_get_trimmed", "avt_get_trim_thresholds"):
        getattr(lib, sym)
        assert sym in capi.SIGNATURES and sym in capi.EXPORTED_SYMBOLS
    vp, dp, ip, ci = ctypes.c_void_p, capi.c_double_p, capi.c_int_p, ctypes.c_int
    assert capi.SIGNATURES["avt_set_corr_trim"] == [vp, ci, dp, dp, dp, ci]
    assert capi.SIGNATURES["avt_get_corr_trim"] == [vp, dp, dp, dp, ip]
    assert capi.SIGNATURES["avt_get_trimmed"] == [vp, ci, ip, ip]
    assert capi.SIGNATURES["avt_get_trim_thresholds"] == [vp, ci, dp]
    from avatar_amd import api, tracker
    for name in ("set_corr_trim", "corr_trim", "trimmed", "trim_thresholds"):
        assert hasattr(api.Context, name)
    assert hasattr(api.AvatarOptimizer, "last_trimmed")
    assert "corr_trim" in tracker.MultiFrameTracker.__init__.__code__.co_varnames and hasattr(tracker.MultiFrameTracker, "set_corr_trim")
    assert "corr_trim" in tracker.FrameTracker.__init__.__code__.co_varnames


def test_the_headers_declare_the_calls_and_the_facade_members():
    import os
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    avt = open(os.path.join(inc, "avt.h")).read()
    for sym in ("avt_set_corr_trim", "avt_get_corr_trim", "avt_get_trimmed", "avt_get_trim_thresholds"):
        assert f"int {sym}(avt_ctx*" in avt
    opt = open(os.path.join(inc, "ark", "AvatarOptimizer.h")).read()
    for member in ("trimQuantile", "trimFactor", "trimFloor", "trimMinMatches"):
        assert member in opt
        assert member in open(os.path.join(inc, "ark", "FrameTracker.h")).read()
    assert "avt_set_corr_trim" in open(os.path.join(inc, "ark", "MultiFrameTracker.h")).read()


# ---- the restatement against the expectations written by hand -----------------------------------------------------------
def test_the_restatement_gives_the_hand_written_expectations(smpl):
    pm, npart, pov, cloud, vis, v0, v1 = tc.hand_model(smpl)
    names = set()
    for case in tc.hand_cases():
        name, data, labels, gate, (rho, kappa, floor, mm), want, gated, tp, T = tc.expand(case, v0, v1, npart)
        names.add(name)
        corr = nr.nn_ref(pov, npart, cloud, vis, data, labels)
        assert (corr >= 0).all(), name                                    # every query has a visible model point of its part
        cg, n = ng.gate_ref(corr, cloud, data, labels, gate)
        out, total, per_part, Tq = nt.trim_ref(cg, cloud, data, labels, npart, rho, kappa, floor, mm)
        assert n == gated and out.tolist() == want.tolist() and total == int(tp.sum()) and per_part.tolist() == tp.tolist(), name
        assert Tq.tobytes() == T.tobytes(), (name, Tq[:2], T[:2])
        assert int((corr >= 0).sum()) == int((out >= 0).sum()) + n + total, name
    assert len(names) == len(tc.hand_cases()) >= 27


def test_order_statistic_not_median_and_the_clamp():
    d2 = np.array([4.0, 1.0, 3.0, 2.0])
    part = np.zeros(4, np.int64)
    assert nt.thresholds(d2, part, 1, 0.5, 1.0)[0] == 2.0                 # k = 2: the 2nd smallest (the median would be 2.5)
    assert nt.thresholds(d2, part, 1, 0.51, 1.0)[0] == 3.0                # k = ceil(2.04) = 3
    assert nt.thresholds(d2, part, 1, 1e-300, 1.0)[0] == 1.0              # k clamped to 1
    assert nt.thresholds(d2, part, 1, 1.0, 1.0)[0] == 4.0                 # k = n
    assert nt.thresholds(d2, part, 1, 0.5, 3.0)[0] == 18.0                # kappa squared
    assert nt.thresholds(d2, part, 1, 0.5, 1.0, 2.0)[0] == 4.0            # floor squared decides
    assert nt.thresholds(d2, part, 1, 0.5, np.inf)[0] == np.inf           # the part is off
    assert nt.thresholds(d2, part, 1, 0.5, 1.0, 0.0, 5)[0] == np.inf      # n < min_matches
    assert nt.thresholds(d2, part, 1, 0.5, 1.0, 0.0, 4)[0] == 2.0
    assert nt.thresholds(d2, part, 2, 0.5, 1.0).tolist() == [2.0, np.inf]  # a part without matches


# ---- the sweep must not hide a kernel that never trims -------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep_rows(smpl):
    """Per group, for every case: (name, parts that both drop and keep, dropped, kept, matches on their threshold, parts with a finite
    threshold) at rho 0.5, kappa 1."""
    out = {}
    for group in nn_cases.GROUPS:
        rows = []
        for name, pm, npart, cloud, vis, data, labels in nn_cases.cases(smpl, group):
            corr = nr.nn_ref(nn_cases.part_of_vertex(smpl, pm), npart, cloud, vis, data, labels)
            trimmed, total, per_part, T = nt.trim_ref(corr, cloud, data, labels, npart, 0.5, 1.0)
            assert total == int(per_part.sum()) == int(((corr >= 0) & (trimmed < 0)).sum()) and np.array_equal(trimmed[trimmed >= 0], corr[trimmed >= 0])
            kept_pp = np.bincount(np.asarray(labels, np.int64)[trimmed >= 0], minlength=npart)
            rows.append((name, int(((per_part > 0) & (kept_pp > 0)).sum()), total, int((trimmed >= 0).sum()), nt.on_threshold(corr, cloud, data, labels, T),
                         int(np.isfinite(T).sum())))
        out[group] = rows
    return out


@pytest.mark.parametrize("group", list(nn_cases.GROUPS))
def test_every_group_has_parts_that_drop_and_keep(sweep_rows, group):
    rows = sweep_rows[group]
    assert rows, f"{group}: no case"
    mixed = [r[0] for r in rows if r[1] > 0]
    print(f"{group}: {len(mixed)} of {len(rows)} cases have a part that both drops and keeps; {sum(r[2] for r in rows)} dropped, {sum(r[3] for r in rows)} kept")
    assert mixed, f"{group}: no part both drops and keeps a match at rho = 0.5, kappa = 1"


def test_matches_sit_exactly_on_their_threshold(sweep_rows):
    total = sum(r[4] for rows in sweep_rows.values() for r in rows)
    more = sum(1 for rows in sweep_rows.values() for r in rows if r[4] > r[5])      # (every finite T is the d2 of one match at least)
    print(f"{total} matched queries with d2 == T; {more} cases with more of them than thresholds (ties on T, all kept)")
    assert total >= 1 and more >= 1


# ---- what the fits of the GPU tests rest on -------------------------------------------------------------------------------
def test_the_fit_settings_drop_what_the_gpu_tests_say(smpl, omodel):
    c = tc.contaminated(smpl, omodel)
    for (rho, kappa), inliers in (((0.75, 3.0), 8), ((0.5, 4.0), 35)):
        out, total, per_part, T = nt.trim_ref(c["ungated_corr"], c["cloud0"], c["D"], c["L"], 24, rho, kappa)
        print(f"rho {rho} kappa {kappa}: {total} dropped, {int((out[c['planted']] < 0).sum())} of them planted")
        assert (out[c["planted"]] == -1).all() and total == 300 + inliers
        assert out[0] >= 0                                               # index 0 (the frame's centre) is kept wherever a fit is compared
    assert (c["ungated_corr"] >= 0).all()
    d, l = c["clean"][0][:600], c["clean"][1][:600]
    corr = nr.nn_ref(nn_cases.part_of_vertex(smpl, c["pm"]), 24, c["cloud0"], np.ones(nn_cases.V, np.uint8), d, l)
    assert (ng.matched_d2(corr, c["cloud0"], d)[1] > 0).all()            # the 600 points of the everything-trimmed fit: nonzero distances
