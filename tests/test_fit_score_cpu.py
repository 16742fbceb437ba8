"""CPU tests of the fit score (include/avt_fitscore.h): the numpy restatement against tables worked out by hand on a 3 x 4 image
that holds every class, fitscore.metrics against ark::FitScore::derive through tests/cpp/fit_score_demo (the same doubles, NaN
cases included), the ABI's names in the built library and in the Python binding, and the argument refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fit_score_cases as fc
import fit_score_restatement as fr
from avatar_amd import capi, fitscore

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEMO = os.path.join(HERE, "cpp", "fit_score_demo")


def test_restatement_against_tables_by_hand():
    args = (fc.HAND_R, fc.HAND_M, fc.HAND_D)
    for want, kw in ((fc.HAND_TABLE, {}), (fc.HAND_TABLE_STRIDE2, dict(stride=2)), (fc.HAND_TABLE_TOL_QUARTER, dict(tol=0.25)),
                     (fc.HAND_TABLE_TOL_ZERO, dict(tol=0.0)), (fc.HAND_TABLE_TOL_INF, dict(tol=np.inf)),
                     (fc.HAND_TABLE_WHOLE, dict(box=(0, 0, -1, -1))), (fc.HAND_TABLE_WHOLE, dict(box=None)), (fc.HAND_TABLE_WHOLE, dict(box=(0, 0, 3, 2)))):
        kw = dict(dict(box=fc.HAND_BOX, tol=fc.HAND_TOL, P=fc.HAND_P), **kw)
        got = fr.table(*args, **kw)
        assert got.dtype == np.int64 and np.array_equal(got, want), kw
    # every class occurs, on a part row and on row P
    assert (fc.HAND_TABLE[:, :5].sum(0) > 0).all() and fc.HAND_TABLE[2, :5].sum() == 3
    # an empty box and one partly outside select no observed pixel: the model pixels are all MODEL_ONLY
    for box in ((2, 0, 1, 2), (0, 0, 4, 2), (0, -1, 3, 2)):
        got = fr.table(*args, box=box, tol=fc.HAND_TOL, P=fc.HAND_P)
        assert got[:, fitscore.MODEL_ONLY].tolist() == [3, 3, 2] and got.sum() == 8, box
    # a bad label counts only where it is selected, and then whatever R is
    bad = fc.HAND_M.copy()
    bad[2, 1] = 2
    assert fc.HAND_R[2, 1] == 0
    with pytest.raises(ValueError, match="num_parts"):
        fr.table(fc.HAND_R, bad, fc.HAND_D, fc.HAND_BOX, fc.HAND_TOL, 1, fc.HAND_P)
    assert np.array_equal(fr.table(fc.HAND_R, bad, fc.HAND_D, fc.HAND_BOX, fc.HAND_TOL, 2, fc.HAND_P), fc.HAND_TABLE_STRIDE2)
    # the stack form, one box per image
    both = fr.tables(np.stack([fc.HAND_R] * 2), np.stack([fc.HAND_M] * 2), np.stack([fc.HAND_D] * 2), [fc.HAND_BOX, (0, 0, -1, -1)], fc.HAND_TOL, 1, fc.HAND_P)
    assert np.array_equal(both, np.stack([fc.HAND_TABLE, fc.HAND_TABLE_WHOLE]))
    # +inf against +inf: the NaN delta is BEHIND with the clamp; rounding is to nearest even
    one = lambda r, d, **kw: fr.table(np.array([[r]], np.float32), np.zeros((1, 1), np.uint8), np.array([[d]], np.float32), P=1, **kw)[0].tolist()
    assert one(np.inf, np.inf) == [0, 0, 1, 0, 0, 10 ** 9, 0]
    assert one(np.inf, np.inf, tol=np.inf) == [0, 0, 1, 0, 0, 10 ** 9, 0]
    assert one(1.0, 1.0 + 2.0 ** -21) == [1, 0, 0, 0, 0, 0, 0]                  # 0.476837 um rounds to 0
    assert one(2.0 ** -21, 2.0 ** -20) == [1, 0, 0, 0, 0, 0, 0]
    assert one(1.0, 1.0 + 2.0 ** -20)[5] == 1                                   # 0.953674 um
    assert one(1.0, 1.0078125)[5] == 7812 and one(1.0, 1.0234375)[5] == 23438  # 7812.5 and 23437.5 um: ties go to the even integer
    assert one(1e-40, 1e-40) == [1, 0, 0, 0, 0, 0, 0]                           # a denormal is data, and model


def _metrics_by_hand():
    nan = np.nan
    t = fc.HAND_TABLE
    m = fitscore.metrics(t)
    both, mo, do = 4, 4, 1
    assert m["iou"] == both / (both + mo + do) and m["agree"] == 1 / 4
    assert m["violation"] == (2 + 4) / (4 + 4) and m["unexplained"] == (1 + 1) / (4 + 1)
    assert m["mean_abs_err"] == 1000812500 / 4 * 1e-6 and m["mean_abs_err_agree"] == 62500 / 1 * 1e-6
    assert np.array_equal(m["part_agree"], [1.0, 0.0, 0.0]) and np.array_equal(m["part_violation"], [2 / 3, 3 / 3, 1 / 2])
    assert np.array_equal(m["part_mean_abs_err"], [62500 / 1 * 1e-6, 1000250000 / 2 * 1e-6, 500000 / 1 * 1e-6])
    assert np.array_equal(m["part_mean_abs_err_agree"], [62500 / 1 * 1e-6, nan, nan], equal_nan=True)
    return m


def test_metrics_by_hand_and_nan_cases():
    _metrics_by_hand()
    z = fitscore.metrics(np.zeros((3, 7), np.int64))
    assert all(np.isnan(z[k]) for k in ("iou", "agree", "violation", "unexplained", "mean_abs_err", "mean_abs_err_agree"))
    assert all(np.isnan(z["part_" + k]).all() and z["part_" + k].shape == (3,) for k in ("agree", "violation", "mean_abs_err", "mean_abs_err_agree"))
    only = np.zeros((2, 7), np.int64)
    only[1, fitscore.DATA_ONLY] = 9                                          # data alone: the model explains nothing
    m = fitscore.metrics(only)
    assert m["iou"] == 0.0 and m["unexplained"] == 1.0 and np.isnan(m["agree"]) and np.isnan(m["violation"]) and np.isnan(m["mean_abs_err"])
    stack = fitscore.metrics(np.stack([fc.HAND_TABLE, fc.HAND_TABLE_WHOLE]))
    assert len(stack) == 2 and stack[1]["iou"] == 5 / (5 + 3 + 3)
    with pytest.raises(ValueError):
        fitscore.metrics(np.zeros((3, 6), np.int64))
    assert fitscore.COLUMNS[fitscore.ABS_UM_AGREE] == "ABS_UM_AGREE" and len(fitscore.COLUMNS) == 7


def _derive_cpp(table, min_iou, max_violation, tmp_path):
    P = table.shape[0] - 1
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        np.array([P], np.int32).tofile(fh)
        np.ascontiguousarray(table, np.int64).tofile(fh)
        np.array([min_iou, max_violation], np.float64).tofile(fh)
    r = subprocess.run([DEMO, "derive", inp, outp], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    v = np.fromfile(outp, np.float64)
    assert len(v) == 6 + 6 * (P + 1) + 4 * (P + 1) + 1
    return v[:6], v[6:6 + 6 * (P + 1)].reshape(P + 1, 6), v[6 + 6 * (P + 1):-1].reshape(P + 1, 4), bool(v[-1])


def test_metrics_equal_the_cpp_derive(tmp_path):
    assert os.path.exists(DEMO), "tests/cpp/fit_score_demo not built (make -C avatar_amd/csrc facade)"
    rng = np.random.default_rng(5)
    big = rng.integers(0, 2 ** 40, (25, 7)).astype(np.int64)
    big[3] = 0                                                               # an empty row: NaN everywhere
    big[4, :3] = 0                                                           # a row with model only
    huge = np.full((2, 7), 2 ** 59 + 1, np.int64)                            # sums beyond 2^53: the one conversion rounds
    same = lambda a, b: np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)
    for t in (fc.HAND_TABLE, fc.HAND_TABLE_WHOLE, np.zeros((3, 7), np.int64), big, huge):
        total, rows, parts, _ = _derive_cpp(t, 0.5, 0.5, tmp_path)
        m = fitscore.metrics(t)
        assert same(total, [m[k] for k in ("iou", "agree", "violation", "unexplained", "mean_abs_err", "mean_abs_err_agree")])
        assert np.isnan(rows[:, 0]).all() and np.isnan(rows[:, 3]).all()   # iou and unexplained have no per-part form
        for col, key in ((1, "agree"), (2, "violation"), (4, "mean_abs_err"), (5, "mean_abs_err_agree")):
            assert same(rows[:, col], m["part_" + key]), key
        assert same(parts, rows[:, [1, 2, 4, 5]])
    # fitLost: either bound crossed, or a NaN figure
    m = _metrics_by_hand()                                                   # iou 4/9, violation 6/8
    assert _derive_cpp(fc.HAND_TABLE, 0.4, 0.8, tmp_path)[3] is False
    assert _derive_cpp(fc.HAND_TABLE, m["iou"], m["violation"], tmp_path)[3] is False      # the bounds themselves are not crossed
    assert _derive_cpp(fc.HAND_TABLE, 0.5, 0.8, tmp_path)[3] is True
    assert _derive_cpp(fc.HAND_TABLE, 0.4, 0.7, tmp_path)[3] is True
    assert _derive_cpp(np.zeros((3, 7), np.int64), 0.0, 1.0, tmp_path)[3] is True


def test_every_declared_function_is_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "avt_fitscore.h")).read()
    declared = re.findall(r"^(?:int|void) (avt_fitscore_\w+)\(", header, re.M)
    assert len(declared) == 7 and sorted(declared) == sorted(fitscore.FITSCORE_SYMBOLS)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert header.count("live-demo.cpp:428-445") >= len(declared)       # each entry cites the display it quantifies


def test_argument_refusals_that_need_no_device():
    lib = capi.load_library()
    err = lambda: lib.avt_last_error()
    h = ctypes.c_void_p()
    for P in (0, -1, 255):
        assert lib.avt_fitscore_create(-1, P, 4, ctypes.byref(h)) != 0 and b"num_parts" in err()
    assert lib.avt_fitscore_create(-1, 24, 0, ctypes.byref(h)) != 0 and b"max_images" in err()
    assert lib.avt_fitscore_create(-1, 24, 4, None) != 0 and b"null" in err()
    R, M, D = np.ones((1, 3, 4), np.float32), np.zeros((1, 3, 4), np.uint8), np.ones((1, 3, 4), np.float32)
    rp, mp, dp = capi.ptr(R, ctypes.c_float), capi.ptr(M, ctypes.c_ubyte), capi.ptr(D, ctypes.c_float)
    f32, i32 = ctypes.c_float, ctypes.c_int
    assert lib.avt_fitscore_images(None, 1, 3, 4, rp, mp, dp, None, f32(0.05), 1) != 0 and b"null" in err()
    assert lib.avt_fitscore_rendered(None, None, dp, None, f32(0.05), 1) != 0 and b"null" in err()
    assert lib.avt_fitscore_rendered_from_bgsub(None, None, None, None, f32(0.05), 1) != 0 and b"null" in err()
    assert lib.avt_fitscore_get(None, None, None) != 0 and b"null" in err()
    assert lib.avt_fitscore_sync(None) != 0 and b"null" in err()
    lib.avt_fitscore_destroy(None)
    s = fitscore.FitScorer(254, 2, device=-1)                                # host-only: checks arguments, refuses to score
    fitscore.FitScorer(1, 1, device=-1)
    for tol in (-0.01, np.nan, -np.inf):
        with pytest.raises(capi.AvtError, match="tol"):
            s.score_images(R, M, D, tol=tol)
        assert lib.avt_fitscore_rendered(s._h, None, dp, None, f32(tol), 1) != 0 and b"tol" in err()
        assert lib.avt_fitscore_rendered_from_bgsub(s._h, None, None, None, f32(tol), 1) != 0 and b"tol" in err()
    for stride in (0, -2):
        with pytest.raises(capi.AvtError, match="stride"):
            s.score_images(R, M, D, stride=stride)
        assert lib.avt_fitscore_rendered(s._h, None, dp, None, f32(0.05), i32(stride)) != 0 and b"stride" in err()
        assert lib.avt_fitscore_rendered_from_bgsub(s._h, None, None, None, f32(0.05), i32(stride)) != 0 and b"stride" in err()
    for args in ((None, mp, dp), (rp, None, dp), (rp, mp, None)):
        assert lib.avt_fitscore_images(s._h, 1, 3, 4, *args, None, f32(0.05), 1) != 0 and b"null" in err()
    assert lib.avt_fitscore_rendered(s._h, None, None, None, f32(0.05), 1) != 0 and b"null" in err()
    for n, rows, cols in ((0, 3, 4), (1, 0, 4), (1, 3, 0), (1, 32768, 1)):
        assert lib.avt_fitscore_images(s._h, n, rows, cols, rp, mp, dp, None, f32(0.05), 1) != 0 and b"n_images" in err()
    assert lib.avt_fitscore_images(s._h, 3, 3, 4, rp, mp, dp, None, f32(0.05), 1) != 0 and b"created for 2" in err()
    with pytest.raises(capi.AvtError, match="host-only"):                   # +inf and 0 are tolerances; the device is what is missing
        s.score_images(R, M, D, tol=np.inf)
    with pytest.raises(capi.AvtError, match="host-only"):
        s.score_images(R, M, D, tol=0.0)
    assert lib.avt_fitscore_rendered(s._h, None, dp, None, f32(0.05), 1) != 0 and b"host-only" in err()
    assert lib.avt_fitscore_rendered_from_bgsub(s._h, None, None, None, f32(0.05), 1) != 0 and b"host-only" in err()
    with pytest.raises(capi.AvtError, match="host-only"):
        s.sync()
    with pytest.raises(capi.AvtError, match="no score"):
        s.get()
    with pytest.raises(ValueError):
        s.score_images(R, M[:, :2], D)
    with pytest.raises(ValueError):
        s.score_images(R, M, D, boxes=[(0, 0, -1, -1)] * 2)
