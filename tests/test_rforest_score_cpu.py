"""CPU tests of the forest's score (include/avt_rforest.h, THE SCORE): the derived figures as one pure function of the matrix
(rforest.score_metrics), the restatement's counting rule on a case small enough to count by hand, the new names in the ABI
list, and the argument errors that need no device."""
import ctypes

import numpy as np
import pytest

import rforest_score_restatement as rs
from avatar_amd import capi, rforest
from test_rforest_cpu import GOLD


def _nan_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_score_metrics_by_hand():
    nan = np.nan
    #            predicted 0  1  2  none
    conf = np.array([[6, 1, 0, 3],          # truth 0
                     [2, 4, 0, 0],          # truth 1
                     [0, 0, 0, 0],          # truth 2 never occurs: an empty row
                     [1, 0, 2, 0]], np.int64)
    m = rforest.score_metrics(conf)
    assert m["accuracy"] == 10 / 16
    assert _nan_equal(m["recall"], [6 / 10, 4 / 6, nan])
    assert _nan_equal(m["precision"], [6 / 9, 4 / 5, 0 / 2])
    assert _nan_equal(m["iou"], [6 / (10 + 9 - 6), 4 / (6 + 5 - 4), 0 / 2])
    assert m["mean_iou"] == (6 / 13 + 4 / 7 + 0.0) / 3
    assert (m["missed"], m["spurious"]) == (3, 3)
    # a part that occurs neither in the truth nor in the prediction: its IoU is NaN and left out of the mean
    conf[3, 2] = 0
    m = rforest.score_metrics(conf)
    assert _nan_equal(m["iou"], [6 / 13, 4 / 7, nan]) and _nan_equal(m["precision"], [6 / 9, 4 / 5, nan]) and _nan_equal(m["recall"], [0.6, 4 / 6, nan])
    assert m["mean_iou"] == (6 / 13 + 4 / 7) / 2 and m["spurious"] == 1


def test_score_metrics_of_empty_and_none_only_matrices():
    m = rforest.score_metrics(np.zeros((5, 5), np.int64))
    assert np.isnan(m["accuracy"]) and np.isnan(m["mean_iou"]) and (m["missed"], m["spurious"]) == (0, 0)
    for key in ("recall", "precision", "iou"):
        assert m[key].shape == (4,) and np.isnan(m[key]).all()
    only = np.zeros((3, 3), np.int64)
    only[0, 2], only[1, 2], only[2, 0] = 7, 2, 5                    # counts in row and column P alone
    m = rforest.score_metrics(only)
    assert m["accuracy"] == 0.0 and (m["missed"], m["spurious"]) == (9, 5)
    assert _nan_equal(m["recall"], [0, 0]) and _nan_equal(m["precision"], [0, np.nan]) and _nan_equal(m["iou"], [0, 0]) and m["mean_iou"] == 0.0
    # exact in float64 beyond 2^24 and beyond 2^32
    big = np.array([[2 ** 40 + 1, 1], [0, 0]], np.int64)
    assert rforest.score_metrics(big)["accuracy"] == (2 ** 40 + 1) / (2 ** 40 + 2)
    with pytest.raises(ValueError):
        rforest.score_metrics(np.zeros((2, 3), np.int64))
    s = rforest.Score(only, 4, 99)
    assert (s.n_images, s.n_pixels, s.missed, s.spurious) == (4, 99, 9, 5) and s.accuracy == 0.0


def test_restatement_counts_by_hand():
    leaf = lambda row: (np.zeros((1, 5), np.float32), np.array([[-1, -1, 0]], np.int32), np.array([row], np.float32))
    depth = np.array([[1, 1, 0], [-1, np.nan, 1]], np.float32)
    mask = np.array([[0, 255, 1], [0, 1, 255]], np.uint8)
    conf, n = rs.confusion([leaf([0.25, 0.5, 0.5])], depth, mask)          # every walked pixel predicts part 1 (the tie's lower index)
    want = np.zeros((4, 4), np.int64)
    want[0, 1], want[3, 1], want[1, 3], want[0, 3] = 1, 2, 2, 1
    assert np.array_equal(conf, want) and n == 6
    conf, n = rs.confusion([leaf([0, 0, 0])], depth, mask)                 # nothing is predicted: only column P, and not [P][P]
    want = np.zeros((4, 4), np.int64)
    want[0, 3], want[1, 3] = 2, 2
    assert np.array_equal(conf, want)
    conf, n = rs.confusion([leaf([0.25, 0.5, 0.5])], depth, mask, stride=2)            # pixels (0, 0) and (0, 2)
    assert n == 2 and conf[0, 1] == 1 and conf[1, 3] == 1 and conf.sum() == 2
    both = rs.confusion([leaf([0.25, 0.5, 0.5])], np.stack([depth, depth]), np.stack([mask, mask]), stride=5)
    assert both[1] == 2 and both[0][0, 1] == 2 and both[0].sum() == 2
    bad = mask.copy()
    bad[1, 2] = 3
    with pytest.raises(ValueError, match="num_parts"):
        rs.confusion([leaf([0.25, 0.5, 0.5])], depth, bad)


def test_the_score_is_in_the_abi_list():
    for name in ("avt_rforest_score_reset", "avt_rforest_score_images", "avt_rforest_score_rendered", "avt_rforest_score_get"):
        assert name in rforest.RFOREST_SYMBOLS
        assert hasattr(ctypes.CDLL(capi.LIB_PATH), name)


def test_argument_errors_that_need_no_device():
    lib = capi.load_library()
    d = np.ones((1, 4, 6), np.float32)
    m = np.zeros((1, 4, 6), np.uint8)
    dp, mp = capi.ptr(d, ctypes.c_float), capi.ptr(m, ctypes.c_ubyte)
    conf = np.zeros(25 * 25, np.int64)
    assert lib.avt_rforest_score_reset(None) != 0 and b"null" in lib.avt_last_error()
    assert lib.avt_rforest_score_images(None, 1, 4, 6, dp, mp, 1) != 0 and b"null" in lib.avt_last_error()
    assert lib.avt_rforest_score_rendered(None, None, 1) != 0 and b"null" in lib.avt_last_error()
    assert lib.avt_rforest_score_get(None, capi.ptr(conf, ctypes.c_longlong), None, None) != 0 and b"null" in lib.avt_last_error()
    f = rforest.RForest([GOLD, GOLD], device=-1)
    assert lib.avt_rforest_score_images(f._h, 1, 4, 6, None, mp, 1) != 0 and b"null" in lib.avt_last_error()
    assert lib.avt_rforest_score_images(f._h, 1, 4, 6, dp, None, 1) != 0 and b"null" in lib.avt_last_error()
    for stride in (0, -3):
        with pytest.raises(RuntimeError, match="stride"):
            f.score_images(d, m, stride)
        assert lib.avt_rforest_score_rendered(f._h, None, stride) != 0 and b"stride" in lib.avt_last_error()
    assert lib.avt_rforest_score_images(f._h, 0, 4, 6, dp, mp, 1) != 0 and b"n_images" in lib.avt_last_error()
    assert lib.avt_rforest_score_images(f._h, 1, 0, 6, dp, mp, 1) != 0 and b"n_images" in lib.avt_last_error()
    with pytest.raises(RuntimeError, match="host-only"):
        f.score_images(d, m)
    assert lib.avt_rforest_score_rendered(f._h, None, 1) != 0 and b"host-only" in lib.avt_last_error()
    # the totals of a forest that has scored nothing are zeros, with or without a device
    conf[:] = -1
    ni, npx = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    assert lib.avt_rforest_score_get(f._h, capi.ptr(conf, ctypes.c_longlong), ctypes.byref(ni), ctypes.byref(npx)) == 0
    assert not conf.any() and (ni.value, npx.value) == (0, 0)
    f.score_reset()
    s = f.score_get()
    assert s.conf.shape == (25, 25) and not s.conf.any() and np.isnan(s.accuracy)
