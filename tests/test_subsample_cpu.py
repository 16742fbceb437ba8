"""The restatement of the subsampling rule (tests/subsample_restatement.py) against the host code that states it today
(tracker.subsample, subsample_depth, reinit_state, frame_decision), bit for bit, and the new entry points' presence in the
header, the binding and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import subsample_restatement as sr
from avatar_amd import capi, subsample, tracker
from avatar_amd.depth import depth_to_xyz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = 6


def _image(rng, rows, cols, fill=0.4):
    lab = np.where(rng.random((rows, cols)) < fill, rng.integers(0, PARTS, (rows, cols)), 255).astype(np.uint8)
    xyz = rng.standard_normal((rows, cols, 3)).astype(np.float32)
    xyz[rng.random((rows, cols)) < 0.05] = [np.nan, -0.0, np.inf]
    return xyz, lab


def _boxes(rng, rows, cols):
    yield (0, 0, cols - 1, rows - 1)
    yield (cols - 1, rows - 1, cols - 1, rows - 1)
    yield (cols - 1, rows - 1, 0, 0)                          # empty, as the background subtractor leaves it
    for _ in range(6):
        x0, x1 = sorted(rng.integers(0, cols, 2).tolist())
        y0, y1 = sorted(rng.integers(0, rows, 2).tolist())
        yield (x0, y0, x1, y1)


@pytest.mark.parametrize("interval", [1, 2, 3, 12])
def test_restatement_is_tracker_subsample(interval):
    rng = np.random.default_rng(100 + interval)
    for rows, cols in ((37, 53), (24, 25)):
        xyz, lab = _image(rng, rows, cols)
        for box in _boxes(rng, rows, cols):
            d, l = sr.subsample(xyz, lab, box, interval, PARTS)
            wd, wl = tracker.subsample(xyz, lab, (box[1], box[0], box[3], box[2]), interval, PARTS)
            assert d.dtype == wd.dtype and l.dtype == wl.dtype
            assert np.array_equal(sr.bits(d), sr.bits(wd)) and np.array_equal(l, wl), (interval, box)
            row = sr.count_row(l, PARTS)
            assert row[0] == len(wl) and np.array_equal(row[1:], np.bincount(wl, minlength=PARTS))
    xyz, lab = _image(rng, 20, 30)
    whole, _ = sr.subsample(xyz, lab, (0, 0, -1, -1), interval, PARTS)
    assert np.array_equal(sr.bits(whole), sr.bits(tracker.subsample(xyz, lab, None, interval, PARTS)[0]))


@pytest.mark.parametrize("interval", [1, 2, 3, 12])
def test_restatement_is_subsample_depth(interval):
    rng = np.random.default_rng(200 + interval)
    rows, cols = 37, 53
    _, lab = _image(rng, rows, cols)
    depth = rng.uniform(0.5, 4.0, (rows, cols)).astype(np.float32)
    k = (505.1, 504.7, 26.3, 18.9)
    xyz = depth_to_xyz(depth, k)
    for box in _boxes(rng, rows, cols):
        d, l = sr.subsample(xyz, lab, box, interval, PARTS)
        wd, wl = tracker.subsample_depth(depth, k, lab, (box[1], box[0], box[3], box[2]), interval, PARTS)
        assert np.array_equal(sr.bits(d), sr.bits(wd)) and np.array_equal(l, wl), (interval, box)


def test_bad_label_is_refused_by_both():
    rng = np.random.default_rng(5)
    xyz, lab = _image(rng, 10, 12)
    lab[4, 6] = PARTS
    with pytest.raises(ValueError):
        sr.subsample(xyz, lab, (0, 0, 11, 9), 2, PARTS)
    with pytest.raises(ValueError):
        tracker.subsample(xyz, lab, (0, 0, 9, 11), 2, PARTS)
    sr.subsample(xyz, lab, (0, 0, 11, 9), 4, PARTS)           # (4, 6) is not on this grid


def test_centroid_is_reinit_state():
    rng = np.random.default_rng(6)
    for n in (1, 2, 3, 7, 8, 9, 63, 64, 65, 1000, 20001):
        data = np.ascontiguousarray(rng.standard_normal((n, 3)) * rng.choice([1e-3, 1.0, 1e3], (n, 1)))
        assert np.array_equal(sr.bits(sr.centroid(data)), sr.bits(np.ascontiguousarray(tracker.reinit_state(data, 24, 10)[0]))), n


class _Policy:
    def __init__(self, **kw):
        self.interval, self.frameICPIters, self.reinitICPIters, self.reinitCnz = 2, 3, 6, 40
        self.initialPerPartCnz, self.initialICPIters, self.firstTime, self.reinit = 0, 8, True, True
        self.__dict__.update(kw)


def test_count_rows_drive_frame_decision_like_label_vectors():
    rng = np.random.default_rng(7)
    for per_part in (0, 8):
        a, b = _Policy(initialPerPartCnz=per_part), _Policy(initialPerPartCnz=per_part)
        answers = []
        for step in range(40):
            n = int(rng.choice([0, 3, 9, 10, 11, 40, 200]))
            labels = rng.integers(0, PARTS if step % 3 else PARTS - 1, n).astype(np.int32)      # sometimes a part is missing
            got = tracker.frame_decision(a, None, PARTS, counts=sr.count_row(labels, PARTS))
            want = tracker.frame_decision(b, labels, PARTS)
            assert got == want and (a.reinit, a.firstTime) == (b.reinit, b.firstTime), (per_part, step)
            answers.append(want)
        assert {x[0] for x in answers} == {True, False} and any(x[2] for x in answers)


def test_new_symbols_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "avt_subsample.h")).read()
    declared = set(re.findall(r"\b(avt_[a-z_]+)\s*\(", hdr))
    assert declared == set(subsample.SUBSAMPLE_SYMBOLS), declared ^ set(subsample.SUBSAMPLE_SYMBOLS)
    assert hdr.count("demo.cpp:216-250") >= len(declared)     # every entry cites what it stands for
    assert os.path.exists(capi.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in declared:
        assert hasattr(lib, s), s
    chunk, width = ctypes.c_int(), ctypes.c_int()
    assert lib.avt_frames_subsample_constants(ctypes.byref(chunk), ctypes.byref(width)) == 0
    assert (chunk.value, width.value) == tuple(int(v) for v in re.findall(r"#define AVT_SUBSAMPLE_(?:CHUNK|SCAN_WIDTH) (\d+)", hdr))
