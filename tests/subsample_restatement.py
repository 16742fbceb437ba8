"""The trackers' interval subsampling (demo.cpp:216-250, :253) restated as plain loops, independent of avatar_amd.tracker: the
reference of tests/test_subsample_cpu.py (which ties it to tracker.subsample / subsample_depth / reinit_state bit for bit) and
of tests/test_gpu_subsample.py (the device stage).  A box is (tl.x, tl.y, br.x, br.y), inclusive, as the C ABI has it; br.x == -1
is the whole image."""
import numpy as np


def grid(box, interval, rows, cols):
    """[(row, col), ...] of the grid in raster order; a box with tl > br in either axis has none; any other box must lie inside"""
    tlx, tly, brx, bry = (int(v) for v in box)
    if brx == -1:
        tlx, tly, brx, bry = 0, 0, cols - 1, rows - 1
    if tlx > brx or tly > bry:
        return []
    assert 0 <= tlx and 0 <= tly and brx < cols and bry < rows and interval >= 1, (box, interval)
    out = []
    r = tly
    while r <= bry:
        c = tlx
        while c <= brx:
            out.append((r, c))
            c += interval
        r += interval
    return out


def subsample(xyz, labels, box, interval, num_parts):
    """(data (n, 3) float64, labels (n,) int32) of one image: xyz (rows, cols, 3) float32, labels (rows, cols) uint8.
    Raises ValueError on a kept label >= num_parts (demo.cpp:236-243)."""
    rows, cols = labels.shape
    lab = labels.tolist()
    kept = []
    for r, c in grid(box, interval, rows, cols):
        l = lab[r][c]
        if l == 255:
            continue
        if l >= num_parts:
            raise ValueError("body part label out of range")
        kept.append((r, c, l))
    if not kept:
        return np.empty((0, 3), np.float64), np.empty(0, np.int32)
    rs, cs, ls = (np.array(v, np.int64) for v in zip(*kept))
    data = np.asarray(xyz, np.float32)[rs, cs].astype(np.float64)      # widened first ...
    data[:, 1] = -data[:, 1]                                           # ... then negated (demo.cpp:245)
    return np.ascontiguousarray(data), ls.astype(np.int32)


def count_row(labels, num_parts):
    """[points, points of part 0, ...] as the device table has it"""
    row = [0] * (1 + num_parts)
    for l in np.asarray(labels).tolist():
        row[0] += 1
        row[1 + l] += 1
    return np.array(row, np.int32)


def centroid(data):
    """s = 0; for k in frame order: s += data[k][c]; s / n (demo.cpp:253), Python floats being IEEE doubles"""
    n = len(data)
    out = np.empty(3, np.float64)
    for c in range(3):
        s = 0.0
        for v in data[:, c].tolist():
            s += v
        out[c] = np.float64(s) / np.float64(n)
    return out


def bits(a):
    """the bit patterns of a float64 / int32 array, for comparisons that tell NaN payloads and signed zeros apart"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.int32)
