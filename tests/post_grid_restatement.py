"""Restatement of the device post-processing rule (include/avt_rtree.h): connected components per part on the
interval grid, written with numpy and scipy.ndimage.label and sharing no code with avatar_amd/csrc/avt_post.hip.

post_process(image, box, interval, com_pre, weight, num_parts, ptype) -> (image', com_pre')
    image     (rows, cols) uint8, 255 = background; not modified
    box       (tl.x, tl.y, br.x, br.y) inclusive; br.x == -1: the whole image; empty or not inside the image: labels untouched
    com_pre   (2, num_parts) float64 or None (not sized yet)
    ptype     0 contiguous, 1 disjoint
A label that is neither 255 nor < num_parts raises ValueError.
"""
import numpy as np
from scipy import ndimage


def _sized(com_pre, num_parts):
    if com_pre is None:
        c = np.zeros((2, num_parts))
        c[0] = -1.0
        return c
    return np.array(com_pre, np.float64)


def grid_of(image, box, interval):
    tlx, tly, brx, bry = box
    return image[tly:bry + 1:interval, tlx:brx + 1:interval]


def post_process(image, box, interval, com_pre, weight, num_parts, ptype):
    rows, cols = image.shape
    tlx, tly, brx, bry = (int(v) for v in box)
    if brx == -1:
        brx, bry = cols - 1, rows - 1
    out = image.copy()
    com = _sized(com_pre, num_parts)
    if not (0 <= tlx <= brx < cols and 0 <= tly <= bry < rows):
        if ptype == 0:
            com[0] = -1.0
        return out, com
    iv = int(interval)
    grid = image[tly:bry + 1:iv, tlx:brx + 1:iv].copy()
    if ((grid != 255) & (grid >= num_parts)).any():
        raise ValueError("label out of range")
    gh, gw = grid.shape
    flat = np.arange(gh * gw, dtype=np.int64).reshape(gh, gw)
    jj, ii = np.meshgrid(np.arange(gw, dtype=np.int64), np.arange(gh, dtype=np.int64))
    min_size = int((rows * cols // (iv * iv)) * 0.0005)
    for part in np.unique(grid[grid != 255]).tolist() if ptype == 0 else []:
        sel = grid == part
        lab, n = ndimage.label(sel)                       # 4-connected
        l = lab[sel]
        size = np.bincount(l, minlength=n + 1)
        sj = np.zeros(n + 1, np.int64); si = np.zeros(n + 1, np.int64)
        np.add.at(sj, l, jj[sel]); np.add.at(si, l, ii[sel])
        first = np.full(n + 1, gh * gw, np.int64)
        np.minimum.at(first, l, flat[sel])
        best, best_score, best_com = 0, 0.0, None
        for k in sorted(range(1, n + 1), key=lambda k: first[k]):          # raster order of the first pixel: ties keep the earlier
            nk = float(size[k])
            cx = float(int(size[k]) * tlx + iv * int(sj[k])) / nk
            cy = float(int(size[k]) * tly + iv * int(si[k])) / nk
            score = nk
            if com[0, part] >= 0.0:
                dx, dy = cx - float(com[0, part]), cy - float(com[1, part])
                score -= (dx * dx + dy * dy) * float(weight)
            if score > best_score:
                best, best_score, best_com = k, score, (cx, cy)
        grid[sel & (lab != best)] = 255
        if best:
            com[0, part], com[1, part] = best_com
        else:
            com[0, part] = -1.0
    if ptype == 0:
        present = np.zeros(num_parts, bool)
        present[np.unique(grid[grid != 255])] = True
        com[0, ~present] = -1.0                           # a part without a winner; y stays
    else:
        for part in np.unique(grid[grid != 255]).tolist():
            sel = grid == part
            lab, n = ndimage.label(sel)
            size = np.bincount(lab[sel], minlength=n + 1)
            grid[sel & (size[lab] < min_size)] = 255
    # upscaleGrid: grid row tl.y is written back as it is, the rows below fill their cells (clamped to br.y and to the image width)
    out[tly, tlx:brx + 1:iv] = grid[0]
    if iv == 1:
        out[tly:bry + 1, tlx:brx + 1] = grid
    elif gh > 1:
        block = np.repeat(np.repeat(grid[1:], iv, 0), iv, 1)
        r0, c1 = tly + iv, min(tlx + gw * iv - 1, cols - 1)
        out[r0:bry + 1, tlx:c1 + 1] = block[:bry + 1 - r0, :c1 + 1 - tlx]
    return out, com
