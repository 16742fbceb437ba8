"""Two CPU restatements of BGSubtractor::run (BGSubtractor.cpp:10-163) in numpy float32, the yardstick of the GPU
background subtraction (include/avt_bgsub.h).  A helper module of the tests, not a test file.

  literal(...)  the reference's own order: the near-background test per pixel (:30-80), then the raster scan with an
                explicit stack (:82-126), then the box (:128-151).  For small images.
  fast(...)     the same result from whole-array operations: the near test over the nine window offsets, components by
                scipy.sparse.csgraph.connected_components on the 4-neighbour edge graph, ids from every component's
                smallest raster index.  For 1280x720.

Both return a dict: mask (uint8), top_left / bot_right ((x, y)), capped, comps (list of (size, id), sorted as
comps_by_size unless capped), masked_depth (float32) and fg_count (demo.cpp:183-192, live-demo.cpp:317-332)."""
from __future__ import annotations

import numpy as np

UNVISITED, INVALID = 254, 255


def thresholds(rows, cols, nn_rel, neighb_rel):
    """1200000.0 / (rows * cols) * rel in double (int product, float member promoted), rounded to float by ffill's
    parameter (:160-161)."""
    n = rows * cols
    return (np.float32(1200000.0 / n * float(np.float32(nn_rel))), np.float32(1200000.0 / n * float(np.float32(neighb_rel))))


def min_points(rows, cols):
    return max(rows * cols // 1000, 100)                      # :19


def _sq(a, b):
    d = (a - b).astype(np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _finish(mask, image, capped, comps, prev_box):
    rows, cols = mask.shape
    if capped:                                                # :124 returns before the box is recomputed
        tl, br = prev_box
    else:
        fg = mask != INVALID
        tl, br = (cols - 1, rows - 1), (0, 0)
        if fg.any():
            rr = np.nonzero(fg.any(axis=1))[0]
            cc = np.nonzero(fg.any(axis=0))[0]
            tl, br = (int(cc.min()), int(rr.min())), (int(cc.max()), int(rr.max()))
        comps = sorted(comps, reverse=True)                   # std::greater<std::array<int, 2>> (:153)
    depth = np.ascontiguousarray(image[:, :, 2], np.float32).copy()
    inside = np.zeros(mask.shape, bool)
    if tl[1] <= br[1] and tl[0] <= br[0]:
        inside[tl[1]:br[1] + 1, tl[0]:br[0] + 1] = True
    depth[inside & (mask >= UNVISITED)] = 0.0
    fg_count = int((inside & (mask < UNVISITED)).sum())
    return dict(mask=mask, top_left=tuple(tl), bot_right=tuple(br), capped=capped, comps=[tuple(c) for c in comps], masked_depth=depth,
                fg_count=fg_count)


def literal(background, image, nn_rel=0.005, neighb_rel=0.005, prev_box=((0, 0), (0, 0))):
    bg = np.asarray(background, np.float32)
    im = np.asarray(image, np.float32)
    rows, cols = im.shape[:2]
    nn, nb = thresholds(rows, cols, nn_rel, neighb_rel)
    min_pts = min_points(rows, cols)
    mask = np.full((rows, cols), UNVISITED, np.uint8)
    for r in range(rows):                                     # :56-71 (window size 1, clipped :33-34)
        for c in range(cols):
            v = im[r, c]
            if v[2] == 0:
                mask[r, c] = INVALID
                continue
            for rr in range(max(r - 1, 0), min(r + 1, rows - 1) + 1):
                hit = False
                for cc in range(max(c - 1, 0), min(c + 1, cols - 1) + 1):
                    nbv = bg[rr, cc]
                    if nbv[2] == 0:
                        continue
                    d = nbv - v
                    if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] < nn:
                        hit = True
                        break
                if hit:
                    mask[r, c] = INVALID
                    break
    comps, compid = [], 0
    for r in range(rows):                                     # :95-126
        for c in range(cols):
            if mask[r, c] != UNVISITED:
                continue
            mask[r, c] = compid
            stk, vis = [(r, c)], [(r, c)]
            while stk:
                cr, cc = stk.pop()
                val = im[cr, cc]
                for nr, nc in ((cr - 1, cc), (cr + 1, cc), (cr, cc - 1), (cr, cc + 1)):
                    if nr < 0 or nr >= rows or nc < 0 or nc >= cols or mask[nr, nc] != UNVISITED:
                        continue
                    d = val - im[nr, nc]
                    if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > nb:
                        continue
                    mask[nr, nc] = compid
                    vis.append((nr, nc))
                    stk.append((nr, nc))
            if len(vis) < min_pts:
                for vr, vc in vis:
                    mask[vr, vc] = INVALID
            else:
                comps.append((len(vis), compid))
                compid += 1
            if compid == UNVISITED:
                return _finish(mask, im, True, comps, prev_box)
    return _finish(mask, im, False, comps, prev_box)


def near_background(bg, im, nn):
    """candidate pixels of the near-background test (:30-76)"""
    rows, cols = im.shape[:2]
    hit = np.zeros((rows, cols), bool)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            r0, r1 = max(0, -dr), rows - max(0, dr)           # pixels whose neighbour (r + dr, c + dc) lies in the image
            c0, c1 = max(0, -dc), cols - max(0, dc)
            nbv = bg[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
            v = im[r0:r1, c0:c1]
            hit[r0:r1, c0:c1] |= (nbv[..., 2] != 0) & (_sq(nbv, v) < nn)
    return (im[..., 2] != 0) & ~hit


def fast(background, image, nn_rel=0.005, neighb_rel=0.005, prev_box=((0, 0), (0, 0))):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    bg = np.asarray(background, np.float32)
    im = np.asarray(image, np.float32)
    rows, cols = im.shape[:2]
    n = rows * cols
    nn, nb = thresholds(rows, cols, nn_rel, neighb_rel)
    cand = near_background(bg, im, nn)
    idx = np.arange(n).reshape(rows, cols)
    # 4-neighbour edges between candidates, joined unless the squared distance is > neighb (:86; NaN joins)
    eh = cand[:, :-1] & cand[:, 1:] & ~(_sq(im[:, :-1], im[:, 1:]) > nb)
    ev = cand[:-1, :] & cand[1:, :] & ~(_sq(im[:-1, :], im[1:, :]) > nb)
    a = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
    b = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    cflat = cand.ravel()
    cl = lab[cflat]
    pix = np.nonzero(cflat)[0]
    ncomp = int(lab.max()) + 1 if n else 0
    first = np.full(ncomp, n, np.int64)
    np.minimum.at(first, cl, pix)
    size = np.bincount(cl, minlength=ncomp)
    present = size > 0
    kept = present & (size >= min_points(rows, cols))
    kept_ids = np.nonzero(kept)[0]
    order = kept_ids[np.argsort(first[kept_ids], kind="stable")]   # the scan reaches components by their first pixel
    code = np.full(ncomp, INVALID, np.int32)
    capped = len(order) >= UNVISITED
    if capped:
        cap_first = first[order[UNVISITED - 1]]
        code[present & (first > cap_first)] = UNVISITED
        order = order[:UNVISITED]
    code[order] = np.arange(len(order))
    mask = np.full(n, INVALID, np.uint8)
    mask[pix] = code[cl].astype(np.uint8)
    comps = [(int(size[c]), i) for i, c in enumerate(order)]
    return _finish(mask.reshape(rows, cols), im, capped, comps, prev_box)


def same(a, b):
    """the two results agree bit for bit (masked depth compared as bits)"""
    return (np.array_equal(a["mask"], b["mask"]) and a["top_left"] == b["top_left"] and a["bot_right"] == b["bot_right"] and
            a["capped"] == b["capped"] and a["comps"] == b["comps"] and a["fg_count"] == b["fg_count"] and
            np.array_equal(a["masked_depth"].view(np.uint32), b["masked_depth"].view(np.uint32)))
